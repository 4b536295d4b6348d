"""Case tables of tests/test_gpu_lintrans.py, test_gpu_lintrans_footprint.py and
test_gpu_lintrans_scale.py, and a pure-Python mirror of the dispatch behind
include/nttmul_lintrans.h (csrc/lintrans.hip apply, csrc/lintrans_plan.hpp lintrans_grid): plain
data and arithmetic, no GPU.

tests/test_lintrans_ledger.py holds the mirror against the cross-compiled
lib/libnttmul_lintrans.so (the kernels it holds beyond libnttmul_ksntt.so's are exactly the ones the
mirror names over these cases); test_gpu_lintrans.py::test_mirror_agrees_with_the_library_dispatch
anchors it on the GPU to the library's own dry run (nttmul_lintrans_kernel_name).

The shapes are the smallest at which the kernel can go wrong.  A workgroup takes the same 256 slots
of V = 4 consecutive batch entries: batch 1 is one partial workgroup per slot range, V + 1 a full
and a partial one, 2 V - 1 a full one and one with a single dead entry (blockIdx.x = run
(n / 256) + range: the range of 256 slots is the faster index).  n = 256 is one slot range
per polynomial (lgs = 0), n = 65536 the widest slot shift (sh = 16)."""
from collections import namedtuple

import ks_ref

V = 4                                        # csrc/lintrans_plan.hpp kLtSlices
MAX_COMPS, MAX_ROTS = 2, 16                  # NTTMUL_MACN_MAX_COMPS, NTTMUL_HOIST_MAX_ROTS
ALL_N = tuple(1 << e for e in range(8, 17))
PARITY_N = (256, 512, 4096, 8192, 65536)
BATCHES = (1, V + 1, 2 * V - 1)
SHAPES = ((1, 1), (4, 2), (12, 4))           # (L, K)
BIG_N, BIG_SHAPE, BIG_MAX_ROTS = 65536, (2, 1), 3
WORST_N = (256, 4096)
WORST = (16, 16, 2)                          # rots, terms, comps
WORST_SHAPE = (2, 1)
CHAIN_N = (256, 8192)
VALIDATE = (256, V + 1, (3, 2))              # n, batch, (L, K)
HOST = ((256, V + 1), (8192, 2))             # (n, batch), HOST_SHAPE
HOST_SHAPE = (3, 2)

# A case names its bases (ks_ref.bases(bits, L, K)) and holds no prime
Case = namedtuple("Case", "bits n batch L K terms comps ks weighted c0 validate",
                  defaults=(False,))


def pool(n):
    """The rotations the cases draw from."""
    return (1, 5, 25, 2 * n - 1)


def k_list(n, kind):
    """one: the identity; step: one real permutation; two: two distinct ones; twice: a repeated
    element; three: a repeated element and the conjugation; many: sixteen, every pool element four
    times over."""
    one, five, sq, conj = pool(n)
    ks = {"one": (one,), "step": (five,), "two": (sq, conj), "twice": (five, five),
          "three": (five, five, conj), "many": (one, five, sq, conj) * 4}[kind]
    assert all(k % 2 == 1 and 0 < k < 2 * n for k in ks) and len(ks) <= MAX_ROTS
    return ks


# (batch, (L, K), terms, comps, k list, weighted, c0): every value of every factor, every kernel
# instantiation with and without c0
ROWS = (
    (1, (1, 1), 1, 1, "one", False, False),
    (V + 1, (4, 2), 3, 2, "two", True, True),
    (2 * V - 1, (12, 4), 1, 2, "many", True, False),
    (V + 1, (1, 1), 3, 1, "many", False, True),
    (2 * V - 1, (4, 2), 1, 1, "twice", True, True),
    (1, (4, 2), 3, 2, "step", False, True),
    (V + 1, (1, 1), 1, 1, "two", True, False),
    (2 * V - 1, (1, 1), 3, 2, "step", False, False),
)
BIG_ROWS = (
    (1, BIG_SHAPE, 1, 1, "one", False, False),
    (V + 1, BIG_SHAPE, 3, 2, "two", True, True),
    (2 * V - 1, BIG_SHAPE, 1, 2, "three", True, False),
    (V + 1, BIG_SHAPE, 3, 1, "step", False, True),
)


def moduli_of(case):
    """(q, p) of a case."""
    return ks_ref.bases(case.bits, case.L, case.K)


def parity_cases():
    out = []
    for bits in (32, 64):
        for n in PARITY_N:
            for batch, (L, K), terms, comps, kind, weighted, c0 in (BIG_ROWS if n == BIG_N else ROWS):
                out.append(Case(bits, n, batch, L, K, terms, comps, k_list(n, kind), weighted, c0))
    return out


def worst_cases():
    rots, terms, comps = WORST
    L, K = WORST_SHAPE
    return [Case(bits, n, 2, L, K, terms, comps, k_list(n, "many"), True, True)
            for bits in (32, 64) for n in WORST_N]


# The caller's memory (tests/test_gpu_lintrans_footprint.py): host "" for the *_device call, "host"
# for the host form
Footprint = namedtuple("Footprint", "entry case host", defaults=("",))
FP_SHAPE = (3, 2)
FP_SIZES = ((256, V + 1), (8192, V + 1))     # (n, batch): a partial last workgroup
FP_CALL = (2, 2, (5, 1))                     # terms, comps, ks
FP_OPTIONAL = ((True, True), (False, False), (True, False), (False, True))   # (w_hat, c0_hat) given


def footprint_cases():
    out = []
    terms, comps, ks = FP_CALL
    L, K = FP_SHAPE
    for bits in (32, 64):
        for n, batch in FP_SIZES:
            for weighted, c0 in FP_OPTIONAL:
                case = Case(bits, n, batch, L, K, terms, comps, ks, weighted, c0)
                out.append(Footprint("nttmul_lintrans_apply_device", case))
                out.append(Footprint("nttmul_lintrans_apply", case, "host"))
    return out


def fp_guard_words(case):
    """The guard width tests/guarded.py gives the call: one batch entry of the widest operand."""
    from guarded import guard_words
    return guard_words(max(case.terms, case.comps) * (case.L + case.K) * case.n)


# ---------------------------------------------------------------------------------------------
# Scale cases (tests/test_gpu_lintrans_scale.py): the rule of tests/scale_cases.py -- the launch
# holds at least MIN_WAVES = 2 * 8192 waves, with the smallest batch that meets it and a partial
# last workgroup
# ---------------------------------------------------------------------------------------------

SCALE_N = 4096
SCALE_SHAPE = (2, 1)
SCALE_CALL = (2, 2, (5, 25))                 # terms, comps, ks; weights and c0 on
WAVE, MIN_WAVES = 64, 2 * 8192


def scale_cases():
    terms, comps, ks = SCALE_CALL
    L, K = SCALE_SHAPE
    out = []
    for bits in (32, 64):
        def make(b):
            return Case(bits, SCALE_N, b, L, K, terms, comps, ks, True, True)
        b = 1
        while min(launch_waves(make(b)).values()) < MIN_WAVES or grid(b, SCALE_N)["tail"] == 0:
            b += 1
        out.append(make(b))
    return out


# a_hat just over 4 GiB, compared with the same call in chunks below 1 GiB
LARGE = (64, 65536, 1, 1, 16, 1, (5,))       # bits, n, L, K, terms, comps, ks
LARGE_BYTES = 1 << 32


def large_case():
    """The smallest batch whose a_hat exceeds 4 GiB."""
    bits, n, L, K, terms, comps, ks = LARGE
    per = terms * (L + K) * n * (bits // 8)
    return Case(bits, n, LARGE_BYTES // per + 1, L, K, terms, comps, ks, True, True)


def referenced_cases():
    """The cases whose every output word a GPU test holds to the CPU reference (tests/full_ref.py):
    all but the scale and the 4 GiB cases, whose batches exist to fill the machine."""
    out = parity_cases() + worst_cases()
    n, batch, (L, K) = VALIDATE
    out += [Case(bits, n, batch, L, K, 2, 1, (5,), True, True, True) for bits in (32, 64)]
    out += [Case(bits, n, batch, *HOST_SHAPE, 2, 2, (5, 1), True, True) for bits in (32, 64)
            for n, batch in HOST]
    out += [f.case for f in footprint_cases()]
    return out


def all_cases():
    return referenced_cases() + scale_cases() + [large_case()]


# ---------------------------------------------------------------------------------------------
# The mirror
# ---------------------------------------------------------------------------------------------

def kernel_name(bits, comps, weighted):
    """lintrans.hip apply_comps: one kernel at every n; the class follows the word size alone, the
    last two arguments are the component count and whether w_hat is given.  What
    nttmul_lintrans_kernel_name returns."""
    assert bits in (32, 64) and 1 <= comps <= MAX_COMPS
    cls, io = ("Arith32P", "u32") if bits == 32 else ("Arith64", "u64")
    return f"k_lintrans<{cls},{io},{comps},{int(bool(weighted))}>"


def grid(batch, n, v=V):
    """lintrans_plan.hpp lintrans_grid, batch-sliced: a unit is a batch entry, a workgroup takes V
    consecutive ones at one range of 256 slots; wgx = ceil(units / V) (n / 256) workgroups per
    limb; tail: the live entries of the last, partial run (0: every run is full)."""
    assert n in ALL_N, "n > 65536 is NTTMUL_EUNSUPPORTED"
    groups = -(-batch // v)
    return dict(units=batch, groups=groups, wgx=groups * (n // 256), tail=batch % v)


def kernels_of(case):
    """The kernel_keys `case` launches, in launch order: with NTTMUL_FLAG_VALIDATE the range check
    (libnttmul_rns.so's kernel: once each for a_hat and b_hat, once more for each of w_hat and
    c0_hat that is given), then the one kernel."""
    q, p = moduli_of(case)
    assert (len(q), len(p)) == (case.L, case.K)
    io = "u32" if case.bits == 32 else "u64"
    checks = [f"k_rns_check_range<{io}>"] * ((2 + case.weighted + case.c0) * case.validate)
    return checks + [kernel_name(case.bits, case.comps, case.weighted)]


def units_per_block(case):
    """{kernel_key: (units per workgroup and grid row, units of the launch per grid row, words per
    unit and workgroup)}: V batch entries, 256 slots of each."""
    return {kernel_name(case.bits, case.comps, case.weighted): (V, case.batch, 256)}


def grid_rows(case):
    """{kernel_key: gridDim.y}: the L + K limbs."""
    return {kernel_name(case.bits, case.comps, case.weighted): case.L + case.K}


def bpu(case):
    """Workgroups per run of V entries: the n / 256 slot ranges."""
    return case.n // 256


def launch_waves(case):
    rows = grid_rows(case)
    return {k: -(-units // per) * bpu(case) * rows[k] * (256 // WAVE)
            for k, (per, units, _) in units_per_block(case).items()}


def launches(n):
    """Launches of the linear transform modup -> apply -> mdntt_moddown, for any number of
    rotations: 2 + 1 + 2, or 4 + 1 + 4 above n = 4096."""
    return 5 if n <= 4096 else 9


def moddown_polys(batch, rots, summed=True):
    """Polynomials ModDown reads: batch 2 after apply, batch rots 2 after ksntt_mac."""
    return batch * 2 if summed else batch * rots * 2


def byte_units(terms, rots, comps, summed=True):
    """Limb polynomials moved per input and limb by the bound the issue states: the summed form
    reads terms of a_hat and writes comps, k_ksntt_mac reads terms and writes rots comps.  (The
    keys are shared by the batch and amortised away.)"""
    return terms + (comps if summed else rots * comps)


# Kernels of libnttmul_lintrans.so beyond libnttmul_ksntt.so's that no call can launch.  None:
# lintrans.hip instantiates only what dispatch reaches.
UNREACHABLE = ()
