"""Case tables of tests/test_gpu_ctmul.py, test_gpu_ctmul_footprint.py and test_gpu_ctmul_scale.py,
and a pure-Python mirror of the dispatch behind include/nttmul_ctmul.h (csrc/ctmul.hip high and
relin, csrc/ctmul_plan.hpp ctmul_high_grid and ctmul_relin_grid): plain data and arithmetic, no
GPU.

tests/test_ctmul_ledger.py holds the mirror against the cross-compiled lib/libnttmul_ctmul.so (the
kernels it holds beyond libnttmul_lintrans.so's are exactly the ones the mirror names over these
cases); test_gpu_ctmul.py::test_mirror_agrees_with_the_library_dispatch anchors it on the GPU to
the library's own dry run (nttmul_ctmul_kernel_name).

The shapes are the smallest at which the kernels can go wrong.  A k_ctmul_relin workgroup takes the
same 256 slots of V = 4 consecutive batch entries: batch 1 is one partial workgroup per slot range,
V + 1 a full and a partial one, 2 V - 1 a full one and one with a single dead entry.  A
k_ctmul_high workgroup takes 256 vectors of 16 bytes of one limb's stream [batch][n]: at n = 256
that is 4 whole polynomials on 32-bit words and 2 on 64-bit words, so the same three batches each
end in a partial workgroup there.  n = 256 is one slot range per polynomial (lgs = 0), n = 65536
the widest."""
from collections import namedtuple

import ks_ref

V = 4                                        # csrc/ctmul_plan.hpp kCtSlices
OPS = ("high", "relin")
ALL_N = tuple(1 << e for e in range(8, 17))
PARITY_N = (256, 512, 4096, 8192, 65536)
BATCHES = (1, V + 1, 2 * V - 1)
SHAPES = ((1, 1), (4, 2), (12, 4))           # (L, K)
BIG_N, BIG_SHAPE = 65536, (2, 1)
WORST_N = (256, 4096)
WORST = (16, 16)                             # pairs, terms
WORST_SHAPE = (2, 1)
CHAIN_N = (256, 8192)
VALIDATE = (256, V + 1, (3, 2))              # n, batch, (L, K)
HOST = ((256, V + 1), (8192, 2))             # (n, batch), HOST_SHAPE
HOST_SHAPE = (3, 2)

# A case names its bases (ks_ref.bases(bits, L, K)) and holds no prime.  terms is ignored by high;
# square: y_hat is x_hat
Case = namedtuple("Case", "op bits n batch L K pairs terms square validate", defaults=(False,))

# (batch, (L, K), pairs, terms, square): every value of every factor
ROWS = (
    (1, (1, 1), 1, 1, False),
    (V + 1, (4, 2), 3, 3, False),
    (2 * V - 1, (12, 4), 1, 3, True),
    (V + 1, (1, 1), 3, 1, True),
    (2 * V - 1, (4, 2), 1, 1, False),
    (1, (12, 4), 3, 3, False),
)
BIG_ROWS = (
    (1, BIG_SHAPE, 1, 1, False),
    (V + 1, BIG_SHAPE, 3, 3, True),
    (2 * V - 1, BIG_SHAPE, 1, 3, False),
)


def moduli_of(case):
    """(q, p) of a case."""
    return ks_ref.bases(case.bits, case.L, case.K)


def parity_cases():
    out = []
    for op in OPS:
        for bits in (32, 64):
            for n in PARITY_N:
                for batch, (L, K), pairs, terms, square in (BIG_ROWS if n == BIG_N else ROWS):
                    out.append(Case(op, bits, n, batch, L, K, pairs, terms, square))
    return out


def worst_cases():
    pairs, terms = WORST
    L, K = WORST_SHAPE
    return [Case(op, bits, n, 2, L, K, pairs, terms, False)
            for op in OPS for bits in (32, 64) for n in WORST_N]


# The caller's memory (tests/test_gpu_ctmul_footprint.py): host "" for the *_device call, "host"
# for the host form
Footprint = namedtuple("Footprint", "entry case host", defaults=("",))
FP_SHAPE = (3, 2)
FP_SIZES = ((256, V + 1), (8192, V + 1))     # (n, batch): a partial last workgroup
FP_CALL = (2, 2)                             # pairs, terms


def footprint_cases():
    out = []
    pairs, terms = FP_CALL
    L, K = FP_SHAPE
    for op in OPS:
        for bits in (32, 64):
            for n, batch in FP_SIZES:
                for square in (False, True):
                    case = Case(op, bits, n, batch, L, K, pairs, terms, square)
                    out.append(Footprint(f"nttmul_ctmul_{op}_device", case))
                    out.append(Footprint(f"nttmul_ctmul_{op}", case, "host"))
    return out


def fp_guard_words(case):
    """The guard width tests/guarded.py gives the call: one batch entry of the widest operand."""
    from guarded import guard_words
    return guard_words(max(max(case.terms, 2) * (case.L + case.K), case.pairs * 2 * case.L) * case.n)


# ---------------------------------------------------------------------------------------------
# Scale cases (tests/test_gpu_ctmul_scale.py): the rule of tests/scale_cases.py -- the launch
# holds at least MIN_WAVES = 2 * 8192 waves, with the smallest batch that meets it and, where the
# kernel takes several units per workgroup, a partial last workgroup
# ---------------------------------------------------------------------------------------------

SCALE_N = 4096
SCALE_SHAPE = (2, 1)
SCALE_CALL = (2, 2)                          # pairs, terms
WAVE, MIN_WAVES = 64, 2 * 8192


def ends_partial(case):
    """Every kernel of the case that takes several units per workgroup ends in a partial one."""
    return all(per == 1 or units % per for per, units, _ in units_per_block(case).values())


def scale_cases():
    pairs, terms = SCALE_CALL
    L, K = SCALE_SHAPE
    out = []
    for op in OPS:
        for bits in (32, 64):
            def make(b):
                return Case(op, bits, SCALE_N, b, L, K, pairs, terms, False)
            b = 1
            while min(launch_waves(make(b)).values()) < MIN_WAVES or not ends_partial(make(b)):
                b += 1
            out.append(make(b))
    return out


# up_hat just over 4 GiB, compared with the same call in chunks below 1 GiB
LARGE = (64, 65536, 1, 1, 1, 16)             # bits, n, L, K, pairs, terms
LARGE_BYTES = 1 << 32


def large_case():
    """The smallest batch whose up_hat exceeds 4 GiB."""
    bits, n, L, K, pairs, terms = LARGE
    per = terms * (L + K) * n * (bits // 8)
    return Case("relin", bits, n, LARGE_BYTES // per + 1, L, K, pairs, terms, False)


def referenced_cases():
    """The cases whose every output word a GPU test holds to the CPU reference (tests/full_ref.py):
    all but the scale and the 4 GiB cases, whose batches exist to fill the machine."""
    out = parity_cases() + worst_cases()
    n, batch, (L, K) = VALIDATE
    out += [Case(op, bits, n, batch, L, K, 2, 2, sq, True) for op in OPS for bits in (32, 64)
            for sq in (False, True)]
    out += [Case(op, bits, n, batch, *HOST_SHAPE, 2, 2, False) for op in OPS for bits in (32, 64)
            for n, batch in HOST]
    out += [f.case for f in footprint_cases()]
    return out


def all_cases():
    return referenced_cases() + scale_cases() + [large_case()]


# ---------------------------------------------------------------------------------------------
# The mirror
# ---------------------------------------------------------------------------------------------

def kernel_name(op, bits):
    """ctmul.hip high / relin: one kernel per operation at every n; the class follows the word
    size alone.  What nttmul_ctmul_kernel_name returns."""
    assert op in OPS and bits in (32, 64)
    cls, io = ("Arith32P", "u32") if bits == 32 else ("Arith64", "u64")
    return f"k_ctmul_{op}<{cls},{io}>"


def relin_grid(batch, n, v=V):
    """ctmul_plan.hpp ctmul_relin_grid (lintrans_grid, batch-sliced): a unit is a batch entry, a
    workgroup takes V consecutive ones at one range of 256 slots; wgx = ceil(units / V) (n / 256)
    workgroups per limb; tail: the live entries of the last, partial run (0: every run is full)."""
    assert n in ALL_N, "n > 65536 is NTTMUL_EUNSUPPORTED"
    groups = -(-batch // v)
    return dict(units=batch, groups=groups, wgx=groups * (n // 256), tail=batch % v)


def vec_words(bits):
    """Words of one 16-byte access of k_ctmul_high."""
    return 128 // bits


def high_grid(batch, n, bits):
    """ctmul_plan.hpp ctmul_high_grid: a lane takes one vector, a workgroup 256 consecutive
    vectors of one limb's stream [batch][n]: per = max(1, 256 vec / n) whole polynomials or one of
    n / (256 vec) parts of one; tail: the vectors of the last, partial workgroup."""
    assert n in ALL_N, "n > 65536 is NTTMUL_EUNSUPPORTED"
    vec = vec_words(bits)
    pv = n // vec
    vectors = batch * pv
    return dict(vectors=vectors, wgx=-(-vectors // 256), vec=vec, per=max(1, 256 // pv),
                tail=vectors % 256)


def kernels_of(case):
    """The kernel_keys `case` launches, in launch order: with NTTMUL_FLAG_VALIDATE the range check
    (libnttmul_rns.so's kernel: once each for up_hat and key_hat of relin, once for x_hat and once
    more for a y_hat that is not x_hat), then the one kernel."""
    q, p = moduli_of(case)
    assert (len(q), len(p)) == (case.L, case.K)
    io = "u32" if case.bits == 32 else "u64"
    count = (2 if case.op == "relin" else 0) + (1 if case.square else 2)
    return [f"k_rns_check_range<{io}>"] * (count * case.validate) + [kernel_name(case.op, case.bits)]


def units_per_block(case):
    """{kernel_key: (units per workgroup and grid row, units of the launch per grid row, words per
    unit and workgroup)}.  relin: V batch entries, 256 slots of each.  high: a unit is a
    polynomial of the limb's stream; per whole ones where 256 vectors hold several (n words of
    each), else one (the 256 vec words of the workgroup's part)."""
    key = kernel_name(case.op, case.bits)
    if case.op == "relin":
        return {key: (V, case.batch, 256)}
    g = high_grid(case.batch, case.n, case.bits)
    return {key: (g["per"], case.batch, min(case.n, 256 * g["vec"]))}


def grid_rows(case):
    """{kernel_key: gridDim.y}: the L + K limbs for relin, the L limbs of Q for high."""
    return {kernel_name(case.op, case.bits): case.L + (case.K if case.op == "relin" else 0)}


def bpu(case):
    """Workgroups per run of units: the n / 256 slot ranges (relin), the parts of a polynomial
    (high)."""
    if case.op == "relin":
        return case.n // 256
    return max(1, case.n // (256 * vec_words(case.bits)))


def launch_waves(case):
    rows = grid_rows(case)
    return {k: -(-units // per) * bpu(case) * rows[k] * (256 // WAVE)
            for k, (per, units, _) in units_per_block(case).items()}


def launches(n, rescale=False):
    """Launches of multiply, relinearise and (with the merged context) rescale: high -> modup ->
    relin -> mdntt_moddown is 1 + 2 + 1 + 2, or 1 + 4 + 1 + 4 above n = 4096, either way."""
    return 6 if n <= 4096 else 10


def relin_byte_units(L, K, pairs, terms):
    """Limb polynomials relin moves per batch entry: terms of up_hat and 2 of c_hat over L + K
    limbs, 4 pairs of x_hat and y_hat over L.  (The key is shared by the batch and amortised
    away.)"""
    return (terms + 2) * (L + K) + 4 * pairs * L


def high_byte_units(L, pairs):
    """Limb polynomials high moves per batch entry: 2 pairs read, 1 written, over L limbs."""
    return (2 * pairs + 1) * L


# Kernels of libnttmul_ctmul.so beyond libnttmul_lintrans.so's that no call can launch.  None:
# ctmul.hip instantiates only what dispatch reaches.
UNREACHABLE = ()
