"""Case tables of tests/test_gpu_level.py, test_gpu_level_footprint.py and test_gpu_level_scale.py,
and a pure-Python mirror of the dispatch behind include/nttmul_level.h (csrc/level.hip,
csrc/level_plan.hpp): plain data and arithmetic, no GPU.

tests/test_level_ledger.py holds the mirror against the cross-compiled lib/libnttmul_level.so (the
kernels it holds beyond libnttmul_xconv.so's are exactly the ones the mirror names over these
cases); test_gpu_level.py anchors it on the GPU to the library's own dry run
(nttmul_level_kernel_name).

The chain of every case: L_TOP = 5 limbs of Q, K = 2 of P, digits of ALPHA = 2, so a top-level key
has TOP_TERMS = 3 terms over 7 limbs.  A context at level L has the first L limbs of Q, the same P,
digits of min(ALPHA, L) and terms(L) = ceil(L / ALPHA) terms: 5 is the identity view, 4 drops a
limb, 3 ends in a partial digit, 1 is below the digit width."""
from collections import namedtuple

import basis_cases as BC

OPS = ("mac", "lintrans", "relin")            # nttmul_level_kernel_name's numbering
L_TOP, K, ALPHA = 5, 2, 2
TOP_TERMS = -(-L_TOP // ALPHA)
VIEW = (L_TOP, TOP_TERMS)
LEVELS = (5, 4, 3, 1)
PROFILE = {32: "chain32", 64: "chain64"}      # mixed, unsorted limb sizes
ALL_N = (256, 512, 8192)
COMPS = (1, 2)
ROTS = (1, 3)
PAIRS = (1, 3)
V = 4                                         # entries or slices a workgroup takes, every kernel
CHAIN_N = (256, 8192)
CHAIN_LEVEL = 3
CHAIN_H = 8                                   # Hamming weight of the chain's secrets

Case = namedtuple("Case", "op bits n batch L comps rots weighted c0 pairs validate",
                  defaults=(1, 1, False, False, 1, False))


def batch_of(n):
    """5 at n = 256 and 3 elsewhere: both leave a partial last workgroup for the kernels that take
    V = 4 batch entries.  k_level_mac takes V slices of 256 slots, batch n / 256 of them: 5 at
    n = 256 and 6 at n = 512 end partial, the 96 at n = 8192 do not (no batch does there)."""
    return 5 if n == 256 else 3


def chain_bases(bits):
    """(q, p) of the whole chain."""
    return BC.basis(PROFILE[bits], L_TOP, K)


def level_bases(bits, L):
    q, p = chain_bases(bits)
    return q[:L], p


def alpha_of(L):
    return min(ALPHA, L)


def terms_of(L):
    return -(-L // ALPHA)


def top_limbs():
    return L_TOP + K


def ks_of(n, rots):
    """Rotations from tests/galois_sweep.py's elements of n, none the identity, so that the gather
    moves: the middle element for one rotation; with three, one from each third."""
    import galois_sweep
    ks = [k for k in galois_sweep.S(n) if k != 1]
    if rots == 1:
        return (ks[len(ks) // 2],)
    return tuple(ks[(2 * i + 1) * len(ks) // (2 * rots)] for i in range(rots))


def parity_cases():
    out = []
    for bits in (32, 64):
        for n in ALL_N:
            b = batch_of(n)
            for L in LEVELS:
                for comps in COMPS:
                    for rots in ROTS:
                        out.append(Case("mac", bits, n, b, L, comps, rots))
                        out += [Case("lintrans", bits, n, b, L, comps, rots, w, z)
                                for w in (False, True) for z in (False, True)]
                out += [Case("relin", bits, n, b, L, 2, 1, pairs=pairs) for pairs in PAIRS]
    return out


def validate_cases():
    """The poison test: every word outside the view all ones, NTTMUL_FLAG_VALIDATE on."""
    out = []
    for bits in (32, 64):
        for L in (4, 3, 1):
            out.append(Case("mac", bits, 256, 5, L, 2, 3, validate=True))
            out.append(Case("lintrans", bits, 256, 5, L, 2, 3, True, True, validate=True))
            out.append(Case("relin", bits, 256, 5, L, 2, 1, pairs=1, validate=True))
    return out


Footprint = namedtuple("Footprint", "entry case host", defaults=("",))
FP_SIZES = ((256, 5), (8192, 3))
FP_LEVEL = 3


def footprint_cases():
    out = []
    for bits in (32, 64):
        for n, b in FP_SIZES:
            for case, stem in ((Case("mac", bits, n, b, FP_LEVEL, 2, 3), "nttmul_ksntt_mac_view"),
                               (Case("lintrans", bits, n, b, FP_LEVEL, 2, 3, True, True),
                                "nttmul_lintrans_apply_view"),
                               (Case("relin", bits, n, b, FP_LEVEL, 2, 1, pairs=3),
                                "nttmul_ctmul_relin_view")):
                out.append(Footprint(stem + "_device", case))
                out.append(Footprint(stem, case, "host"))
    return out


# ---------------------------------------------------------------------------------------------
# The mirror
# ---------------------------------------------------------------------------------------------

def _cls(bits):
    assert bits in (32, 64)
    return ("Arith32P", "u32") if bits == 32 else ("Arith64", "u64")


def kernel_name(case):
    """level.hip: one kernel per call at every n; the class follows the word size alone.  What
    nttmul_level_kernel_name returns."""
    cls, io = _cls(case.bits)
    if case.op == "mac":
        return f"k_level_mac<{cls},{io},{case.comps}>"
    if case.op == "lintrans":
        return f"k_level_lintrans<{cls},{io},{case.comps},{int(case.weighted)}>"
    assert case.op == "relin"
    return f"k_level_relin<{cls},{io}>"


def kernels_of(case):
    """The kernel_keys `case` launches, in launch order.  With NTTMUL_FLAG_VALIDATE: the dense
    operands through libnttmul_rns.so's range check (a_hat or up_hat; then c0_hat; x_hat and y_hat
    of relin, the same memory once), the viewed operands through k_level_check_range (the key; then
    w_hat), in the order the dense call checks them."""
    _, io = _cls(case.bits)
    dense, view = f"k_rns_check_range<{io}>", f"k_level_check_range<{io}>"
    checks = []
    if case.validate:
        checks = [dense, view]
        if case.op == "lintrans":
            checks += [view] * case.weighted + [dense] * case.c0
        if case.op == "relin":
            checks += [dense, dense]
    return checks + [kernel_name(case)]


def units_per_block(case):
    """{kernel_key: (units per workgroup and grid row, units of the launch per grid row)}: V slices
    of 256 slots for mac (batch n / 256 of them), V batch entries for the other two."""
    units = case.batch * (case.n // 256) if case.op == "mac" else case.batch
    return {kernel_name(case): (V, units)}


def bpu(case):
    """Workgroups per run of V units: the rotations (mac), the n / 256 slot ranges (the others)."""
    return case.rots if case.op == "mac" else case.n // 256


def launch_waves(case, wave=64):
    (key, (per, units)), = units_per_block(case).items()
    return {key: -(-units // per) * bpu(case) * (case.L + K) * (256 // wave)}


def ends_partial(case):
    return all(units % per for per, units in units_per_block(case).values())


# Scale cases (tests/test_gpu_level_scale.py): the rule of tests/scale_cases.py on one row per new
# kernel and word class: at least MIN_WAVES = 2 * 8192 waves in the launch, the smallest batch that
# meets it and ends in a partial last workgroup
SCALE_N = {"mac": 256, "lintrans": 4096, "relin": 4096}   # mac's slices of 256 slots come in
SCALE_LEVEL = 3                                            # fours above n = 512: no partial run
WAVE, MIN_WAVES = 64, 2 * 8192


def scale_cases():
    out = []
    for bits in (32, 64):
        for proto in (Case("mac", bits, SCALE_N["mac"], 1, SCALE_LEVEL, 2, 3),
                      Case("lintrans", bits, SCALE_N["lintrans"], 1, SCALE_LEVEL, 2, 3, True, True),
                      Case("relin", bits, SCALE_N["relin"], 1, SCALE_LEVEL, 2, 1, pairs=2)):
            b = 1
            while (min(launch_waves(proto._replace(batch=b)).values()) < MIN_WAVES
                   or not ends_partial(proto._replace(batch=b))):
                b += 1
            out.append(proto._replace(batch=b))
    return out


def referenced_cases():
    """The cases whose every output word a GPU test holds to the CPU reference (tests/full_ref.py)
    of the dense call on the gathered operand: the parity cases and the clean call of the
    validate cases, at every n."""
    return parity_cases() + validate_cases()


def all_cases():
    return referenced_cases() + [f.case for f in footprint_cases()] + scale_cases()


# Kernels of libnttmul_level.so beyond libnttmul_xconv.so's that no call can launch.  None:
# level.hip instantiates only what dispatch reaches.
UNREACHABLE = ()
