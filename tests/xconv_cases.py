"""Case tables of tests/test_gpu_xconv.py, test_gpu_xconv_footprint.py, test_gpu_xconv_scale.py and
test_gpu_xconv_bases.py, and a pure-Python mirror of the dispatch behind include/nttmul_xconv.h
(csrc/xconv.hip dispatch, csrc/xconv.cpp run, csrc/xconv_plan.hpp xconv_shape): plain data and
arithmetic, no GPU.  Built from tests/mdntt_cases.py's constants: the two libraries share their
shapes, their scratch and their sub-batch rule.

tests/test_xconv_ledger.py holds the mirror against the cross-compiled lib/libnttmul_xconv.so (the
kernels it holds beyond libnttmul_ctmul.so's are exactly the ones the mirror names over these
cases); test_gpu_xconv.py::test_mirror_agrees_with_the_library_dispatch anchors it on the GPU to
the library's own dry run (nttmul_xconv_kernel_name).

The conversion sum holds K + 1 products, the correction last, and folds every CADENCE of them:
CADENCE_K is mdntt_cases' shifted by one, so that K + 1 sits on both sides of each cadence and at
the lengths where an unfolded sum overflows."""
from collections import namedtuple

import mdntt_cases as MC

OPS = ("extend", "moddown")                   # nttmul_xconv_kernel_name's numbering
SCALES = (1, 65537)
CADENCE = MC.CADENCE
ALL_N = MC.ALL_N
DEFAULT_SCRATCH_MB = MC.DEFAULT_SCRATCH_MB
BAND_LOG2 = 46                                # csrc/xconv_plan.hpp kXcBandLog2
MIN_BAND_LOG2 = 40                            # the interface's requirement

Case = namedtuple("Case", "op bits n batch L K t validate scratch_mb moduli",
                  defaults=(1, False, 0, None))

N = MC.N
BATCHES = MC.BATCHES
SHAPES = MC.SHAPES
WIDE = MC.WIDE                                # batch 1; (1, 63): K + 1 = 64 products
CADENCE_K = {bits: tuple(k - 1 for k in ks if k > 1) for bits, ks in MC.CADENCE_K.items()}
CADENCE_L = MC.CADENCE_L
DEGREE_SHAPE = MC.DEGREE_SHAPE                # every n, batch 2 (1 at 65536)
SAMPLE_STEP = 64                              # the composition samples first, last, one per 1/64
SUBBATCH = MC.SUBBATCH
VALIDATE = MC.VALIDATE
HOST = MC.HOST
HOST_SHAPE = MC.HOST_SHAPE
RESCALE = ((256, 1), (256, 3), (8192, 3))     # (n, L): K = 1, t = 1, batch RESCALE_BATCH
RESCALE_BATCH = 2
EDGE_N = (256, 8192)
EDGE_K = (1, 2, 5)
EDGE_L = 2
CHAIN_N = (256, 8192)


def md_case(case):
    """The mdntt_cases.Case of the same shape (the moduli, the chunks)."""
    return MC.Case(case.bits, case.n, case.batch, case.L, case.K, case.validate, case.scratch_mb,
                   case.moduli)


def moduli_of(case):
    """(q, p) of a case: ks_ref.bases of its class, or the profile of tests/basis_cases.py its
    `moduli` names."""
    if case.moduli not in (None, "small"):
        import basis_cases as BC
        return BC.basis(case.moduli, case.L, case.K)
    return MC.moduli_of(md_case(case))


def parity_cases():
    """Both operations, both word classes, both scales, over mdntt_cases' shapes."""
    out = []
    for op in OPS:
        for bits in (32, 64):
            rows = [(N, b, L, K) for b in BATCHES for L, K in SHAPES]
            rows += [(N, 1, L, K) for L, K in WIDE]
            rows += [(N, 1, CADENCE_L, K) for K in CADENCE_K[bits]]
            rows += [(n, 1 if n == 65536 else 2, *DEGREE_SHAPE) for n in ALL_N]
            out += [Case(op, bits, n, b, L, K, t) for t in SCALES for n, b, L, K in rows]
    return out


def subbatch_cases():
    return [Case(op, bits, n, batch, L, K, 65537, False, 1)
            for op in OPS for bits, n, L, K, batch, _ in SUBBATCH]


Footprint = namedtuple("Footprint", "entry case host", defaults=("",))
FP_SHAPES = MC.FP_SHAPES
FP_SIZES = MC.FP_SIZES


def footprint_cases():
    out = []
    for op in OPS:
        for bits in (32, 64):
            for shape in FP_SHAPES:
                for n, batch in FP_SIZES:
                    case = Case(op, bits, n, batch, *shape, 65537)
                    out.append(Footprint(f"nttmul_xconv_{op}_device", case))
                    out.append(Footprint(f"nttmul_xconv_{op}", case, "host"))
    return out


def in_limbs(case):
    return case.K if case.op == "extend" else case.L + case.K


def fp_guard_words(case):
    """The guard width tests/guarded.py gives the call: one batch entry of the larger operand."""
    from guarded import guard_words
    return guard_words(max(case.L, in_limbs(case)) * case.n)


# Scale cases (tests/test_gpu_xconv_scale.py): the rule of tests/scale_cases.py on one case per new
# kernel template and word class
SCALE_N = MC.SCALE_N
SCALE_SHAPE = MC.SCALE_SHAPE
WAVE, MIN_WAVES = MC.WAVE, MC.MIN_WAVES


def launch_waves(case):
    rows = grid_rows(case)
    return {k: -(-units // per) * bpu(k) * rows[k] * (256 // WAVE)
            for k, (per, units, _) in units_per_block(case).items()}


def scale_batch(op, bits, n):
    """The smallest batch at which every launch of the call meets the rule."""
    L, K = SCALE_SHAPE

    def full(b):
        return all(w >= MIN_WAVES for w in launch_waves(Case(op, bits, n, b, L, K)).values())

    lo, hi = 0, 1
    while not full(hi):
        lo, hi = hi, 2 * hi
        assert hi < 1 << 24
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if full(mid) else (mid, hi)
    for b in range(hi, hi + 64):
        case = Case(op, bits, n, b, L, K)
        assert len(chunks(case)) == 1
        if all(units % per for per, units, _ in units_per_block(case).values() if per > 1):
            return b
    raise AssertionError((op, bits, n))


def scale_cases():
    """k_xconv_fwd<.., 0> and <.., 1> at n = 4096; k_xconv_cols_fwd by either operation and
    k_xconv_rows by extend at n = 8192."""
    L, K = SCALE_SHAPE
    rows = [(op, 4096) for op in OPS] + [("extend", 8192)]
    return [Case(op, bits, n, scale_batch(op, bits, n), L, K, 65537)
            for bits in (32, 64) for op, n in rows]


def referenced_cases():
    """The cases whose every output word a GPU test holds to the CPU reference (tests/full_ref.py):
    all but the scale and the 4 GiB cases, whose batches exist to fill the machine."""
    out = parity_cases() + subbatch_cases()
    n, batch, shape = VALIDATE
    out += [Case(op, bits, n, batch, *shape, 1, True) for op in OPS for bits in (32, 64)]
    out += [Case(op, bits, n, batch, *HOST_SHAPE) for op in OPS for bits in (32, 64)
            for n, batch in HOST]
    out += [Case("moddown", bits, n, 1, EDGE_L, K, t) for bits in (32, 64) for n in EDGE_N
            for K in EDGE_K for t in SCALES]
    out += [f.case for f in footprint_cases()]
    return out


def all_cases():
    return referenced_cases() + scale_cases()


# ---------------------------------------------------------------------------------------------
# The seeded inputs of the GPU tests (tests/test_xconv_ref.py holds every one of them to have no
# coefficient inside the guard band, so no GPU assertion is ever conditional on seeded data)
# ---------------------------------------------------------------------------------------------

def seed_of(case):
    return (1000 * case.L + 10 * case.K + case.n + 7 * case.batch + (case.t > 1)
            + 3 * OPS.index(case.op) + case.bits)


def seeded_input(case, seed=None):
    """Seeded canonical words in NTT order (any canonical vector is a transform of something):
    [batch, K, n] over P for extend, [batch, L + K, n] over Q u P for moddown."""
    import numpy as np
    import bconv_ref as B
    q, p = moduli_of(case)
    rng = np.random.default_rng(seed_of(case) if seed is None else seed)
    dt = np.uint32 if case.bits == 32 else np.uint64
    x = B.random_words(rng, p if case.op == "extend" else q + p, case.batch, case.n, dt)
    if seed is None and case.batch == 1 and case.n == N and case.moduli is None:
        # the conversion's worst case as the P part of the batch-1 rows (the wide shapes and K + 1
        # over the cadence): the transform of x_j = -Ph_j t^-1 mod p_j at every coefficient, so
        # that every y_j = p_j - 1 under every target modulus
        import hoist_ref as H
        worst = [w * pow(case.t, -1, m) % m for w, m in zip(B.worst_case(p), p)]
        flat = np.empty((1, case.K, case.n), dtype=dt)
        flat[0] = np.array(worst, dtype=dt)[:, None]
        x[:, -case.K:, :] = H.forward(flat, p)
    return x


def rescale_case(bits, n, L):
    return Case("moddown", bits, n, RESCALE_BATCH, L, 1)


def rescale_input(case):
    """(X, x): per batch entry n seeded big integers in [0, Q p), the ends of the range among
    them, and their residues [batch, L + 1, n] in coefficient order (the test transforms them)."""
    import numpy as np
    import mdntt_ref
    from math import prod
    q, p = moduli_of(case)
    ext = q + p
    rng = np.random.default_rng(case.n * case.L + case.bits)
    dt = np.uint32 if case.bits == 32 else np.uint64
    X = [mdntt_ref.big_integers(rng, case.n, prod(int(v) for v in ext)) for _ in range(case.batch)]
    return X, np.stack([mdntt_ref.residues(Xb, ext, dt) for Xb in X])


def sample_indices(n):
    """The coefficients the device composition is compared on: the first, the last, and one in
    each of the 64 blocks of n / 64 (at a position that moves with the block)."""
    step = n // SAMPLE_STEP
    return sorted({0, n - 1} | {i * step + (i * 37 + 11) % step for i in range(SAMPLE_STEP)})


def seeded_gpu_inputs():
    """(case, input) of every seeded input a GPU test feeds the library."""
    n, batch, shape = VALIDATE
    cases = parity_cases() + subbatch_cases()
    cases += [Case(op, bits, n, batch, *shape, 1, True) for op in OPS for bits in (32, 64)]
    cases += [Case(op, bits, n, batch, *HOST_SHAPE) for op in OPS for bits in (32, 64)
              for n, batch in HOST]
    cases += [f.case._replace(batch=max(b for _, b in FP_SIZES if _ == f.case.n))
              for f in footprint_cases() if not f.host]
    for case in cases:
        yield case, seeded_input(case)
    for case in bases_cases():
        yield case, bases_input(case)
    import hoist_ref as H
    for bits in (32, 64):
        for n, L in RESCALE:                  # coefficient order: the NTT-order input is its forward
            case = rescale_case(bits, n, L)
            yield case, H.forward(rescale_input(case)[1], sum(moduli_of(case), ()))


# Mixed-size bases (tests/test_gpu_xconv_bases.py, tests/basis_cases.py): a case's `moduli` names a
# profile.  P above every q (chain64, chain32) and P below every q (the _rev profiles)
BASES_N = (256, 8192)
BASES_PROFILES = ("chain64", "chain64_rev", "chain32", "chain32_rev")
BASES_SHAPES = ((4, 2), (3, 2))
BASES_BATCH = 2


def bases_input(case):
    """seeded_input with the ends of every limb's range in the first two words."""
    x = seeded_input(case)
    q, p = moduli_of(case)
    for l, m in enumerate(p if case.op == "extend" else q + p):
        x[0, l, :2] = (0, m - 1)
    return x


def bases_cases():
    import basis_cases as BC
    return [Case(op, BC.bits_of(prof), n, BASES_BATCH, L, K, t, False, 0, prof)
            for op in OPS for prof in BASES_PROFILES for n in BASES_N for L, K in BASES_SHAPES
            for t in SCALES]


# ---------------------------------------------------------------------------------------------
# The mirror
# ---------------------------------------------------------------------------------------------

def l1_of(n):
    return MC.l1_of(n)


def sequence(op, n, bits):
    """xconv.hip dispatch: the launches of one sub-batch, in order.  The inverse half is
    mdntt.hip's (and above n = 4096 rnsmp.hip's column pass); the forward half is k_xconv_fwd with
    the operation as its last template argument up to n = 4096, k_xconv_cols_fwd above, followed
    by k_xconv_rows (extend) or mdntt.hip's k_mdntt_rows (moddown)."""
    assert n in ALL_N, "n > 65536 is NTTMUL_EUNSUPPORTED"
    assert op in OPS
    cls, io = ("Arith32P", "u32") if bits == 32 else ("Arith64", "u64")
    if n <= 4096:
        logn = n.bit_length() - 1
        return [f"k_mdntt_inv<{cls},{io},{logn}>",
                f"k_xconv_fwd<{cls},{io},{logn},{OPS.index(op)}>"]
    l1 = l1_of(n)
    last = "k_xconv_rows" if op == "extend" else "k_mdntt_rows"
    return [f"k_mdntt_inv_rows<{cls},{io},{l1}>", f"k_rnsmp_cols_inv<{cls},{io},{l1}>",
            f"k_xconv_cols_fwd<{cls},{io},{l1}>", f"{last}<{cls},{io},{l1}>"]


def kernel_name(op, n, bits):
    """What nttmul_xconv_kernel_name returns."""
    return " + ".join(sequence(op, n, bits))


def chunks(case):
    """xconv.cpp run / xconv_plan.hpp xconv_shape: mdntt's sub-batches, for both operations."""
    return MC.chunks(md_case(case))


def kernels_of(case):
    """The kernel_keys `case` launches, in launch order."""
    io = "u32" if case.bits == 32 else "u64"
    return ([f"k_rns_check_range<{io}>"] if case.validate else []) + \
        sequence(case.op, case.n, case.bits) * len(chunks(case))


def units_per_block(case):
    """{kernel_key: (units per workgroup and limb, units of the launch per limb, words per unit
    and limb)}: mdntt_cases.units_per_block under this library's kernel names."""
    seq = sequence(case.op, case.n, case.bits)
    md = MC.units_per_block(md_case(case))
    return dict(zip(seq, (md[k] for k in MC.sequence(case.n, case.bits))))


def grid_rows(case):
    """{kernel_key: limbs the launch covers}: K for the inverse's kernels, L for the forward's."""
    seq = sequence(case.op, case.n, case.bits)
    inv = seq[:1] if case.n <= 4096 else seq[:2]
    return {k: case.K if k in inv else case.L for k in seq}


bpu = MC.bpu

# Kernels of libnttmul_xconv.so beyond libnttmul_ctmul.so's that no call can launch.  None:
# xconv.hip instantiates only what dispatch reaches.
UNREACHABLE = ()
