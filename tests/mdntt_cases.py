"""Case tables of tests/test_gpu_mdntt.py, test_gpu_mdntt_footprint.py and test_gpu_mdntt_scale.py,
and a pure-Python mirror of the dispatch behind include/nttmul_mdntt.h (csrc/mdntt.hip dispatch,
csrc/mdntt.cpp run, csrc/mdntt_plan.hpp mdntt_shape): plain data and arithmetic, no GPU.

tests/test_mdntt_ledger.py holds the mirror against the cross-compiled lib/libnttmul_mdntt.so (the
kernels it holds beyond libnttmul_hoist.so's are exactly the ones the mirror names over these
cases); test_gpu_mdntt.py::test_mirror_agrees_with_the_library_dispatch anchors it on the GPU to
the library's own dry run (nttmul_mdntt_kernel_name).

The shapes are the smallest at which the kernels can go wrong.  At n = 256 a transform thread
group is 16 threads, a workgroup of the inverse holds 16 thread groups of two polynomials each on
32-bit words (32 polynomials) and of one on 64-bit words, a workgroup of the forward kernel 16
polynomials: batch 3 is an odd batch with a half-empty pair, batch 33 a partial second (inverse,
32-bit) or third workgroup.  The conversion sum folds every CADENCE products."""
from collections import namedtuple

import bconv_cases as BC
import ks_cases as KC
import ks_ref

CADENCE = BC.CADENCE                         # csrc/bconv_dev.hpp BconvArith<W>::kCadence
ALL_N = tuple(1 << e for e in range(8, 17))
MAX_LIMBS = 64                               # NTTMUL_RNS_MAX_LIMBS bounds L + K
DEFAULT_SCRATCH_MB = 512

# moduli: None for ks_ref.bases(bits, L, K), or "small" for ks_cases.small_moduli().  A case names
# its bases and holds no prime (ks_cases.Case has the reason)
Case = namedtuple("Case", "bits n batch L K validate scratch_mb moduli", defaults=(False, 0, None))

N = 256
BATCHES = (3, 33)
SHAPES = ((1, 1), (4, 1), (4, 2), (3, 2), (5, 3), (12, 4))
WIDE = ((60, 4), (1, 63))                    # batch 1
# K on both sides of the fold cadence and at the lengths where an unfolded sum overflows (32-bit:
# 5 products pass 2^64; 64-bit: 17 pass 2^128); L = 2, batch 1
CADENCE_K = {32: (1, 2, 3, 5, 9), 64: (3, 4, 5, 17)}
CADENCE_L = 2
DEGREE_SHAPE = (4, 2)                        # every n, batch 2 (1 at 65536)
RANGE_N = (256, 4096, 8192)                  # worst-case ranges, (L, K) = RANGE_SHAPE, batch 2
RANGE_SHAPE = (3, 2)
RANGE_FILLS = ("top", "zero_p", "zero_q")
RESCALE = tuple((n, L) for n in (256, 8192) for L in (1, 3))   # K = 1, batch 2
RESCALE_BATCH = 2
# (bits, n, L, K, batch, sub-batches) with scratch_mb = 1
SUBBATCH = ((64, 4096, 3, 2, 35, (16, 16, 3)), (64, 65536, 2, 2, 3, (1, 1, 1)))
VALIDATE = (256, 2, (3, 2))                  # n, batch, shape
HOST = ((256, 5), (8192, 2))                 # (n, batch), shape (3, 2)
HOST_SHAPE = (3, 2)


def moduli_of(case):
    """(q, p) of a case."""
    assert case.moduli in (None, "small")
    return KC.small_moduli() if case.moduli else ks_ref.bases(case.bits, case.L, case.K)


def parity_cases():
    out = []
    for bits in (32, 64):
        out += [Case(bits, N, b, L, K) for b in BATCHES for L, K in SHAPES]
        out += [Case(bits, N, 1, L, K) for L, K in WIDE]
        out += [Case(bits, N, 1, CADENCE_L, K) for K in CADENCE_K[bits]]
        out += [Case(bits, n, 1 if n == 65536 else 2, *DEGREE_SHAPE) for n in ALL_N]
    L, K, _ = KC.SMALL_SHAPE
    out.append(Case(32, N, 3, L, K, False, 0, "small"))
    return out


def subbatch_cases():
    return [Case(bits, n, batch, L, K, False, 1) for bits, n, L, K, batch, _ in SUBBATCH]


# The caller's memory (tests/test_gpu_mdntt_footprint.py): host "" for the *_device call, "host"
# for the host form
Footprint = namedtuple("Footprint", "entry case host", defaults=("",))
FP_SHAPES = ((3, 2), (5, 1))
FP_SIZES = ((256, 1), (256, 33), (4096, 1), (8192, 1))   # (n, batch)


def footprint_cases():
    out = []
    for bits in (32, 64):
        for shape in FP_SHAPES:
            for n, batch in FP_SIZES:
                case = Case(bits, n, batch, *shape)
                out.append(Footprint("nttmul_mdntt_moddown_device", case))
                out.append(Footprint("nttmul_mdntt_moddown", case, "host"))
    return out


def fp_guard_words(case):
    """The guard width tests/guarded.py gives the call: one batch entry of x_hat, (L + K) n."""
    from guarded import guard_words
    return guard_words((case.L + case.K) * case.n)


# ---------------------------------------------------------------------------------------------
# Scale cases (tests/test_gpu_mdntt_scale.py): the rule of tests/scale_cases.py -- every launch of
# a row holds at least MIN_WAVES = 2 * 8192 waves and ends in a partial workgroup where the kernel
# takes several units per workgroup -- on one case per new kernel template and word class
# ---------------------------------------------------------------------------------------------

SCALE_N = (4096, 8192)
SCALE_SHAPE = (2, 1)
WAVE, MIN_WAVES = 64, 2 * 8192


def launch_waves(case):
    """{kernel_key: waves of the launch} for one sub-batch of the whole batch."""
    rows = grid_rows(case)
    return {k: -(-units // per) * bpu(k) * rows[k] * (256 // WAVE)
            for k, (per, units, _) in units_per_block(case).items()}


def scale_batch(bits, n):
    """The smallest batch at which every launch of the call meets the rule."""
    L, K = SCALE_SHAPE

    def full(b):
        return all(w >= MIN_WAVES for w in launch_waves(Case(bits, n, b, L, K)).values())

    lo, hi = 0, 1
    while not full(hi):
        lo, hi = hi, 2 * hi
        assert hi < 1 << 24
    while hi - lo > 1:                       # the waves grow with the batch
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if full(mid) else (mid, hi)
    for b in range(hi, hi + 64):
        case = Case(bits, n, b, L, K)
        assert len(chunks(case)) == 1
        if all(units % per for per, units, _ in units_per_block(case).values() if per > 1):
            return b
    raise AssertionError((bits, n))


def scale_cases():
    L, K = SCALE_SHAPE
    return [Case(bits, n, scale_batch(bits, n), L, K) for bits in (32, 64) for n in SCALE_N]


# x_hat just over 4 GiB, compared with the same call in chunks below 1 GiB: (bits, n, L, K)
LARGE = ((32, 4096, 1, 1), (64, 65536, 1, 1))
LARGE_BYTES = 1 << 32


def large_batch(bits, n, L, K):
    """The smallest batch whose x_hat exceeds 4 GiB."""
    return LARGE_BYTES // ((L + K) * n * (bits // 8)) + 1


def referenced_cases():
    """The cases whose every output word a GPU test holds to the CPU reference (tests/full_ref.py):
    all but the scale and the 4 GiB cases, whose batches exist to fill the machine."""
    out = parity_cases() + subbatch_cases()
    out += [Case(bits, n, 2, *RANGE_SHAPE) for bits in (32, 64) for n in RANGE_N]
    out += [Case(bits, n, RESCALE_BATCH, L, 1) for bits in (32, 64) for n, L in RESCALE]
    n, batch, shape = VALIDATE
    out += [Case(bits, n, batch, *shape, True) for bits in (32, 64)]
    out += [Case(bits, n, batch, *HOST_SHAPE) for bits in (32, 64) for n, batch in HOST]
    out += [f.case for f in footprint_cases()]
    return out


def all_cases():
    out = referenced_cases() + scale_cases()
    out += [Case(bits, n, large_batch(bits, n, L, K), L, K) for bits, n, L, K in LARGE]
    return out


# ---------------------------------------------------------------------------------------------
# The mirror
# ---------------------------------------------------------------------------------------------

def word_bits(q, p):
    """mdntt_plan.hpp mdntt_validate: ks_cases.word_bits, one word class over both bases."""
    return KC.word_bits(q, p)


def l1_of(n):
    """mdntt.hip dispatch: the 2^L1 x 4096 split above n = 4096, L1 = logn - 12."""
    assert n in ALL_N and n > 4096
    return n.bit_length() - 1 - 12


def sequence(n, bits):
    """mdntt.hip single / passes: the launches of one sub-batch, in order.  The class follows the
    word size alone (plain Arith32P at every degree: a full transform has no base blocks); two
    launches up to n = 4096, four above, of which the inverse column pass is rnsmp.hip's kernel."""
    assert n in ALL_N, "n > 65536 is NTTMUL_EUNSUPPORTED"
    cls, io = ("Arith32P", "u32") if bits == 32 else ("Arith64", "u64")
    if n <= 4096:
        logn = n.bit_length() - 1
        return [f"k_mdntt_inv<{cls},{io},{logn}>", f"k_mdntt_fwd<{cls},{io},{logn}>"]
    l1 = l1_of(n)
    return [f"k_mdntt_inv_rows<{cls},{io},{l1}>", f"k_rnsmp_cols_inv<{cls},{io},{l1}>",
            f"k_mdntt_cols_fwd<{cls},{io},{l1}>", f"k_mdntt_rows<{cls},{io},{l1}>"]


def kernel_name(n, bits):
    """What nttmul_mdntt_kernel_name returns."""
    return " + ".join(sequence(n, bits))


def chunks(case):
    """mdntt.cpp run / mdntt_plan.hpp mdntt_shape: the sub-batches of a call.  At most scratch_mb
    MiB per scratch buffer -- y [cnt][K][n] and, above n = 4096, t [cnt][L][n] -- in whole
    polynomials, never less than one."""
    wb = case.bits // 8
    per_poly = max(case.K * case.n * wb, case.L * case.n * wb if case.n > 4096 else 0)
    limit = (case.scratch_mb or DEFAULT_SCRATCH_MB) << 20
    chunk = max(1, min(case.batch, limit // per_poly))
    return [min(chunk, case.batch - p) for p in range(0, case.batch, chunk)]


def kernels_of(case):
    """The kernel_keys `case` launches, in launch order: with NTTMUL_FLAG_VALIDATE the range check
    (libnttmul_rns.so's kernel) once, then the sequence once per sub-batch."""
    q, p = moduli_of(case)
    assert word_bits(q, p) == case.bits and (len(q), len(p)) == (case.L, case.K)
    io = "u32" if case.bits == 32 else "u64"
    return ([f"k_rns_check_range<{io}>"] if case.validate else []) + \
        sequence(case.n, case.bits) * len(chunks(case))


def units_per_block(case):
    """{kernel_key: (units per workgroup and limb, units of the launch per limb, words per unit and
    limb)} for one sub-batch of the whole batch.  n <= 4096: a unit is a polynomial, a workgroup
    holds 256 / (n / 16) thread groups, each of one polynomial -- of two in k_mdntt_inv on 32-bit
    words (xform_upg).  Above: one row of 4096 per workgroup in the row kernels, 256 columns of one
    polynomial per workgroup in the column kernels (16 workgroups per unit)."""
    seq = sequence(case.n, case.bits)
    if case.n <= 4096:
        pb = 256 // (case.n // 16)
        return {seq[0]: (pb * (2 if case.bits == 32 else 1), case.batch, case.n),
                seq[1]: (pb, case.batch, case.n)}
    l1 = l1_of(case.n)
    return {seq[0]: (1, case.batch << l1, 4096), seq[1]: (1, case.batch, case.n),
            seq[2]: (1, case.batch, case.n), seq[3]: (1, case.batch << l1, 4096)}


def grid_rows(case):
    """{kernel_key: limbs the launch covers}: K for the inverse's kernels (gridDim.y), L for the
    forward's (the limb fastest in a one-dimensional grid, blockIdx.x % L)."""
    seq = sequence(case.n, case.bits)
    inv = seq[:1] if case.n <= 4096 else seq[:2]
    return {k: case.K if k in inv else case.L for k in seq}


def bpu(key):
    """Workgroups per unit: the column kernels spread a polynomial over 4096 / 256 = 16."""
    return 16 if "_cols_" in key else 1


# Kernels of libnttmul_mdntt.so beyond libnttmul_hoist.so's that no call can launch: (regular
# expression over the kernel_key, reason).  None: mdntt.hip instantiates only what dispatch reaches.
UNREACHABLE = ()
