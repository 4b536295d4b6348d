"""Case tables of tests/test_gpu_ks.py and test_gpu_ks_footprint.py, and a pure-Python mirror of
the dispatch behind include/nttmul_ks.h (csrc/ks.hip dispatch, csrc/ks.cpp run): plain data and
arithmetic, no GPU.

tests/test_ks_ledger.py holds the mirror against the cross-compiled lib/libnttmul_ks.so (the
kernels it holds beyond libnttmul_galois.so's are exactly the ones the mirror names over these
cases); test_gpu_ks.py::test_mirror_agrees_with_the_library_dispatch anchors it on the GPU to the
library's own dry run (nttmul_ks_kernel_name).

The shapes are the smallest at which k_ks_modup (csrc/ks_dev.hpp) can go wrong.  A workgroup takes
4 (32-bit words) or 1 (64-bit) slices of 256 coefficients of one digit, so n = 256 with batch 3 is
several workgroups in both classes and, on 32-bit words, a partial one that holds several
polynomials; a thread passes over the L + K target limbs in tiles of TILE; the accumulator is
folded every CADENCE products of a digit."""
from collections import namedtuple

import bconv_cases as BC
import ks_ref as ref

TILE = BC.TILE                               # csrc/bconv.hpp kBconvTile
CADENCE = BC.CADENCE                         # csrc/bconv_dev.hpp BconvArith<W>::kCadence
OPS = ("modup", "moddown")                   # nttmul_ks_kernel_name's op numbers
ALL_N = tuple(1 << e for e in range(8, 17))
MAX_LIMBS = 64                               # NTTMUL_RNS_MAX_LIMBS bounds L + K

# moduli: None for ks_ref.bases(bits, L, K), or "small" for small_moduli().  A case names its
# bases and holds no prime: finding primes loads lib/libnttmul.so (nttmul.is_prime), which a GPU
# test module must not do while it is collected, before its fixture has imported torch
Case = namedtuple("Case", "op bits n batch L K alpha validate moduli", defaults=(False, None))

N, BATCH = 256, 3
# (L, K, alpha): the smallest basis; even digits; a last digit of one limb; one digit; dnum = L;
# L + K on both sides of the tile of 4; L + K = 64
SHAPES = ((1, 1, 1), (4, 2, 2), (5, 2, 2), (5, 3, 5), (6, 1, 1), (2, 1, 1), (3, 2, 2), (60, 4, 15))
# digit widths on both sides of the fold cadence and at the lengths where an unfolded sum
# overflows (32-bit: 5 products pass 2^64; 64-bit: 17 pass 2^128); L = 2 alpha, K = 1, batch 1
CADENCE_ALPHA = {32: (1, 2, 3, 5, 9), 64: (3, 4, 5, 17)}
CADENCE_K = 1
DEGREES = ((4096, 2), (65536, 1))            # (n, batch) with DEGREE_SHAPE: the logn = 16 addressing
DEGREE_SHAPE = (4, 2, 2)
MODDOWN = ((8192, 2), (65536, 1))            # (n, batch) against bconv_ref.moddown
MODDOWN_BCONV = ((256, 3), (4096, 2))        # (n, batch) against nttmul.BaseConverter.moddown
MODDOWN_SHAPE = (3, 2)                       # (L, K)
VALIDATE = (256, 2, (3, 2, 2))               # n, batch, shape
HOST = (256, 5, (3, 2, 2))
CHAIN = ((256, "rns"), (8192, "rnsmp"))      # the mac_ntt context of the degree
CHAIN_SHAPE, CHAIN_BATCH, CHAIN_H = (4, 2, 2), 2, 8
# small moduli on 32-bit words: bconv_cases.SMALL and one prime of the top to fill Q, P of the top
SMALL_SHAPE = (4, 2, 2)


def small_moduli():
    L, K, _ = SMALL_SHAPE
    top = ref.bases(32, L - len(BC.SMALL), K)
    return tuple(BC.SMALL) + top[0], top[1]


def moduli_of(case):
    """(q, p) of a case."""
    assert case.moduli in (None, "small")
    return small_moduli() if case.moduli else ref.bases(case.bits, case.L, case.K)


def dnum(case):
    return -(-case.L // case.alpha)


def modup_cases():
    out = []
    for bits in (32, 64):
        out += [Case("modup", bits, N, BATCH, *s) for s in SHAPES]
        out += [Case("modup", bits, N, 1, 2 * a, CADENCE_K, a) for a in CADENCE_ALPHA[bits]]
        out += [Case("modup", bits, n, batch, *DEGREE_SHAPE) for n, batch in DEGREES]
    out.append(Case("modup", 32, N, BATCH, *SMALL_SHAPE, False, "small"))
    return out


def moddown_cases():
    L, K = MODDOWN_SHAPE
    return [Case("moddown", bits, n, batch, L, K, 1) for bits in (32, 64)
            for n, batch in MODDOWN + MODDOWN_BCONV]


# The caller's memory (tests/test_gpu_ks_footprint.py).  n = 256 with batch 1 and 5: on 32-bit
# words a workgroup takes four 256-word slices, so both batches end in a partial workgroup
# (5 = 4 + 1); on 64-bit words a workgroup takes one slice.  n = 4096 with batch 1.  (L, K, alpha)
# = (3, 2, 2): L + K = 5 leaves a padded target tile in modup, and moddown's L = 3 one in k_bconv;
# (5, 1, 5): one digit, L + K = 6.  host: "" for a *_device call, "host" for the host form.
Footprint = namedtuple("Footprint", "entry case host", defaults=("",))
FP_SHAPES = ((3, 2, 2), (5, 1, 5))
FP_SIZES = ((256, 1), (256, 5), (4096, 1))   # (n, batch)


def footprint_cases():
    out = []
    for bits in (32, 64):
        for op in OPS:
            for shape in FP_SHAPES:
                for n, batch in FP_SIZES:
                    case = Case(op, bits, n, batch, *shape)
                    out.append(Footprint(f"nttmul_ks_{op}_device", case))
                    out.append(Footprint(f"nttmul_ks_{op}", case, "host"))
    return out


def all_cases():
    out = modup_cases() + moddown_cases()
    n, batch, shape = VALIDATE
    out += [Case(op, bits, n, batch, *shape, True) for op in OPS for bits in (32, 64)]
    n, batch, shape = HOST
    out += [Case(op, bits, n, batch, *shape) for op in OPS for bits in (32, 64)]
    out += [Case(op, bits, n, CHAIN_BATCH, *CHAIN_SHAPE) for op in OPS for bits in (32, 64)
            for n, _ in CHAIN]
    out += [f.case for f in footprint_cases()]
    # the launches that fill the GPU twice over (tests/test_gpu_scale.py, tests/scale_cases.py)
    import scale_cases
    out += scale_cases.cases_of("ks")
    return out


def fp_guard_words(case):
    """The guard width tests/guarded.py gives the call: the widest batch entry is modup's output,
    dnum * (L + K) * n words."""
    from guarded import guard_words
    return guard_words(dnum(case) * (case.L + case.K) * case.n)


# ---------------------------------------------------------------------------------------------
# The mirror
# ---------------------------------------------------------------------------------------------

def word_bits(q, p):
    """ks_plan.cpp ks_validate: one word class over both bases, all primes distinct."""
    m = tuple(q) + tuple(p)
    assert len(q) >= 1 and len(p) >= 1 and len(m) <= MAX_LIMBS and len(set(m)) == len(m)
    if all(v < (1 << 31) for v in m):
        return 32
    assert all((1 << 32) <= v < (1 << 62) for v in m), "mixed classes are NTTMUL_EUNSUPPORTED"
    return 64


def kernel_name(op, n, bits):
    """What nttmul_ks_kernel_name returns: one kernel per word size and operation for every n, L,
    K and digit width; moddown is bconv.hip's kernel (csrc/ks.cpp run)."""
    assert n in ALL_N, "n > 65536 is NTTMUL_EUNSUPPORTED"
    io = "u32" if bits == 32 else "u64"
    return f"k_ks_modup<{io}>" if op == "modup" else f"k_bconv<{io},{BC.OPS.index('moddown')}>"


def kernels_of(case):
    """The kernel_keys `case` launches, in launch order (with NTTMUL_FLAG_VALIDATE the range check
    of libnttmul_rns.so runs first, once)."""
    assert 1 <= case.alpha <= case.L
    q, p = moduli_of(case)
    assert word_bits(q, p) == case.bits and (len(q), len(p)) == (case.L, case.K)
    io = "u32" if case.bits == 32 else "u64"
    return ([f"k_rns_check_range<{io}>"] if case.validate else []) + \
        [kernel_name(case.op, case.n, case.bits)]


def units_per_block(case):
    """{kernel_key: (slices per workgroup, slices of the launch per digit, 256)}: a slice is 256
    consecutive coefficients of one polynomial, a workgroup takes BconvArith<W>::kV = 4 (32-bit
    words) or 1 (64-bit words) of them (csrc/ks_dev.hpp `live[v]`; csrc/ks.hip modup); modup's
    digit is a grid dimension."""
    return {kernel_name(case.op, case.n, case.bits): (4 if case.bits == 32 else 1,
                                                      case.batch * (case.n // 256), 256)}


# Kernels of libnttmul_ks.so beyond libnttmul_galois.so's that no call can launch: (regular
# expression over the kernel_key, reason).  None: ks.hip instantiates only what dispatch reaches.
UNREACHABLE = ()
