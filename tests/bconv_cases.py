"""Case tables of tests/test_gpu_bconv.py and a pure-Python mirror of the dispatch behind
include/nttmul_bconv.h (csrc/bconv.hip dispatch): plain data and arithmetic, no GPU.

tests/test_bconv_ledger.py holds the mirror against the cross-compiled lib/libnttmul_bconv.so
(the kernels it holds beyond libnttmul_rns.so's are exactly the ones the mirror names over these
cases); test_gpu_bconv.py::test_mirror_agrees_with_the_library_dispatch anchors it on the GPU to
the library's own dry run (nttmul_bconv_kernel_name).

The shapes are the smallest at which k_bconv (csrc/bconv_dev.hpp) can go wrong.  A workgroup takes
4 (32-bit words) or 1 (64-bit) slices of 256 coefficients, so n = 256 with batch 3 is several
workgroups in both classes and, on 32-bit words, a partial last one that holds more than one
polynomial; a thread passes over the target limbs in tiles of TILE; the accumulator is folded every
CADENCE products."""
from collections import namedtuple

import dispatch_cases as D
from bconv_ref import primes_below

TILE = 4                                     # csrc/bconv.hpp kBconvTile
CADENCE = {32: 2, 64: 4}                     # csrc/bconv_dev.hpp BconvArith<W>::kCadence
OPS = ("convert", "moddown")                 # nttmul_bconv_kernel_name's op numbers
TOP = {32: 1 << 31, 64: 1 << 62}
STEP = 2 * 4096

Case = namedtuple("Case", "op bits n batch L K validate", defaults=(False,))

N, BATCH = 256, 3
BIG_N, BIG_BATCH = 4096, 2
# (L, K): the issue's five, and one K on each side of the target-limb tile
SHAPES = ((1, 1), (1, 3), (3, 1), (4, 4), (5, 7), (2, TILE - 1), (2, TILE + 1))
BIG_SHAPE = (4, 4)
# accumulator cadence: K = 2.  32-bit: 4, 5 (the first length at which an unfolded 64-bit sum
# overflows for these primes), 8, 9, 64, and both sides of the cadence of 2 (1, 2, 3).  64-bit:
# 16, 17 (overflows an unfolded 128-bit sum), 33, 64, and both sides of the cadence of 4 (3, 4, 5)
CADENCE_L = {32: (1, 2, 3, 4, 5, 8, 9, 64), 64: (3, 4, 5, 16, 17, 33, 64)}
CADENCE_K = 2
SMALL = (7681, D.Q0, D.Q20)                  # small moduli on 32-bit words
EXACT_L = (1, 2, 5)
HOST = {32: (3, 2), 64: (2, 3)}              # host forms: (L, K) per class


def bases(bits, L, K):
    """Disjoint from / to bases of the class at the top of its range: the first L primes below
    the class's top, then the next K."""
    p = primes_below(TOP[bits], STEP, L + K)
    return tuple(p[:L]), tuple(p[L:])


def all_cases():
    out = []
    for bits in (32, 64):
        for op in OPS:
            out += [Case(op, bits, N, BATCH, L, K) for L, K in SHAPES]
            out.append(Case(op, bits, BIG_N, BIG_BATCH, *BIG_SHAPE))
            out += [Case(op, bits, N, 1, L, CADENCE_K) for L in CADENCE_L[bits]]
            out.append(Case(op, bits, N, 2, 2, 2, True))
            out.append(Case(op, bits, N, BATCH, *HOST[bits]))
        out += [Case("moddown", bits, N, BATCH, L, 3) for L in EXACT_L]
    out += [Case(op, 32, N, BATCH, 2, 1) for op in OPS] + [Case(op, 32, N, BATCH, 1, 2) for op in OPS]
    out += [f.case for f in footprint_cases()]
    # the launches that fill the GPU twice over (tests/test_gpu_scale.py, tests/scale_cases.py)
    import scale_cases
    out += scale_cases.cases_of("bconv")
    return out


# The caller's memory (tests/test_gpu_footprint.py).  n = 256 with batch 1 and 5: on 32-bit words
# a workgroup takes four 256-word slices, so both batches end in a partial workgroup (5 = 4 + 1);
# on 64-bit words a workgroup takes one slice, so those cases have no partial workgroup and
# exercise guards and alignment only.  n = 4096 with batch 1.  (L, K) = (3, 2) and (1, 5): K = 5
# leaves a padded target-limb tile, whose jx clamp reads limb K - 1 (csrc/bconv_dev.hpp:152).
# host: "" for a *_device call, "host" for the host form.
Footprint = namedtuple("Footprint", "entry case host", defaults=("",))
FP_SHAPES = ((3, 2), (1, 5))
FP_SIZES = ((256, 1), (256, 5), (4096, 1))           # (n, batch)
FP_HOST_SIZE = (256, 5)


def footprint_cases():
    out = []
    for bits in (32, 64):
        for op in OPS:
            for L, K in FP_SHAPES:
                out += [Footprint(f"nttmul_bconv_{op}_device", Case(op, bits, n, batch, L, K))
                        for n, batch in FP_SIZES]
                out.append(Footprint(f"nttmul_bconv_{op}", Case(op, bits, *FP_HOST_SIZE, L, K), "host"))
    return out


def units_per_block(case):
    """{kernel_key: (slices per workgroup, slices of the launch, 256)}: a slice is 256 consecutive
    coefficients of one polynomial, a workgroup takes BconvArith<W>::kV = 4 (32-bit words) or 1
    (64-bit words) of them (csrc/bconv_dev.hpp:60, :86, `live[v]` :138; csrc/bconv.hip:11)."""
    return {bconv_kernel(case.op, case.n, case.bits): (4 if case.bits == 32 else 1,
                                                       case.batch * (case.n // 256), 256)}


def fp_guard_words(case):
    """The guard width tests/guarded.py gives the call: the widest batch entry is moddown's input,
    (K + L) * n words."""
    from guarded import guard_words
    return guard_words((case.K + case.L) * case.n)


# ---------------------------------------------------------------------------------------------
# The mirror
# ---------------------------------------------------------------------------------------------

def word_bits(from_q, to_q):
    """bconv.cpp validate: one word class over both bases, all primes distinct."""
    q = tuple(from_q) + tuple(to_q)
    assert 1 <= len(from_q) <= 64 and 1 <= len(to_q) <= 64 and len(set(q)) == len(q)
    if all(v < (1 << 31) for v in q):
        return 32
    assert all((1 << 32) <= v < (1 << 62) for v in q), "mixed classes are NTTMUL_EUNSUPPORTED"
    return 64


def bconv_kernel(op, n, bits):
    """bconv.hip dispatch: one kernel per word size and operation, for every n, L and K."""
    assert n & (n - 1) == 0 and 256 <= n <= 4096, "n > 4096 is NTTMUL_EUNSUPPORTED"
    return f"k_bconv<{'u32' if bits == 32 else 'u64'},{OPS.index(op)}>"


def kernels_of(case):
    """The kernel_keys `case` launches, in launch order (with NTTMUL_FLAG_VALIDATE the range check
    of libnttmul_rns.so runs first, once: a conversion reads one operand)."""
    io = "u32" if case.bits == 32 else "u64"
    return ([f"k_rns_check_range<{io}>"] if case.validate else []) + \
        [bconv_kernel(case.op, case.n, case.bits)]


# Kernels of libnttmul_bconv.so beyond libnttmul_rns.so's that no call can launch: (regular
# expression over the kernel_key, reason).  None: bconv.hip instantiates only what dispatch reaches.
UNREACHABLE = ()
