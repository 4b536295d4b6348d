"""Case tables of tests/test_gpu_galois.py and test_gpu_galois_footprint.py, and a pure-Python
mirror of the dispatch behind include/nttmul_galois.h (csrc/galois.hip dispatch, csrc/galois.cpp
run): plain data and arithmetic, no GPU, no library.

tests/test_galois_ledger.py holds the mirror against the cross-compiled lib/libnttmul_galois.so
(the kernels it holds beyond libnttmul_rnsmp.so's are exactly the ones the mirror names over these
cases); test_gpu_galois.py::test_mirror_agrees_with_the_library_dispatch anchors it on the GPU to
the library's own dry run (nttmul_galois_kernel_name)."""
from collections import namedtuple

import galois_ref as ref
import rnsmp_cases as P

# several polynomials per workgroup, the single-pass limit, the first multi-pass n, and the n where
# index products wrap 32 bits and a limb polynomial exceeds the LDS of a compute unit
GALOIS_N = (256, 4096, 8192, 65536)
ALL_N = tuple(1 << e for e in range(8, 17))
BASES = P.BASES                              # every prime is 1 mod 2^17: the bases serve every n
LIMBS = (1, 3)                               # prefixes of a basis
BATCHES = (3, 1)
COUNTS = (1, 3, 16)
MAX_COUNT = 16
OPS = ("coeff", "ntt", "ntt_many")           # nttmul_galois_kernel_name's op numbers
ENTRY = {"coeff": "nttmul_galois_coeff", "ntt": "nttmul_galois_ntt",
         "ntt_many": "nttmul_galois_ntt_many"}

# ks: the automorphisms of the call (one for coeff and ntt)
Case = namedtuple("Case", "op n moduli batch ks validate", defaults=(False,))


def ks_at(n):
    """1 (a copy), 3, n - 1, n + 1 (k r wraps n), 2n - 1 (the conjugation: the largest k, whose
    products wrap 32 bits at n = 65536), one rotation step, three steps back."""
    return (1, 3, n - 1, n + 1, 2 * n - 1, ref.element(n, 1), ref.element(n, -3))


def many_ks(n, count):
    """`count` automorphisms: ks_at(n), then further powers of 5."""
    ks = list(ks_at(n)) + [ref.element(n, s) for s in range(2, 2 + MAX_COUNT)]
    return tuple(ks[:count])


def bases_at(n):
    return [basis[:k] for basis in BASES for k in LIMBS]


def shapes():
    """(n, moduli, batch): every n, both word classes, L in {1, 3}, batch 3 and 1."""
    return [(n, m, batch) for n in GALOIS_N for m in bases_at(n) for batch in BATCHES]


# The coefficient kernel takes another path at every n where a limb polynomial is split in more
# residue classes (coeff_lgm below), and where a stage above 64 KiB needs the raised LDS limit:
# besides 65536 these two.  On 32-bit words 32768 is the largest n staged whole; on 64-bit words
# that is 16384, and 32768 the first split in two.  L = 3, batch 3.
SPLIT_N = (16384, 32768)
SPLIT_BATCH = 3


def split_shapes():
    return [(n, basis, SPLIT_BATCH) for n in SPLIT_N for basis in BASES]


def parity_cases():
    out = []
    for n, m, batch in shapes():
        out += [Case(op, n, m, batch, (k,)) for op in OPS[:2] for k in ks_at(n)]
        out += [Case("ntt_many", n, m, batch, many_ks(n, c)) for c in COUNTS]
    for n, m, batch in split_shapes():
        out += [Case("coeff", n, m, batch, (k,)) for k in ks_at(n)]
    return out


# NTTMUL_FLAG_VALIDATE, one basis per class: (n, moduli, the limb whose own modulus the bad word
# equals, a limb with a larger modulus where the same value is in range)
VALIDATE = ((256, P.BASIS32, 2, 0), (8192, P.BASIS64, 2, 0))
STREAM = (4096, P.BASIS32)                   # a non-default stream
HOST = ((4096, P.BASIS32), (8192, P.BASIS64))        # host forms: one n per class
HOST_BATCH = 5

# The caller's memory (tests/test_gpu_galois_footprint.py): the three device calls and the two
# host forms at the smallest and the largest n, L = 3, both word classes, batch 1 and 5 (5 at
# n = 256: one whole workgroup of four polynomials and a partial one).  host: "" for a *_device
# call, "host" for the host form.
Footprint = namedtuple("Footprint", "entry case host", defaults=("",))
FP_N = (256, 65536)
FP_BATCHES = (1, 5)
FP_COUNT = 3


def footprint_cases():
    out = []
    for n in FP_N:
        k = ref.element(n, 1)
        for m in BASES:
            for batch in FP_BATCHES:
                out += [Footprint(ENTRY[op] + "_device", Case(op, n, m, batch, (k,)))
                        for op in OPS[:2]]
                out.append(Footprint(ENTRY["ntt_many"] + "_device",
                                     Case("ntt_many", n, m, batch, many_ks(n, FP_COUNT))))
                out += [Footprint(ENTRY[op], Case(op, n, m, batch, (k,)), "host")
                        for op in OPS[:2]]
    return out


def all_cases():
    out = parity_cases()
    for n, m, _, _ in VALIDATE:
        out += [Case(op, n, m, 3, many_ks(n, 2) if op == "ntt_many" else (3,), True) for op in OPS]
    n, m = STREAM
    out += [Case(op, n, m, 3, many_ks(n, 3) if op == "ntt_many" else (5,)) for op in OPS]
    out += [Case(op, n, m, HOST_BATCH, (ref.element(n, 1),)) for n, m in HOST for op in OPS[:2]]
    out += [f.case for f in footprint_cases()]
    # the launches that fill the GPU twice over (tests/test_gpu_scale.py, tests/scale_cases.py)
    import scale_cases
    out += scale_cases.cases_of("galois")
    return out


def fp_guard_words(case):
    """The guard width tests/guarded.py gives the call: the widest batch entry is limbs * n words,
    and no workgroup spans more than max(n, 1024) words of one limb."""
    from guarded import guard_words
    return guard_words(len(case.moduli) * max(case.n, STAGE_WORDS))


# ---------------------------------------------------------------------------------------------
# The mirror
# ---------------------------------------------------------------------------------------------

SLICE = 256                                  # words of one slice (galois_dev.hpp)
SLICES = 4                                   # kGaloisSlices: slices per workgroup
STAGE_WORDS = 1024                           # kGaloisStage: fewest words the staged form takes
LDS_BYTES = 128 << 10                        # kGaloisLdsBytes


def word_bits(moduli):
    """galois.cpp nttmul_galois_create: one word class per context."""
    assert 1 <= len(moduli) <= 64 and len(set(moduli)) == len(moduli)
    if all(q < (1 << 31) for q in moduli):
        return 32
    assert all((1 << 32) <= q < (1 << 62) for q in moduli), "mixed classes are NTTMUL_EUNSUPPORTED"
    return 64


def coeff_lgm(n, bits):
    """galois.hip coeff_lgm: log2 of the residue classes mod M a limb polynomial is split in, the
    fewest whose n / M words fit the 128 KiB stage: 0 up to n = 32768 on 32-bit words and
    n = 16384 on 64-bit words, 1 and 2 at n = 65536."""
    lgm = 0
    while (n * (bits // 8)) >> lgm > LDS_BYTES:
        lgm += 1
    return lgm


def kernel_name(op, n, moduli):
    """What nttmul_galois_kernel_name returns: one kernel per call."""
    assert n in ALL_N, "n > 65536 is NTTMUL_EUNSUPPORTED"
    bits = word_bits(moduli)
    io = "u32" if bits == 32 else "u64"
    if op == "coeff":
        return f"k_galois_coeff<{io},{coeff_lgm(n, bits)}>"
    assert op in ("ntt", "ntt_many")
    return f"k_galois_{op}<{io}>"


def kernels_of(case):
    """The kernel_keys `case` launches, in launch order: with NTTMUL_FLAG_VALIDATE the range check
    of the input (libnttmul_rns.so's kernel, common to the libraries), then the one launch."""
    assert 1 <= len(case.ks) <= (MAX_COUNT if case.op == "ntt_many" else 1)
    assert all(k % 2 == 1 and 0 < k < 2 * case.n for k in case.ks)
    io = "u32" if word_bits(case.moduli) == 32 else "u64"
    return ([f"k_rns_check_range<{io}>"] if case.validate else []) + \
        [kernel_name(case.op, case.n, case.moduli)]


def units_per_block(case):
    """{kernel_key: (units per workgroup and limb, units of the launch, words per unit and limb)};
    the limb is a grid dimension.  The coefficient kernel takes whole polynomials, 1024 / n of them
    below n = 1024, or one residue class of one polynomial (n / M words of it, M apart) where it
    splits; every other kernel takes four slices of 256 words, which at n = 256 are four
    polynomials."""
    key = kernel_name(case.op, case.n, case.moduli)
    if key.startswith("k_galois_coeff"):
        lgm = coeff_lgm(case.n, word_bits(case.moduli))
        if lgm:
            return {key: (1, case.batch << lgm, case.n >> lgm)}
        return {key: (max(1, STAGE_WORDS // case.n), case.batch, case.n)}
    return {key: (SLICES, case.batch * case.n // SLICE, SLICE)}


def polys_per_block(case):
    """Polynomials of one limb a workgroup of the case's kernel holds."""
    (per, _, words), = units_per_block(case).values()
    return max(1, per * words // case.n)


# Kernels of libnttmul_galois.so beyond libnttmul_rnsmp.so's that no call can launch: (regular
# expression over the kernel_key, reason).  None: galois.hip instantiates only what dispatch
# reaches.
UNREACHABLE = ()
