"""Case tables of tests/test_gpu_mac.py and a pure-Python mirror of the dispatch behind
include/nttmul_mac.h (csrc/mac.hip mac_dispatch): plain data and arithmetic, no GPU, no library.

tests/test_mac_ledger.py holds the mirror against the cross-compiled lib/libnttmul_mac.so (the
kernels it holds beyond libnttmul.so's are exactly the ones the mirror names over these cases);
test_gpu_mac.py::test_mirror_agrees_with_the_library_dispatch anchors it on the GPU to the
library's own dry run (nttmul_mac_kernel_name)."""
from collections import namedtuple

import dispatch_cases as D

MAC_N = (256, 512, 1024, 2048, 4096)
# a partial last block at every n: 256 / (n / 16) = 16, 8, 4, 2, 1 polynomials per block
BATCH = 17
# one modulus per arithmetic class at every n; the Plantard class rotates through its three
PLANTARD_AT = {256: D.Q31HI, 512: D.Q31LO, 1024: D.Q20, 2048: D.Q31HI, 4096: D.Q31LO}
TERMS = (1, 3)
TERMS_LONG = 7              # added at the smallest and the largest n
LONG_N = (256, 4096)

# op "mac": one nttmul_mac_ntt_* call
Case = namedtuple("Case", "n q word_bits terms shared batch validate", defaults=(BATCH, False))


def moduli_at(n):
    return (PLANTARD_AT[n], D.Q32, D.Q62)


def terms_at(n):
    return TERMS + ((TERMS_LONG,) if n in LONG_N else ())


def parity_cases():
    """Test 1: every n, one modulus per class, every word width, terms, shared and per-batch."""
    return [Case(n, q, w, t, s) for n in MAC_N for q in moduli_at(n) for w in D.word_options(q)
            for t in terms_at(n) for s in (False, True)]


# Test 2: worst-case ranges (every word q - 1) at terms = 7; the 31-bit entry None stands for
# 2^31 - 1 where it is a usable prime for n, else the largest prime below 2^31 with 2n | q - 1
RANGE_N = LONG_N
RANGE_MODULI = (D.Q31HI, None, D.Q32, D.Q62)
RANGE_BATCH = 3
# Test 3: cyclic contexts (n, q, omega; q None: the largest 31-bit prime with n | q - 1)
CYCLIC = ((256, 12289, 8595), (1024, None, 0))
CYCLIC_TERMS = 2
# Test 4: the device-path rules
RULES = (1024, D.Q31, 32)
VALIDATE = (512, D.Q31HI, 32)
UNSUPPORTED_N = 8192
# Test 5: host forms
HOST = (1024, 5, 3)         # n, batch, terms


def all_cases():
    out = parity_cases()
    out += [Case(n, q, D.native_bits(q), TERMS_LONG, s, RANGE_BATCH)
            for n in RANGE_N for q in RANGE_MODULI if q for s in (False, True)]
    # saturated operands (tests/test_gpu_saturation.py): S(1, q - 1) against b_hat = q - 1
    out += [Case(n, q, D.native_bits(q), D.SAT_MAC_TERMS, s, RANGE_BATCH)
            for n in D.SAT_MAC_N for q in D.sat_moduli(n) for s in (False, True)]
    n, q, w = RULES
    out += [Case(n, q, w, 2, s, 5) for s in (False, True)]
    n, q, w = VALIDATE
    out.append(Case(n, q, w, 2, False, 3, validate=True))
    n, batch, terms = HOST
    out += [Case(n, q, w, terms, False, batch) for q in moduli_at(n) for w in D.word_options(q)]
    out += [f.case for f in footprint_cases()]
    # the launches that fill the GPU twice over (tests/test_gpu_scale.py, tests/scale_cases.py)
    import scale_cases
    out += scale_cases.cases_of("mac")
    return out


# The caller's memory (tests/test_gpu_footprint.py): the smallest and the largest n, terms 3,
# batch 1 and 33 (one live polynomial in the last block of 16 at n = 256), shared and per-batch
# b_hat, one modulus per class in every word width; the host forms at the same n with batch 3.
# host: "" for nttmul_mac_ntt_device, "host" for nttmul_mac_ntt_u32 / _u64.
Footprint = namedtuple("Footprint", "entry case host", defaults=("",))
FP_N = (256, 4096)
FP_TERMS = 3
FP_BATCHES = (1, 33)
FP_HOST_BATCH = 3


def footprint_cases():
    out = []
    for n in FP_N:
        for q in moduli_at(n):
            for w in D.word_options(q):
                out += [Footprint("nttmul_mac_ntt_device", Case(n, q, w, FP_TERMS, s, batch))
                        for batch in FP_BATCHES for s in (False, True)]
                out += [Footprint(f"nttmul_mac_ntt_u{w}", Case(n, q, w, FP_TERMS, s, FP_HOST_BATCH),
                                  "host") for s in (False, True)]
    return out


def units_per_block(case):
    """{kernel_key: (polynomials per workgroup, polynomials of the launch, words per polynomial)}:
    k_mac takes PB = 256 / (n / 16) output polynomials per 256-thread workgroup
    (csrc/mac_dev.hpp:52, `live` :56); the range check one word per thread."""
    io = "u32" if case.word_bits == 32 else "u64"
    out = {mac_kernel(case.n, case.q, case.word_bits): (256 // (case.n // 16), case.batch, case.n)}
    if case.validate:
        out[f"k_check_range<{io}>"] = (256, case.batch * case.terms * case.n, 1)
    return out


def fp_guard_words(case):
    """The guard width tests/guarded.py gives the call: a's batch entry is terms * n words."""
    from guarded import guard_words
    return guard_words(case.terms * case.n)


# ---------------------------------------------------------------------------------------------
# The mirror
# ---------------------------------------------------------------------------------------------

def mac_kernel(n, q, word_bits):
    """mac.hip mac_dispatch: the class follows q alone (plain Arith32P at n = 4096 too), one
    kernel per (class, caller word, n); shared operands are a stride of the same kernel."""
    assert word_bits == 64 or q < (1 << 32), "io_ok refuses 32-bit words for q >= 2^32"
    assert n & (n - 1) == 0 and 256 <= n <= 4096, "n > 4096 is NTTMUL_EUNSUPPORTED"
    io = "u32" if word_bits == 32 else "u64"
    return f"k_mac<{D.arith_class(q)},{io},{io},{n.bit_length() - 1}>"


def kernels_of(case):
    """The kernel_keys `case` launches, in launch order (the range check runs once per operand)."""
    io = "u32" if case.word_bits == 32 else "u64"
    return ([f"k_check_range<{io}>"] * 2 if case.validate else []) + \
        [mac_kernel(case.n, case.q, case.word_bits)]


# Kernels of libnttmul_mac.so beyond libnttmul.so's that no call can launch: (regular expression
# over the kernel_key, reason).  None: mac.hip instantiates only what mac_dispatch reaches.
UNREACHABLE = ()
