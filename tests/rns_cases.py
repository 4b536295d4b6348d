"""Case tables of tests/test_gpu_rns.py and a pure-Python mirror of the dispatch behind
include/nttmul_rns.h (csrc/rns.hip dispatch): plain data and arithmetic, no GPU, no library.

tests/test_rns_ledger.py holds the mirror against the cross-compiled lib/libnttmul_rns.so (the
kernels it holds beyond libnttmul_mac.so's are exactly the ones the mirror names over these
cases); test_gpu_rns.py::test_mirror_agrees_with_the_library_dispatch anchors it on the GPU to the
library's own dry run (nttmul_rns_kernel_name)."""
from collections import namedtuple

import dispatch_cases as D

RNS_N = (256, 512, 1024, 2048, 4096)
# a partial last workgroup at every n <= 2048 (256 / (n / 16) = 16, 8, 4, 2 polynomials per block),
# and a half-empty last pair of the 32-bit transforms (two polynomials per thread group)
BATCH = 17
# primes with 2 * 4096 | q - 1, so each basis serves every n
P61 = 2305843009213554689
BASIS32 = (D.Q31, D.Q31HI, D.Q31LO)          # every q < 2^31: 32-bit words
BASIS32_5 = BASIS32 + (D.Q30, D.Q20)
BASIS64 = (D.Q62, P61, D.Q33)                # every q >= 2^32: 64-bit words
BASES = (BASIS32, BASIS64)
LIMBS = (1, 3)                               # prefixes of a basis
FIVE_N = (256, 4096)                         # the five-limb case
TERMS = (1, 3)
TERMS_LONG = 7                               # added at the smallest and the largest n
LONG_N = (256, 4096)
OPS = ("multiply", "forward", "inverse", "mac")      # nttmul_rns_kernel_name's op numbers

Case = namedtuple("Case", "op n moduli batch terms shared validate",
                  defaults=(BATCH, 1, False, False))


def terms_at(n):
    return TERMS + ((TERMS_LONG,) if n in LONG_N else ())


def bases_at(n):
    """The moduli lists tested at n: L = 1 and 3 of each class, and five 32-bit limbs at two n."""
    out = [basis[:k] for basis in BASES for k in LIMBS]
    return out + ([BASIS32_5] if n in FIVE_N else [])


def parity_cases():
    """Every n, both word classes, L in {1, 3} (and 5), batch 17 and 1; the mac with terms 1 and 3
    (7 at two n), shared and per-batch."""
    out = []
    for n in RNS_N:
        for m in bases_at(n):
            for batch in (BATCH, 1):
                out += [Case(op, n, m, batch) for op in OPS[:3]]
            out += [Case("mac", n, m, BATCH, t, s) for t in terms_at(n) for s in (False, True)]
            out.append(Case("mac", n, m, 1, max(terms_at(n))))
    return out


# worst-case range: every word q_l - 1, product and 7-term mac
RANGE_N = LONG_N
RANGE_BATCH = 3
# NTTMUL_FLAG_VALIDATE, one basis per class: (n, moduli, the limb whose own modulus the bad word
# equals, a limb with a larger modulus where the same value is in range)
VALIDATE = ((512, BASIS32, 2, 0), (256, BASIS64, 2, 0))
# a non-default stream, reversed basis, in-place transforms
RULES = (1024, BASIS32)
UNSUPPORTED_N = 8192
HOST = ((1024, BASIS32), (512, BASIS64))     # host forms: one n per class
HOST_BATCH, HOST_TERMS = 5, 3


def all_cases():
    out = parity_cases()
    out += [Case(op, n, m, RANGE_BATCH, TERMS_LONG if op == "mac" else 1, s)
            for n in RANGE_N for m in BASES for op, s in (("multiply", False), ("mac", False),
                                                          ("mac", True))]
    for n, m, _, _ in VALIDATE:
        out += [Case(op, n, m, 3, 2 if op == "mac" else 1, False, True) for op in OPS]
    n, m = RULES
    out += [Case(op, n, m, 5, 2 if op == "mac" else 1) for op in OPS]
    out += [Case(op, n, m, HOST_BATCH, HOST_TERMS if op == "mac" else 1, s)
            for n, m in HOST for op, s in [(o, False) for o in OPS] + [("mac", True)]]
    out += [f.case for f in footprint_cases()]
    # the launches that fill the GPU twice over (tests/test_gpu_scale.py, tests/scale_cases.py)
    import scale_cases
    out += scale_cases.cases_of("rns")
    return out


# The caller's memory (tests/test_gpu_footprint.py): product, both transforms and the mac at three
# n (1024 and 4096 on 32-bit words take the descriptor path, with the limb in the span base),
# L = 3, both word classes, batch 1 and 33; the transforms also in place; the host forms with
# batch 3.  alias: "" or "out=in"; host: "" for a *_device call, "host" for the host form.
Footprint = namedtuple("Footprint", "entry case alias host", defaults=("", ""))
FP_N = (256, 1024, 4096)
FP_BATCHES = (1, 33)
FP_TERMS = 3
FP_HOST_BATCH = 3
ENTRY = {"multiply": "nttmul_rns_multiply", "forward": "nttmul_rns_forward",
         "inverse": "nttmul_rns_inverse", "mac": "nttmul_rns_mac_ntt"}


def footprint_cases():
    out = []
    for n in FP_N:
        for m in BASES:
            for batch in FP_BATCHES:
                out += [Footprint(ENTRY[op] + "_device", Case(op, n, m, batch)) for op in OPS[:3]]
                out += [Footprint(ENTRY["mac"] + "_device", Case("mac", n, m, batch, FP_TERMS, s))
                        for s in (False, True)]
                out += [Footprint(ENTRY[op] + "_device", Case(op, n, m, batch), "out=in")
                        for op in ("forward", "inverse")]
            out += [Footprint(ENTRY[op], Case(op, n, m, FP_HOST_BATCH), host="host")
                    for op in OPS[:3]]
            out += [Footprint(ENTRY["mac"], Case("mac", n, m, FP_HOST_BATCH, FP_TERMS, s),
                              host="host") for s in (False, True)]
    return out


def units_per_block(case):
    """{kernel_key: (polynomials per workgroup and limb, polynomials of the launch, words per
    polynomial and limb)}; the limb is a grid dimension (csrc/rns.hip:57).  k_rns_rows:
    rows_threads(LOGS) / (n / 16), with rows_threads(10) = 64, else 256 (csrc/rns_dev.hpp:45,
    `live` :51; rns.hip:70); k_rns_xform: 256 / (n / 16) thread groups of xform_upg = 2
    polynomials on 32-bit words, else 1 (rns_dev.hpp:116, :118, `live` / `live2` :126;
    rns.hip:80); k_rns_mac: 256 / (n / 16) (rns_dev.hpp:178, `live` :184; rns.hip:91)."""
    n = case.n
    tp = n // 16
    if case.op == "multiply":
        upb = (64 if n == 1024 else 256) // tp
    elif case.op in ("forward", "inverse"):
        upb = 256 // tp * (2 if word_bits(case.moduli) == 32 else 1)
    else:
        upb = 256 // tp
    return {rns_kernel(case.op, n, case.moduli): (upb, case.batch, n)}


def fp_guard_words(case):
    """The guard width tests/guarded.py gives the call: the widest batch entry is
    terms * limbs * n words."""
    from guarded import guard_words
    return guard_words(case.terms * len(case.moduli) * case.n)


# ---------------------------------------------------------------------------------------------
# The mirror
# ---------------------------------------------------------------------------------------------

def word_bits(moduli):
    """rns.cpp nttmul_rns_create: one word class per context."""
    assert 1 <= len(moduli) <= 64 and len(set(moduli)) == len(moduli)
    if all(q < (1 << 31) for q in moduli):
        return 32
    assert all((1 << 32) <= q < (1 << 62) for q in moduli), "mixed classes are NTTMUL_EUNSUPPORTED"
    return 64


def rns_kernel(op, n, moduli):
    """rns.hip dispatch: one kernel per (class, n) and operation.  The class follows the word size
    alone; the product at n = 4096 on 32-bit words is Arith32P3, the transforms and the mac stay
    plain Arith32P there (a full transform has no base blocks)."""
    assert n & (n - 1) == 0 and 256 <= n <= 4096, "n > 4096 is NTTMUL_EUNSUPPORTED"
    bits = word_bits(moduli)
    cls, io = ("Arith32P", "u32") if bits == 32 else ("Arith64", "u64")
    logn = n.bit_length() - 1
    if op == "multiply":
        if bits == 32 and n == 4096:
            assert all(D.p3_fold_ok(q) for q in moduli)
            cls = "Arith32P3"
        return f"k_rns_rows<{cls},{io},{logn}>"
    if op in ("forward", "inverse"):
        return f"k_rns_xform<{cls},{io},{logn},{OPS.index(op) - 1}>"
    assert op == "mac"
    return f"k_rns_mac<{cls},{io},{logn}>"


def kernels_of(case):
    """The kernel_keys `case` launches, in launch order (with NTTMUL_FLAG_VALIDATE the range check
    runs once per operand read)."""
    io = "u32" if word_bits(case.moduli) == 32 else "u64"
    operands = 2 if case.op in ("multiply", "mac") else 1
    return ([f"k_rns_check_range<{io}>"] * operands if case.validate else []) + \
        [rns_kernel(case.op, case.n, case.moduli)]


# Kernels of libnttmul_rns.so beyond libnttmul_mac.so's that no call can launch: (regular
# expression over the kernel_key, reason).  None: rns.hip instantiates only what dispatch reaches.
UNREACHABLE = ()
