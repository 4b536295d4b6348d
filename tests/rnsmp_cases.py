"""Case tables of tests/test_gpu_rnsmp.py and test_gpu_rnsmp_footprint.py, and a pure-Python mirror
of the dispatch behind include/nttmul_rnsmp.h (csrc/rnsmp.hip passes / dispatch, csrc/rnsmp.cpp
run): plain data and arithmetic, no GPU, no library.

tests/test_rnsmp_ledger.py holds the mirror against the cross-compiled lib/libnttmul_rnsmp.so (the
kernels it holds beyond libnttmul_bconv.so's are exactly the ones the mirror names over these
cases); test_gpu_rnsmp.py::test_mirror_agrees_with_the_library_dispatch anchors it on the GPU to
the library's own dry run (nttmul_rnsmp_kernel_name)."""
from collections import namedtuple

import dispatch_cases as D

RNSMP_N = (8192, 16384, 32768, 65536)
# every row kernel takes one row of 4096 per workgroup and every column workgroup 256 columns of
# one polynomial, so no batch leaves a partial workgroup: 3 is "more than one, not a power of two"
BATCH = 3
# primes with 2 * 65536 | q - 1, so each basis serves every n.  P61 and P60 are
# nttmul_find_prime(65536, 61) and (65536, 60); rns_cases.P61 has q - 1 = 2^13 * odd only
P61 = 2305843009211596801
P60 = 1152921504606584833
BASIS32 = (D.Q31, D.Q31HI, D.Q31LO)          # every q < 2^31: 32-bit words
BASIS32_5 = BASIS32 + (D.Q30, D.Q20)
BASIS64 = (D.Q62, P61, P60)                  # every q >= 2^32: 64-bit words
BASES = (BASIS32, BASIS64)
LIMBS = (1, 3)                               # prefixes of a basis
FIVE_N = (8192, 65536)                       # the five-limb case
TERMS = (1, 3)
TERMS_LONG = 7                               # added at the smallest and the largest n
LONG_N = (8192, 65536)
OPS = ("multiply", "forward", "inverse", "mac")      # nttmul_rnsmp_kernel_name's op numbers
DEFAULT_SCRATCH_MB = 512

Case = namedtuple("Case", "op n moduli batch terms shared validate scratch_mb",
                  defaults=(BATCH, 1, False, False, 0))


def terms_at(n):
    return TERMS + ((TERMS_LONG,) if n in LONG_N else ())


def bases_at(n):
    """The moduli lists tested at n: L = 1 and 3 of each class, and five 32-bit limbs at two n."""
    out = [basis[:k] for basis in BASES for k in LIMBS]
    return out + ([BASIS32_5] if n in FIVE_N else [])


def parity_cases():
    """Every n, both word classes, L in {1, 3} (and 5), batch 3 and 1; the mac with terms 1 and 3
    (7 at two n), shared and per-batch."""
    out = []
    for n in RNSMP_N:
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
VALIDATE = ((8192, BASIS32, 2, 0), (8192, BASIS64, 2, 0))
# a non-default stream, reversed basis, in-place transforms, the lifetime sequence
RULES = (8192, BASIS32)
HOST = ((8192, BASIS32), (16384, BASIS64))   # host forms: one n per class
HOST_BATCH, HOST_TERMS = 5, 3
# Sub-batches with scratch_mb = 1: (n, moduli, batch of product and transforms, their chunks,
# terms of the mac, its batch, its chunks).  3 * 8192 * 4 B = 96 KiB per polynomial and buffer:
# 10 polynomials per MiB, and 3 of a three-term mac's a (288 KiB each); 3 * 65536 * 8 B = 1.5 MiB:
# one polynomial exceeds the limit, the scratch grows to hold it
SUBBATCH = (
    (8192, BASIS32, 23, (10, 10, 3), 3, 8, (3, 3, 2)),
    (65536, BASIS64, 2, (1, 1), 3, 2, (1, 1)),
)
# the lifetime sequence raises its batch from the first to the second in the middle
LIFETIME_BATCHES = (2, 5)
LIFETIME_TERMS = 2


def subbatch_cases():
    out = []
    for n, m, batch, _, terms, mbatch, _ in SUBBATCH:
        out += [Case(op, n, m, batch, scratch_mb=1) for op in OPS[:3]]
        out += [Case("mac", n, m, mbatch, terms, s, scratch_mb=1) for s in (False, True)]
    return out


def all_cases():
    out = parity_cases()
    out += [Case(op, n, m, RANGE_BATCH, TERMS_LONG if op == "mac" else 1, s)
            for n in RANGE_N for m in BASES for op, s in (("multiply", False), ("mac", False),
                                                          ("mac", True))]
    for n, m, _, _ in VALIDATE:
        out += [Case(op, n, m, 3, 2 if op == "mac" else 1, False, True) for op in OPS]
    n, m = RULES
    out += [Case(op, n, m, b, LIFETIME_TERMS if op == "mac" else 1)
            for op in OPS for b in (5,) + LIFETIME_BATCHES]
    out += [Case(op, n, m, HOST_BATCH, HOST_TERMS if op == "mac" else 1, s)
            for n, m in HOST for op, s in [(o, False) for o in OPS] + [("mac", True)]]
    out += subbatch_cases()
    out += [f.case for f in footprint_cases()]
    # the launches that fill the GPU twice over (tests/test_gpu_scale.py, tests/scale_cases.py)
    import scale_cases
    out += scale_cases.cases_of("rnsmp")
    return out


# The caller's memory (tests/test_gpu_rnsmp_footprint.py): product, both transforms and the mac at
# the smallest and the largest n, L = 3, both word classes, batch 1 and 5 (5: no multiple of
# anything the addressing shifts or multiplies by); the transforms also in place; the host forms
# with batch 3.  alias: "" or "out=in"; host: "" for a *_device call, "host" for the host form.
Footprint = namedtuple("Footprint", "entry case alias host", defaults=("", ""))
FP_N = (8192, 65536)
FP_BATCHES = (1, 5)
FP_TERMS = 3
FP_HOST_BATCH = 3
ENTRY = {"multiply": "nttmul_rnsmp_multiply", "forward": "nttmul_rnsmp_forward",
         "inverse": "nttmul_rnsmp_inverse", "mac": "nttmul_rnsmp_mac_ntt"}


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


def fp_guard_words(case):
    """The guard width tests/guarded.py gives the call: the widest batch entry is
    terms * limbs * n words."""
    from guarded import guard_words
    return guard_words(case.terms * len(case.moduli) * case.n)


# ---------------------------------------------------------------------------------------------
# The mirror
# ---------------------------------------------------------------------------------------------

def word_bits(moduli):
    """rnsmp.cpp nttmul_rnsmp_create: one word class per context."""
    assert 1 <= len(moduli) <= 64 and len(set(moduli)) == len(moduli)
    if all(q < (1 << 31) for q in moduli):
        return 32
    assert all((1 << 32) <= q < (1 << 62) for q in moduli), "mixed classes are NTTMUL_EUNSUPPORTED"
    return 64


def l1_of(n):
    """rnsmp.hip dispatch: the 2^L1 x 4096 split, L1 = logn - 12, for both word classes."""
    assert n in RNSMP_N, "n <= 4096 and n > 65536 are NTTMUL_EUNSUPPORTED"
    return n.bit_length() - 1 - 12


def sequence(op, n, moduli):
    """rnsmp.hip passes: the launches of one sub-batch of an operation, in order.  The class
    follows the word size alone (plain Arith32P: no Arith32P3 above n = 4096); the mac is three
    launches for any number of terms, the transforms are two."""
    bits = word_bits(moduli)
    cls, io = ("Arith32P", "u32") if bits == 32 else ("Arith64", "u64")
    l1 = l1_of(n)
    cols_fwd = lambda npoly: f"k_rnsmp_cols_fwd<{cls},{io},{l1},{npoly}>"      # noqa: E731
    cols_inv = f"k_rnsmp_cols_inv<{cls},{io},{l1}>"
    if op == "multiply":
        return [cols_fwd(2), f"k_rnsmp_rows<{cls},{l1}>", cols_inv]
    if op == "forward":
        return [cols_fwd(1), f"k_rnsmp_xform<{cls},{io},{l1},0>"]
    if op == "inverse":
        return [f"k_rnsmp_xform<{cls},{io},{l1},1>", cols_inv]
    assert op == "mac"
    return [cols_fwd(1), f"k_rnsmp_mac<{cls},{io},{l1}>", cols_inv]


def kernel_name(op, n, moduli):
    """What nttmul_rnsmp_kernel_name returns: the sequence joined as nttmul_kernel_name joins a
    plain multi-pass product's."""
    return " + ".join(sequence(op, n, moduli))


def chunks(case):
    """rnsmp.cpp run: the sub-batches of a call.  At most scratch_mb MiB per scratch buffer, in
    whole polynomials (all limbs; for the mac's a, all terms as well), never less than one."""
    poly = len(case.moduli) * case.n * (word_bits(case.moduli) // 8)
    apoly = poly * case.terms if case.op == "mac" else poly
    limit = (case.scratch_mb or DEFAULT_SCRATCH_MB) << 20
    chunk = max(1, min(case.batch, limit // apoly))
    return [min(chunk, case.batch - p) for p in range(0, case.batch, chunk)]


def kernels_of(case):
    """The kernel_keys `case` launches, in launch order: with NTTMUL_FLAG_VALIDATE the range check
    (libnttmul_rns.so's kernel, common to both libraries) once per operand read, then the sequence
    once per sub-batch."""
    io = "u32" if word_bits(case.moduli) == 32 else "u64"
    operands = 2 if case.op in ("multiply", "mac") else 1
    return ([f"k_rns_check_range<{io}>"] * operands if case.validate else []) + \
        sequence(case.op, case.n, case.moduli) * len(chunks(case))


def units_per_block(case):
    """{kernel_key: (units per workgroup and limb, units of the launch, words per unit and limb)}
    for one sub-batch of the whole batch; the limb is a grid dimension.  Column kernels: 256
    threads = 256 columns of one polynomial, 16 workgroups per unit (rnsmp_dev.hpp `gid`); row
    kernels: one row of 4096 per workgroup (`u = blockIdx.x`).  No kernel shares a workgroup
    between units."""
    l1 = l1_of(case.n)
    out = {}
    for key in sequence(case.op, case.n, case.moduli):
        if key.startswith("k_rnsmp_cols_fwd") and case.op == "mac":
            out[key] = (1, case.batch * case.terms, case.n)
        elif key.startswith("k_rnsmp_cols"):
            out[key] = (1, case.batch, case.n)
        else:
            out[key] = (1, case.batch << l1, 4096)
    return out


# Kernels of libnttmul_rnsmp.so beyond libnttmul_bconv.so's that no call can launch: (regular
# expression over the kernel_key, reason).  None: rnsmp.hip instantiates only what dispatch reaches.
UNREACHABLE = ()
