"""Case tables of tests/test_gpu_macn.py and test_gpu_macn_footprint.py, and a pure-Python mirror of
the dispatch behind include/nttmul_macn.h (csrc/macn.hip, csrc/macn.cpp, and the sub-batch rule of
csrc/subbatch.hpp as csrc/rnsmp.cpp run applies it): plain data and arithmetic, no GPU, no library.

tests/test_macn_ledger.py holds the mirror against the cross-compiled lib/libnttmul_macn.so (the
kernels it holds beyond libnttmul_ks.so's are exactly the ones the mirror names over these cases);
test_gpu_macn.py::test_mirror_names_the_kernels_the_library_names anchors it on the GPU to the
library's own dry run (nttmul_rns_macn_kernel_name, nttmul_rnsmp_macn_kernel_name).

A case's family follows its degree: n <= 4096 is nttmul_rns (tests/rns_cases.py: batch 17 leaves a
partial last workgroup at every n <= 2048), n >= 8192 is nttmul_rnsmp (tests/rnsmp_cases.py:
batch 3).  The bases, limb counts and term counts are those two modules'."""
from collections import namedtuple

import ks_cases as K
import rns_cases as R
import rnsmp_cases as M

MAX_COMPS = 2                                # NTTMUL_MACN_MAX_COMPS
ALL_N = R.RNS_N + M.RNSMP_N
ORACLE_N = (256, 4096, 8192, 65536)          # parity with the CPU oracle
ORACLE_BATCH, ORACLE_TERMS, ORACLE_LIMBS = 2, 3, 2
RANGE_N = (256, 4096, 8192, 65536)           # every word at the top of its range
RANGE_TERMS = 7
VALIDATE = R.VALIDATE[:2] + M.VALIDATE[:2]   # (n, moduli, limb of the bad word, a limb above it)
VALIDATE_BATCH, VALIDATE_TERMS = 3, 2
HOST = R.HOST + M.HOST                       # host forms: one n per class and family
HOST_BATCH, HOST_TERMS = 5, 3
STREAMS = M.RULES                            # two streams and a growing scratch
STREAMS_BATCHES, STREAMS_TERMS = M.LIFETIME_BATCHES, M.LIFETIME_TERMS
CHAIN, CHAIN_SHAPE, CHAIN_BATCH, CHAIN_H = K.CHAIN, K.CHAIN_SHAPE, K.CHAIN_BATCH, K.CHAIN_H
# Sub-batches with scratch_mb = 1 at n = 8192, three 32-bit limbs (96 KiB per polynomial and
# buffer, tests/rnsmp_cases.py SUBBATCH row 0): (n, moduli, terms, batch, chunks with comps = 2).
# terms = 3: a's 288 KiB per batch entry bound the chunk, as for mac_ntt; terms = 1: the two
# output polynomials, 192 KiB, bound it (mac_ntt's own rule would take 10 polynomials at a time)
SUBBATCH = (
    (M.SUBBATCH[0][0], M.SUBBATCH[0][1], M.SUBBATCH[0][4], M.SUBBATCH[0][5], (3, 3, 2)),
    (M.SUBBATCH[0][0], M.SUBBATCH[0][1], 1, 11, (5, 5, 1)),
)

Case = namedtuple("Case", "n moduli batch terms comps shared validate scratch_mb",
                  defaults=(2, True, False, 0))


def family(n):
    assert n in ALL_N, "n < 256 is NTTMUL_EINVAL, n > 65536 NTTMUL_EUNSUPPORTED, at create"
    return "rns" if n <= 4096 else "rnsmp"


def cases_of(n):
    return R if family(n) == "rns" else M


def equality_cases():
    """Every n and both word classes, the family's batch, L in {1, 3} (and five 32-bit limbs at two
    n per family), terms 1 and 3 (7 at the same n), shared and per-batch b_hat, comps = 2; and
    comps = 1 once per (n, basis)."""
    out = []
    for n in ALL_N:
        T = cases_of(n)
        for m in T.bases_at(n):
            out += [Case(n, m, T.BATCH, t, 2, s) for t in T.terms_at(n) for s in (True, False)]
            out.append(Case(n, m, T.BATCH, T.TERMS[-1], 1, True))
    return out


def subbatch_cases():
    return [Case(n, m, batch, terms, 2, s, False, 1) for n, m, terms, batch, _ in SUBBATCH
            for s in (True, False)]


# The caller's memory (tests/test_gpu_macn_footprint.py): the four writing entry points, both word
# classes, L = 3, terms 3, comps 2, shared and per-batch.  n = 256 with batch 1 and 5 (a workgroup
# holds 16 polynomials: both end in a partial one), n = 4096 with batch 1, n = 8192 with batch 1
# and 5.  host: "" for a *_device call, "host" for the host form.
Footprint = namedtuple("Footprint", "entry case host", defaults=("",))
FP_SIZES = ((256, 1), (256, 5), (4096, 1), (8192, 1), (8192, 5))
FP_TERMS = 3


def footprint_cases():
    out = []
    for n, batch in FP_SIZES:
        for m in cases_of(n).BASES:
            for s in (True, False):
                case = Case(n, m, batch, FP_TERMS, 2, s)
                out.append(Footprint(f"nttmul_{family(n)}_macn_ntt_device", case))
                out.append(Footprint(f"nttmul_{family(n)}_macn_ntt", case, "host"))
    return out


def all_cases():
    out = equality_cases()
    for n in ORACLE_N:
        out += [Case(n, b[:ORACLE_LIMBS], ORACLE_BATCH, ORACLE_TERMS, 2, s)
                for b in cases_of(n).BASES for s in (True, False)]
    out += [Case(n, b, cases_of(n).RANGE_BATCH, RANGE_TERMS, c) for n in RANGE_N
            for b in cases_of(n).BASES for c in (1, 2)]
    out += subbatch_cases()
    out += [Case(n, m, VALIDATE_BATCH, VALIDATE_TERMS, 2, True, True) for n, m, _, _ in VALIDATE]
    out += [Case(n, m, HOST_BATCH, HOST_TERMS, c, s) for n, m in HOST for c in (1, 2)
            for s in (True, False)]
    out += [Case(STREAMS[0], STREAMS[1], b, STREAMS_TERMS, 2) for b in STREAMS_BATCHES]
    L, P, alpha = CHAIN_SHAPE
    import ks_ref
    for n, _ in CHAIN:
        for bits in (32, 64):
            q, p = ks_ref.bases(bits, L, P)
            out.append(Case(n, q + p, CHAIN_BATCH, -(-L // alpha), 2, True))
    out += [f.case for f in footprint_cases()]
    # the launches that fill the GPU twice over (tests/test_gpu_scale.py, tests/scale_cases.py)
    import scale_cases
    out += scale_cases.cases_of("macn")
    return out


def fp_guard_words(case):
    """The guard width tests/guarded.py gives the call: the widest batch entry is b_hat's,
    comps * terms * limbs * n words."""
    from guarded import guard_words
    return guard_words(case.comps * case.terms * len(case.moduli) * case.n)


# ---------------------------------------------------------------------------------------------
# The mirror
# ---------------------------------------------------------------------------------------------

def word_bits(moduli):
    return R.word_bits(moduli)


def macn_kernel(n, moduli):
    """macn.hip: the one new kernel per (class, n) with comps = 2.  The class follows the word size
    alone, as the mac's (plain Arith32P at n = 4096 too: a full transform has no base blocks)."""
    cls, io = ("Arith32P", "u32") if word_bits(moduli) == 32 else ("Arith64", "u64")
    if family(n) == "rns":
        return f"k_rns_macn<{cls},{io},{n.bit_length() - 1},2>"
    return f"k_rnsmp_macn<{cls},{io},{M.l1_of(n)},2>"


def sequence(n, moduli, comps):
    """The launches of one call (n <= 4096) or of one sub-batch (above), in order.  comps = 1 is
    the context's own mac; comps = 2 replaces its one mac kernel and keeps the column passes."""
    assert 1 <= comps <= MAX_COMPS, "NTTMUL_EINVAL"
    if family(n) == "rns":
        return [R.rns_kernel("mac", n, moduli) if comps == 1 else macn_kernel(n, moduli)]
    seq = M.sequence("mac", n, moduli)
    return seq if comps == 1 else [seq[0], macn_kernel(n, moduli), seq[2]]


def kernel_name(n, moduli, comps):
    """What nttmul_rns_macn_kernel_name / nttmul_rnsmp_macn_kernel_name return."""
    return " + ".join(sequence(n, moduli, comps))


def chunks(case):
    """rnsmp.cpp run with subbatch.hpp mp_chunk: the largest polynomial count for which neither
    chunk * terms nor chunk * comps polynomials (all limbs) exceed scratch_mb MiB, never less than
    one.  One chunk at n <= 4096: no scratch."""
    if family(case.n) == "rns":
        return [case.batch]
    poly = len(case.moduli) * case.n * (word_bits(case.moduli) // 8)
    limit = (case.scratch_mb or M.DEFAULT_SCRATCH_MB) << 20
    chunk = max(1, min(case.batch, limit // (poly * max(case.terms, case.comps))))
    return [min(chunk, case.batch - p) for p in range(0, case.batch, chunk)]


def kernels_of(case):
    """The kernel_keys `case` launches, in launch order: with NTTMUL_FLAG_VALIDATE the range check
    once per operand read (a, then all of b_hat), then the sequence once per sub-batch."""
    io = "u32" if word_bits(case.moduli) == 32 else "u64"
    return ([f"k_rns_check_range<{io}>"] * 2 if case.validate else []) + \
        sequence(case.n, case.moduli, case.comps) * len(chunks(case))


def units_per_block(case):
    """{kernel_key: (units per workgroup and limb, units of the launch, words per unit and limb)}
    of the new kernel for the whole batch: k_rns_macn 256 / (n / 16) output polynomials (of comps
    components each) per workgroup (csrc/macn_dev.hpp `live`), k_rnsmp_macn one row of 4096."""
    if family(case.n) == "rns":
        return {macn_kernel(case.n, case.moduli): (256 // (case.n // 16), case.batch, case.n)}
    return {macn_kernel(case.n, case.moduli): (1, case.batch << M.l1_of(case.n), 4096)}


# Kernels of libnttmul_macn.so beyond libnttmul_ks.so's that no call can launch: (regular expression
# over the kernel_key, reason).  None: macn.hip instantiates only what dispatch reaches.
UNREACHABLE = ()
