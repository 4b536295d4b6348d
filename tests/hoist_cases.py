"""Case tables of tests/test_gpu_hoist.py and test_gpu_hoist_footprint.py, and a pure-Python mirror
of the dispatch behind include/nttmul_hoist.h (csrc/hoist.hip, csrc/hoist.cpp, and the sub-batch
rule of csrc/subbatch.hpp mp_unit_chunk as csrc/rnsmp.cpp run_units applies it): plain data and
arithmetic, no GPU, no library.

tests/test_hoist_ledger.py holds the mirror against the cross-compiled lib/libnttmul_hoist.so (the
kernels it holds beyond libnttmul_macn.so's are exactly the ones the mirror names over these
cases); test_gpu_hoist.py::test_mirror_names_the_kernels_the_library_names anchors it on the GPU
to the library's own dry run (nttmul_rns_hoist_kernel_name, nttmul_rnsmp_hoist_kernel_name).

A case's family follows its degree, as in tests/macn_cases.py: n <= 4096 is nttmul_rns (batch 17
leaves a partial last workgroup at n = 256 .. 2048), n >= 8192 is nttmul_rnsmp (batch 3).  The
bases, limb counts and term counts are tests/rns_cases.py's and rnsmp_cases.py's."""
from collections import namedtuple

import macn_cases as N
import rns_cases as R
import rnsmp_cases as M

MAX_COMPS = 2                                # NTTMUL_MACN_MAX_COMPS
MAX_ROTS = 16                                # NTTMUL_HOIST_MAX_ROTS = NTTMUL_GALOIS_MAX_COUNT
ALL_N = R.RNS_N + M.RNSMP_N
LIMBS = (1, 3)
ORACLE_N = (256, 4096, 8192, 65536)          # against Python integers
ORACLE_BATCH, ORACLE_TERMS, ORACLE_LIMBS = 2, 3, 2
RANGE_N = (256, 4096, 8192, 65536)           # every word at the top of its range
RANGE_TERMS = 7
VALIDATE = R.VALIDATE[:2] + M.VALIDATE[:2]   # (n, moduli, limb of the bad word, a limb above it)
VALIDATE_BATCH, VALIDATE_TERMS = 3, 2
HOST = R.HOST + M.HOST                       # host forms: one n per class and family
HOST_BATCH, HOST_TERMS = 5, 3
CHAIN, CHAIN_SHAPE, CHAIN_BATCH, CHAIN_H = N.CHAIN, N.CHAIN_SHAPE, N.CHAIN_BATCH, N.CHAIN_H
CHAIN_ROTS = 3

Case = namedtuple("Case", "n moduli batch terms comps ks validate scratch_mb",
                  defaults=(False, 0))


def family(n):
    return N.family(n)


def cases_of(n):
    return N.cases_of(n)


def word_bits(moduli):
    return R.word_bits(moduli)


def pool(n):
    """The rotations the tests draw from: the identity, one step, two steps, the conjugation and
    one step back (5^-1 mod 2n)."""
    return (1, 5, 25, 2 * n - 1, pow(5, -1, 2 * n))


def draw(n, rots, shift):
    """`rots` pairwise distinct rotations of the pool, from entry `shift` on."""
    ks = tuple(pool(n)[(shift + i) % 5] for i in range(rots))
    assert len(set(ks)) == rots <= 5 and all(k % 2 == 1 and 0 < k < 2 * n for k in ks)
    return ks


def equality_cases():
    """Every n and both word classes, the family's batch, L in {1, 3}, terms 1 and 3 (7 at the
    family's smallest and largest n); per term count one call with comps 2 and one with comps 1,
    one of them with three rotations and the other with one, alternating, so that both component
    counts meet both rotation counts at every (n, basis); the rotations walk the pool, so every k
    of it is used at every (n, basis)."""
    out = []
    for n in ALL_N:
        T = cases_of(n)
        for basis in T.BASES:
            for L in LIMBS:
                shift = 0
                for i, t in enumerate(T.terms_at(n)):
                    for comps, rots in (((2, 3), (1, 1)) if i % 2 == 0 else ((1, 3), (2, 1))):
                        out.append(Case(n, basis[:L], T.BATCH, t, comps, draw(n, rots, shift)))
                        shift += rots
    return out


# Sub-batches with scratch_mb = 1: (n, moduli, batch, terms, comps, rots, chunks in output units).
# n = 8192, three 32-bit limbs: 96 KiB per polynomial, so 5 units of two components per MiB and
# 10 of one; the borders fall inside a batch entry (unit 5 is (p, r) = (1, 2)).  n = 65536, three
# 64-bit limbs: 1.5 MiB per polynomial, one unit exceeds the limit and the scratch grows to hold it
SUBBATCH = (
    (8192, M.BASIS32, 4, 2, 2, 3, (5, 5, 2)),
    (8192, M.BASIS32, 7, 1, 1, 3, (10, 10, 1)),
    (65536, M.BASIS64, 2, 1, 1, 2, (1, 1, 1, 1)),
)


def subbatch_cases():
    return [Case(n, m, batch, terms, comps, draw(n, rots, 2), False, 1)
            for n, m, batch, terms, comps, rots, _ in SUBBATCH]


# The caller's memory (tests/test_gpu_hoist_footprint.py): the four writing entry points, both word
# classes, L = 3, terms 3, comps 2, three rotations.  n = 256 with batch 1 and 5 (a workgroup holds
# 16 polynomials: both end in a partial one), n = 4096 with batch 1, n = 8192 with batch 1 and 5.
# host: "" for a *_device call, "host" for the host form.
Footprint = namedtuple("Footprint", "entry case host", defaults=("",))
FP_SIZES = ((256, 1), (256, 5), (4096, 1), (8192, 1), (8192, 5))
FP_TERMS, FP_ROTS = 3, 3


def footprint_cases():
    out = []
    for n, batch in FP_SIZES:
        for m in cases_of(n).BASES:
            case = Case(n, m, batch, FP_TERMS, 2, draw(n, FP_ROTS, 1))
            out.append(Footprint(f"nttmul_{family(n)}_hoist_ntt_device", case))
            out.append(Footprint(f"nttmul_{family(n)}_hoist_ntt", case, "host"))
    return out


def all_cases():
    out = equality_cases()
    for n in ORACLE_N:
        out += [Case(n, b[:ORACLE_LIMBS], ORACLE_BATCH, ORACLE_TERMS, 2, (5, 2 * n - 1))
                for b in cases_of(n).BASES]
    out += [Case(n, b, cases_of(n).RANGE_BATCH, RANGE_TERMS, 2, (2 * n - 1, 5)) for n in RANGE_N
            for b in cases_of(n).BASES]
    out += subbatch_cases()
    out += [Case(n, m, VALIDATE_BATCH, VALIDATE_TERMS, 2, draw(n, 2, 3), True)
            for n, m, _, _ in VALIDATE]
    out += [Case(n, m, HOST_BATCH, HOST_TERMS, c, draw(n, 3, 1)) for n, m in HOST for c in (1, 2)]
    L, P, alpha = CHAIN_SHAPE
    import ks_ref
    for n, _ in CHAIN:
        for bits in (32, 64):
            q, p = ks_ref.bases(bits, L, P)
            out.append(Case(n, q + p, CHAIN_BATCH, -(-L // alpha), 2, draw(n, CHAIN_ROTS, 1)))
    out += [f.case for f in footprint_cases()]
    # the launches that fill the GPU twice over (tests/test_gpu_scale.py, tests/scale_cases.py)
    import scale_cases
    out += scale_cases.cases_of("hoist")
    return out


def fp_guard_words(case):
    """The guard width tests/guarded.py gives the call: the widest batch entry is c's,
    rots * comps * limbs * n words, or a_hat's, terms * limbs * n."""
    from guarded import guard_words
    poly = len(case.moduli) * case.n
    return guard_words(len(case.ks) * case.comps * poly, case.terms * poly)


# ---------------------------------------------------------------------------------------------
# The mirror
# ---------------------------------------------------------------------------------------------

def hoist_kernel(n, moduli, comps):
    """hoist.hip: one kernel per (class, n, comps).  The class follows the word size alone, as the
    mac's (plain Arith32P at n = 4096 too)."""
    assert 1 <= comps <= MAX_COMPS, "NTTMUL_EINVAL"
    cls, io = ("Arith32P", "u32") if word_bits(moduli) == 32 else ("Arith64", "u64")
    if family(n) == "rns":
        return f"k_rns_hoist<{cls},{io},{n.bit_length() - 1},{comps}>"
    return f"k_rnsmp_hoist<{cls},{io},{M.l1_of(n)},{comps}>"


def sequence(n, moduli, comps):
    """The launches of one call (n <= 4096) or of one sub-batch (above), in order: no forward
    column pass, the context's own inverse column pass."""
    if family(n) == "rns":
        return [hoist_kernel(n, moduli, comps)]
    return [hoist_kernel(n, moduli, comps), M.sequence("mac", n, moduli)[2]]


def kernel_name(n, moduli, comps):
    """What nttmul_rns_hoist_kernel_name / nttmul_rnsmp_hoist_kernel_name return."""
    return " + ".join(sequence(n, moduli, comps))


def chunks(case):
    """subbatch.hpp mp_unit_chunk as rnsmp.cpp run_units walks it: sub-batches of output units
    (p, r), the largest count whose count * comps polynomials (all limbs) fit scratch_mb MiB, never
    less than one.  One chunk at n <= 4096: no scratch."""
    units = case.batch * len(case.ks)
    if family(case.n) == "rns":
        return [units]
    poly = len(case.moduli) * case.n * (word_bits(case.moduli) // 8)
    limit = (case.scratch_mb or M.DEFAULT_SCRATCH_MB) << 20
    chunk = max(1, min(units, limit // (poly * case.comps)))
    return [min(chunk, units - u) for u in range(0, units, chunk)]


def kernels_of(case):
    """The kernel_keys `case` launches, in launch order: with NTTMUL_FLAG_VALIDATE the range check
    once per operand read (a_hat, then all of b_hat), then the sequence once per sub-batch."""
    io = "u32" if word_bits(case.moduli) == 32 else "u64"
    return ([f"k_rns_check_range<{io}>"] * 2 if case.validate else []) + \
        sequence(case.n, case.moduli, case.comps) * len(chunks(case))


def units_per_block(case):
    """{kernel_key: (units per workgroup and limb, units of the launch, words per unit and limb)}
    of the new kernel for the whole call: k_rns_hoist 256 / (n / 16) polynomials of one rotation
    per workgroup, ceil(batch / that) * rots workgroups (csrc/hoist_dev.hpp `live`); k_rnsmp_hoist
    one row of 4096 of one output unit."""
    key = hoist_kernel(case.n, case.moduli, case.comps)
    if family(case.n) == "rns":
        return {key: (256 // (case.n // 16), case.batch, case.n)}
    return {key: (1, (case.batch * len(case.ks)) << M.l1_of(case.n), 4096)}


def transforms(dnum, rots):
    """(hoisted, unhoisted) transforms per limb polynomial of `rots` rotations of one ciphertext:
    dnum forward and 2 rots inverse, against rots key switches of dnum forward and 2 inverse."""
    return dnum + 2 * rots, rots * (dnum + 2)


# Kernels of libnttmul_hoist.so beyond libnttmul_macn.so's that no call can launch: (regular
# expression over the kernel_key, reason).  None: hoist.hip instantiates only what dispatch reaches.
UNREACHABLE = ()
