"""Case tables of tests/test_gpu_ksntt.py, test_gpu_ksntt_footprint.py and test_gpu_ksntt_scale.py,
and a pure-Python mirror of the dispatch behind include/nttmul_ksntt.h (csrc/ksntt.hip modup / mac,
csrc/ksntt.cpp run_modup, csrc/ksntt_plan.hpp ksntt_shape): plain data and arithmetic, no GPU.

tests/test_ksntt_ledger.py holds the mirror against the cross-compiled lib/libnttmul_ksntt.so (the
kernels it holds beyond libnttmul_mdntt.so's are exactly the ones the mirror names over these
cases); test_gpu_ksntt.py::test_mirror_agrees_with_the_library_dispatch anchors it on the GPU to
the library's own dry run (nttmul_ksntt_kernel_name).

The shapes are the smallest at which the kernels can go wrong.  At n = 256 a transform thread
group is 16 threads: a workgroup of the inverse holds 16 thread groups of two polynomials each on
32-bit words (32 polynomials) and of one on 64-bit words, a workgroup of k_ksntt_fwd 16
polynomials of one target (d, m), a workgroup of k_ksntt_mac four slices of 256 slots, that is
four polynomials: batch 3 is an odd batch with a half-empty pair and a partial workgroup, batch 33
a partial second (inverse, 32-bit), third or ninth workgroup.  The conversion sum folds every CADENCE
products; a digit of alpha limbs is its length."""
from collections import namedtuple

import bconv_cases as BC
import ks_ref

CADENCE = BC.CADENCE                         # csrc/bconv_dev.hpp BconvArith<W>::kCadence
ALL_N = tuple(1 << e for e in range(8, 17))
OPS = ("modup", "mac")                       # nttmul_ksntt_kernel_name's op numbers
MAX_COMPS, MAX_ROTS = 2, 16                  # NTTMUL_MACN_MAX_COMPS, NTTMUL_HOIST_MAX_ROTS
MAC_SLICES = 4                               # csrc/ksntt_dev.hpp kKsMacSlices
DEFAULT_SCRATCH_MB = 512

# A case names its bases (ks_ref.bases(bits, L, K)) and holds no prime
Up = namedtuple("Up", "bits n batch L K alpha validate scratch_mb", defaults=(False, 0))
Mac = namedtuple("Mac", "bits n batch L K terms comps ks validate", defaults=(False,))

N = 256
BATCHES = (3, 33)
# (L, K, alpha).  (5, 2, 2) and (3, 2, 2) end in a short digit; (12, 4, 5) crosses the fold cadence
# of both classes with a remainder in both (5 = 2 * 2 + 1 = 4 + 1) and ends in a digit of 2
SHAPES = ((1, 1, 1), (4, 2, 2), (5, 2, 2), (5, 3, 5), (6, 1, 1), (3, 2, 2), (12, 4, 5))
WIDE = ((60, 4, 15),)                        # batch 1
DEGREE_SHAPE = (4, 2, 2)                     # every n, batch 2 (1 at 65536)
RANGE_N = (256, 4096, 8192)                  # worst-case ranges, RANGE_SHAPE, batch 2
RANGE_SHAPE = (5, 2, 2)
RANGE_FILLS = ("top", "worst", "zero")
# (bits, n, L, K, alpha, batch, sub-batches) with scratch_mb = 1: y is L n words per polynomial
SUBBATCH = ((64, 4096, 3, 2, 2, 23, (10, 10, 3)), (32, 65536, 2, 1, 1, 5, (2, 2, 1)))
VALIDATE = (256, 2, (3, 2, 2))               # n, batch, shape
HOST = ((256, 5), (8192, 2))                 # (n, batch), HOST_SHAPE
HOST_SHAPE = (3, 2, 2)

MAC_N = (256, 4096, 8192, 65536)
MAC_BATCH = 3
MAC_SHAPE = (2, 1)                           # (L, K): M = 3 limbs
MAC_WORST_TERMS = 16
CHAIN_N = (256, 8192)                        # identity (C), on hoist_ref.chain


def rotations(n, count):
    """`count` pairwise distinct rotations: 5^i mod 2n, the identity first."""
    ks = tuple(pow(5, i, 2 * n) for i in range(count))
    assert len(set(ks)) == count and all(k % 2 == 1 and 0 < k < 2 * n for k in ks)
    return ks


def mac_lists(n):
    """The k lists of the issue: the plain mac, three rotations with the conjugation, sixteen."""
    return ((1,), (5, 2 * n - 1, 25), rotations(n, MAX_ROTS))


def moduli_of(case):
    """(q, p) of a case."""
    return ks_ref.bases(case.bits, case.L, case.K)


def dnum(case):
    return -(-case.L // case.alpha)


def modup_cases():
    out = []
    for bits in (32, 64):
        out += [Up(bits, N, b, *s) for b in BATCHES for s in SHAPES]
        out += [Up(bits, N, 1, *s) for s in WIDE]
        out += [Up(bits, n, 1 if n == 65536 else 2, *DEGREE_SHAPE) for n in ALL_N]
    return out


def mac_cases():
    """Per n and class: terms 1 and 3 with comps 1 and 2, each k list with each kernel
    instantiation's other argument (the identity and a real permutation under both comps)."""
    out = []
    L, K = MAC_SHAPE
    for bits in (32, 64):
        for n in MAC_N:
            one, three, many = mac_lists(n)
            out += [Mac(bits, n, MAC_BATCH, L, K, 1, 2, one),
                    Mac(bits, n, MAC_BATCH, L, K, 3, 1, one),
                    Mac(bits, n, MAC_BATCH, L, K, 3, 1, three),
                    Mac(bits, n, MAC_BATCH, L, K, 1, 2, three),
                    Mac(bits, n, MAC_BATCH, L, K, 3, 2, many),
                    Mac(bits, n, MAC_BATCH, L, K, 1, 1, many)]
    return out


def mac_worst_cases():
    L, K = MAC_SHAPE
    return [Mac(bits, n, 1, L, K, MAC_WORST_TERMS, 2, (5, 1)) for bits in (32, 64) for n in MAC_N]


def subbatch_cases():
    return [Up(bits, n, batch, L, K, alpha, False, 1)
            for bits, n, L, K, alpha, batch, _ in SUBBATCH]


# The caller's memory (tests/test_gpu_ksntt_footprint.py): host "" for the *_device call, "host"
# for the host form
Footprint = namedtuple("Footprint", "entry case host", defaults=("",))
FP_SHAPES = ((3, 2, 2), (5, 1, 5))
FP_SIZES = ((256, 1), (256, 33), (4096, 1), (8192, 1))   # (n, batch)
FP_MAC = (2, 2, (5, 1))                                   # terms, comps, ks


def footprint_cases():
    out = []
    terms, comps, ks = FP_MAC
    for bits in (32, 64):
        for L, K, alpha in FP_SHAPES:
            for n, batch in FP_SIZES:
                up = Up(bits, n, batch, L, K, alpha)
                mac = Mac(bits, n, batch, L, K, terms, comps, ks)
                out.append(Footprint("nttmul_ksntt_modup_device", up))
                out.append(Footprint("nttmul_ksntt_modup", up, "host"))
                out.append(Footprint("nttmul_ksntt_mac_device", mac))
                out.append(Footprint("nttmul_ksntt_mac", mac, "host"))
    return out


def fp_guard_words(case):
    """The guard width tests/guarded.py gives the call: one batch entry of the widest operand."""
    from guarded import guard_words
    M = case.L + case.K
    if isinstance(case, Up):
        return guard_words(dnum(case) * M * case.n)
    return guard_words(max(case.terms, len(case.ks) * case.comps) * M * case.n)


# ---------------------------------------------------------------------------------------------
# Scale cases (tests/test_gpu_ksntt_scale.py): the rule of tests/scale_cases.py -- every launch
# holds at least MIN_WAVES = 2 * 8192 waves, with the smallest batch that meets it and a partial
# last workgroup where the kernel takes several units per workgroup
# ---------------------------------------------------------------------------------------------

SCALE_N = (4096, 8192)                       # modup
SCALE_SHAPE = (2, 1, 1)
SCALE_MAC_N = 4096
SCALE_MAC = (2, 1, (5,))                     # terms, comps, ks
WAVE, MIN_WAVES = 64, 2 * 8192


def launch_waves(case):
    """{kernel_key: waves of the launch} for one sub-batch of the whole batch."""
    rows = grid_rows(case)
    return {k: -(-units // per) * bpu(k) * rows[k] * (256 // WAVE)
            for k, (per, units, _) in units_per_block(case).items()}


def _fit(make):
    """The smallest batch at which every launch of make(batch) meets the rule."""
    def full(b):
        return all(w >= MIN_WAVES for w in launch_waves(make(b)).values())

    lo, hi = 0, 1
    while not full(hi):
        lo, hi = hi, 2 * hi
        assert hi < 1 << 24
    while hi - lo > 1:                       # the waves grow with the batch
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if full(mid) else (mid, hi)
    for b in range(hi, hi + 64):
        case = make(b)
        assert isinstance(case, Mac) or len(chunks(case)) == 1
        # (scale_cases.wants_partial: a partial last workgroup exists for some batch only where a
        # polynomial's units are no multiple of a workgroup's; at n = 4096 the mac's 16 slices are)
        if all(units % per for per, units, _ in units_per_block(case).values()
               if per > 1 and (units // b) % per):
            return b
    raise AssertionError(make(hi))


def scale_cases():
    terms, comps, ks = SCALE_MAC
    L, K, alpha = SCALE_SHAPE
    out = []
    for bits in (32, 64):
        for n in SCALE_N:
            out.append(Up(bits, n, _fit(lambda b: Up(bits, n, b, L, K, alpha)), L, K, alpha))
        n = SCALE_MAC_N
        out.append(Mac(bits, n, _fit(lambda b: Mac(bits, n, b, L, K, terms, comps, ks)), L, K,
                       terms, comps, ks))
    return out


# The output just over 4 GiB, compared with the same call in chunks below 1 GiB
LARGE_UP = (32, 4096, 1, 1, 1)               # bits, n, L, K, alpha
LARGE_MAC = (64, 65536, 1, 1, 1, 1, (5,))    # bits, n, L, K, terms, comps, ks
LARGE_BYTES = 1 << 32


def out_polys(case):
    """Limb polynomials of the output per batch entry."""
    M = case.L + case.K
    return dnum(case) * M if isinstance(case, Up) else len(case.ks) * case.comps * M


def large_cases():
    """The smallest batch whose output exceeds 4 GiB, per op."""
    out = []
    for proto in (Up(*LARGE_UP[:2], 1, *LARGE_UP[2:]), Mac(*LARGE_MAC[:2], 1, *LARGE_MAC[2:])):
        per = out_polys(proto) * proto.n * (proto.bits // 8)
        out.append(proto._replace(batch=LARGE_BYTES // per + 1))
    return out


def referenced_cases():
    """The cases whose every output word a GPU test holds to the CPU reference (tests/full_ref.py):
    all but the scale and the 4 GiB cases, whose batches exist to fill the machine."""
    out = modup_cases() + mac_cases() + mac_worst_cases() + subbatch_cases()
    out += [Up(bits, n, 2, *RANGE_SHAPE) for bits in (32, 64) for n in RANGE_N]
    n, batch, shape = VALIDATE
    out += [Up(bits, n, batch, *shape, True) for bits in (32, 64)]
    out += [Mac(bits, n, batch, *shape[:2], 2, 1, (5,), True) for bits in (32, 64)]
    out += [Up(bits, n, batch, *HOST_SHAPE) for bits in (32, 64) for n, batch in HOST]
    out += [Mac(bits, n, batch, *HOST_SHAPE[:2], 2, 2, (5, 1)) for bits in (32, 64)
            for n, batch in HOST]
    out += [f.case for f in footprint_cases()]
    return out


def all_cases():
    return referenced_cases() + scale_cases() + large_cases()


# ---------------------------------------------------------------------------------------------
# The mirror
# ---------------------------------------------------------------------------------------------

def l1_of(n):
    """ksntt.hip modup: the 2^L1 x 4096 split above n = 4096, L1 = logn - 12."""
    assert n in ALL_N and n > 4096
    return n.bit_length() - 1 - 12


def sequence(op, n, bits, comps=1):
    """ksntt.hip: the launches of one sub-batch, in order.  The class follows the word size alone.
    modup: mdntt.hip's inverse half (k_mdntt_inv; above n = 4096 k_mdntt_inv_rows and rnsmp.hip's
    k_rnsmp_cols_inv), then k_ksntt_fwd or k_ksntt_cols_fwd + k_ksntt_rows.  mac: one kernel at
    every n, its last argument the component count."""
    assert n in ALL_N, "n > 65536 is NTTMUL_EUNSUPPORTED"
    assert op in OPS
    cls, io = ("Arith32P", "u32") if bits == 32 else ("Arith64", "u64")
    if op == "mac":
        assert 1 <= comps <= MAX_COMPS
        return [f"k_ksntt_mac<{cls},{io},{comps}>"]
    if n <= 4096:
        logn = n.bit_length() - 1
        return [f"k_mdntt_inv<{cls},{io},{logn}>", f"k_ksntt_fwd<{cls},{io},{logn}>"]
    l1 = l1_of(n)
    return [f"k_mdntt_inv_rows<{cls},{io},{l1}>", f"k_rnsmp_cols_inv<{cls},{io},{l1}>",
            f"k_ksntt_cols_fwd<{cls},{io},{l1}>", f"k_ksntt_rows<{cls},{io},{l1}>"]


def kernel_name(op, n, bits, comps=1):
    """What nttmul_ksntt_kernel_name returns."""
    return " + ".join(sequence(op, n, bits, comps))


def op_of(case):
    return "modup" if isinstance(case, Up) else "mac"


def chunks(case):
    """ksntt.cpp run_modup / ksntt_plan.hpp ksntt_shape: the sub-batches of a modup.  At most
    scratch_mb MiB per scratch buffer -- y [cnt][L][n], and above n = 4096 the inverse rows' output
    of the same size -- in whole polynomials, never less than one.  The column-passed sums go
    through up_hat and bound nothing.  mac has no scratch and is one launch."""
    if isinstance(case, Mac):
        return [case.batch]
    per_poly = case.L * case.n * (case.bits // 8)
    limit = (case.scratch_mb or DEFAULT_SCRATCH_MB) << 20
    chunk = max(1, min(case.batch, limit // per_poly))
    return [min(chunk, case.batch - p) for p in range(0, case.batch, chunk)]


def kernels_of(case):
    """The kernel_keys `case` launches, in launch order: with NTTMUL_FLAG_VALIDATE the range check
    (libnttmul_rns.so's kernel: once for modup's x_hat, once each for mac's a_hat and b_hat), then
    the sequence once per sub-batch."""
    q, p = moduli_of(case)
    assert (len(q), len(p)) == (case.L, case.K)
    io = "u32" if case.bits == 32 else "u64"
    checks = [f"k_rns_check_range<{io}>"] * ((1 if isinstance(case, Up) else 2) * case.validate)
    comps = getattr(case, "comps", 1)
    return checks + sequence(op_of(case), case.n, case.bits, comps) * len(chunks(case))


def units_per_block(case):
    """{kernel_key: (units per workgroup and grid row, units of the launch per grid row, words per
    unit)} for one sub-batch of the whole batch.  modup, n <= 4096: a unit is a polynomial, a
    workgroup holds 256 / (n / 16) thread groups, each of one polynomial -- of two in k_mdntt_inv
    on 32-bit words (xform_upg).  Above: one row of 4096 per workgroup in the row kernels, 256
    columns of one polynomial per workgroup in the column kernels (16 workgroups per unit).  mac: a
    unit is a slice of 256 slots, MAC_SLICES per workgroup, n / 256 per polynomial."""
    if isinstance(case, Mac):
        (key,) = sequence("mac", case.n, case.bits, case.comps)
        return {key: (MAC_SLICES, case.batch * (case.n // 256), 256)}
    seq = sequence("modup", case.n, case.bits)
    if case.n <= 4096:
        pb = 256 // (case.n // 16)
        return {seq[0]: (pb * (2 if case.bits == 32 else 1), case.batch, case.n),
                seq[1]: (pb, case.batch, case.n)}
    l1 = l1_of(case.n)
    return {seq[0]: (1, case.batch << l1, 4096), seq[1]: (1, case.batch, case.n),
            seq[2]: (1, case.batch, case.n), seq[3]: (1, case.batch << l1, 4096)}


def grid_rows(case):
    """{kernel_key: grid rows the launch covers}: L for the inverse's kernels (gridDim.y), the
    dnum (L + K) targets for the forward's (fastest in a one-dimensional grid), for the mac its
    L + K limbs (gridDim.y) times the rotations (fastest in gridDim.x)."""
    if isinstance(case, Mac):
        (key,) = sequence("mac", case.n, case.bits, case.comps)
        return {key: (case.L + case.K) * len(case.ks)}
    seq = sequence("modup", case.n, case.bits)
    inv = seq[:1] if case.n <= 4096 else seq[:2]
    return {k: case.L if k in inv else dnum(case) * (case.L + case.K) for k in seq}


def bpu(key):
    """Workgroups per unit: the column kernels spread a polynomial over 4096 / 256 = 16."""
    return 16 if "_cols_" in key else 1


def transforms(L, K, alpha, rots):
    """(new, old) transforms per input of the NTT-domain key switch with `rots` rotations of two
    components: modup -> mac -> mdntt_moddown against inverse, ks_modup, forward, hoist_ntt,
    ks_moddown, forward."""
    dn, M = -(-L // alpha), L + K
    return dn * M + 2 * rots * M, L + dn * M + 2 * rots * M + 2 * rots * L


def launches(n, old=False):
    """Launches of the chain: 2 + 1 + 2 (4 + 1 + 4 above n = 4096) against 6 (10)."""
    if old:
        return 6 if n <= 4096 else 10
    return 5 if n <= 4096 else 9


# Kernels of libnttmul_ksntt.so beyond libnttmul_mdntt.so's that no call can launch: (regular
# expression over the kernel_key, reason).  None: ksntt.hip instantiates only what dispatch reaches.
UNREACHABLE = ()
