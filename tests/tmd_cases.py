"""Case tables of tests/test_gpu_tmd.py, test_gpu_tmd_bases.py, test_gpu_tmd_footprint.py and
test_gpu_tmd_scale.py, and a pure-Python mirror of the dispatch behind include/nttmul_tmd.h
(csrc/tmd.hip dispatch, csrc/tmd.cpp run, csrc/tmd_plan.hpp tmd_shape): plain data and arithmetic,
no GPU.  Built from tests/mdntt_cases.py's constants: the two libraries share their shapes, their
scratch and their sub-batch rule.

tests/test_tmd_ledger.py holds the mirror against the cross-compiled lib/libnttmul_tmd.so (the
kernels it holds beyond libnttmul_ctlin.so's are exactly the ones the mirror names over these
cases); test_gpu_tmd.py::test_mirror_agrees_with_the_library_dispatch anchors it on the GPU to the
library's own dry run (nttmul_tmd_kernel_name).

The conversion sum holds K + 1 products, the correction last, and folds every CADENCE of them:
SHAPES puts K + 1 = 2, 3, 4 and 6 on both sides of both cadences (2 and 4)."""
from collections import namedtuple

import mdntt_cases as MC

CADENCE = MC.CADENCE
ALL_N = MC.ALL_N
DEFAULT_SCRATCH_MB = MC.DEFAULT_SCRATCH_MB
T_BOUND = {32: 1 << 31, 64: 1 << 62}          # csrc/tmd_plan.hpp tmd_t_bound


def plain_moduli(bits):
    """3, 65537 and the largest odd t below the class bound."""
    return (3, 65537, T_BOUND[bits] - 1)


Case = namedtuple("Case", "bits n batch L K t validate scratch_mb moduli",
                  defaults=(False, 0, None))

REF_N = (256, 512)                            # every coefficient in Python integers
REF_BATCH = 3                                 # a workgroup ends partial
SHAPES = ((1, 1), (3, 1), (4, 2), (3, 3), (2, 5))
IDENTITY_N = (256, 1024, 4096, 8192, 65536)   # every kernel size: L1 = 1 and 4 above 4096
IDENTITY_BATCH = 2
IDENTITY_SHAPE = (3, 2)
DEGREE_N = (2048, 16384, 32768)               # the degrees between: every kernel has a case
# (bits, n, L, K, batch, sub-batches) with scratch_mb = 1: per polynomial the larger scratch
# buffer is L n words, 96 KiB and 192 KiB
SUBBATCH = ((32, 8192, 3, 2, 23, (10, 10, 3)), (64, 8192, 3, 2, 12, (5, 5, 2)))
EDGE_N = (256, 8192)
EDGE_K = (1, 2, 5)
EDGE_L = 2
VALIDATE = MC.VALIDATE
CHAIN_N = (256, 8192)
CHAIN_T = (3, 65537)
E2E_N, E2E_T = 256, 65537


def md_case(case):
    return MC.Case(case.bits, case.n, case.batch, case.L, case.K, case.validate, case.scratch_mb,
                   None)


def moduli_of(case):
    """(q, p) of a case: ks_ref.bases of its class, or the profile of tests/basis_cases.py its
    `moduli` names."""
    if case.moduli is not None:
        import basis_cases as BC
        return BC.basis(case.moduli, case.L, case.K)
    return MC.moduli_of(md_case(case))


def parity_cases():
    return [Case(bits, n, REF_BATCH, L, K, t) for bits in (32, 64) for n in REF_N
            for L, K in SHAPES for t in plain_moduli(bits)]


def identity_cases():
    return [Case(bits, n, IDENTITY_BATCH, *IDENTITY_SHAPE, t) for bits in (32, 64)
            for n in IDENTITY_N for t in plain_moduli(bits)]


def degree_cases():
    """The identity at the degrees IDENTITY_N and REF_N leave out, at t = 65537."""
    return [Case(bits, n, IDENTITY_BATCH, *IDENTITY_SHAPE, 65537) for bits in (32, 64)
            for n in DEGREE_N]


def subbatch_cases():
    return [Case(bits, n, batch, L, K, 65537, False, 1) for bits, n, L, K, batch, _ in SUBBATCH]


Footprint = namedtuple("Footprint", "entry case host", defaults=("",))
FP_SHAPES = MC.FP_SHAPES
FP_SIZES = MC.FP_SIZES


def footprint_cases():
    out = []
    for bits in (32, 64):
        for shape in FP_SHAPES:
            for n, batch in FP_SIZES:
                case = Case(bits, n, batch, *shape, 65537)
                out.append(Footprint("nttmul_tmd_moddown_device", case))
                out.append(Footprint("nttmul_tmd_moddown", case, "host"))
    return out


def fp_guard_words(case):
    """The guard width tests/guarded.py gives the call: one batch entry of x_hat, (L + K) n."""
    from guarded import guard_words
    return guard_words((case.L + case.K) * case.n)


# Scale cases (tests/test_gpu_tmd_scale.py): the rule of tests/scale_cases.py on one case per new
# kernel template and word class
SCALE_N = MC.SCALE_N
SCALE_SHAPE = MC.SCALE_SHAPE
WAVE, MIN_WAVES = MC.WAVE, MC.MIN_WAVES


def launch_waves(case):
    rows = grid_rows(case)
    return {k: -(-units // per) * bpu(k) * rows[k] * (256 // WAVE)
            for k, (per, units, _) in units_per_block(case).items()}


def scale_cases():
    """mdntt_cases' batches: the launches have the same shapes under this library's names."""
    L, K = SCALE_SHAPE
    return [Case(bits, n, MC.scale_batch(bits, n), L, K, 65537) for bits in (32, 64)
            for n in SCALE_N]


# Mixed-size bases (tests/test_gpu_tmd_bases.py, tests/basis_cases.py)
BASES_N = (256, 8192)
BASES_PROFILES = ("chain64", "chain64_rev", "chain32", "chain32_rev")
BASES_SHAPES = ((4, 2), (3, 2))
BASES_BATCH = 2
BASES_T = (3, 65537)


def bases_cases():
    import basis_cases as BC
    return [Case(BC.bits_of(prof), n, BASES_BATCH, L, K, t, False, 0, prof)
            for prof in BASES_PROFILES for n in BASES_N for L, K in BASES_SHAPES for t in BASES_T]


def referenced_cases():
    """The cases whose every output word a GPU test holds to the CPU reference (tests/full_ref.py):
    all but the scale and the 4 GiB cases, whose batches exist to fill the machine."""
    out = parity_cases() + identity_cases() + degree_cases() + subbatch_cases()
    out += [Case(bits, n, 1, EDGE_L, K, t) for bits in (32, 64) for n in EDGE_N for K in EDGE_K
            for t in plain_moduli(bits)]
    n, batch, shape = VALIDATE
    out += [Case(bits, n, batch, *shape, 65537, True) for bits in (32, 64)]
    out += [f.case for f in footprint_cases()]
    out += bases_cases()
    return out


def all_cases():
    return referenced_cases() + scale_cases()


# ---------------------------------------------------------------------------------------------
# Seeded inputs
# ---------------------------------------------------------------------------------------------

def seed_of(case):
    return 1000 * case.L + 10 * case.K + case.n + 7 * case.batch + case.t % 1009 + case.bits


def seeded_input(case, seed=None):
    """Seeded canonical words in NTT order, [batch, L + K, n] over Q u P (any canonical vector is
    a transform of something)."""
    import numpy as np
    import bconv_ref as B
    q, p = moduli_of(case)
    rng = np.random.default_rng(seed_of(case) if seed is None else seed)
    return B.random_words(rng, q + p, case.batch, case.n,
                          np.uint32 if case.bits == 32 else np.uint64)


def bases_input(case):
    """seeded_input with the ends of every limb's range in the first two words."""
    x = seeded_input(case)
    q, p = moduli_of(case)
    for l, m in enumerate(q + p):
        x[0, l, :2] = (0, m - 1)
    return x


def chain_error_polys(ch, out):
    """e = c_0 + c_1 s - sigma_k(x) sigma_k(s2), centred modulo Q, per (batch entry, rotation) of
    hoist_ref.chain's data and an output [batch, rots, 2, L, n]: a list of lists of n signed
    Python integers."""
    from math import prod
    import numpy as np
    import galois_ref
    import ks_ref
    from hoist_ref import rotate_signed
    from xconv_ref import _crt
    q = ch["q"]
    Q = prod(q)
    es = []
    for b in range(out.shape[0]):
        for r, k in enumerate(ch["ks"]):
            xr = galois_ref.coeff(ch["x"][b:b + 1], k, q)[0]
            s2 = rotate_signed(ch["s2"], k)
            limbs = [(np.asarray(out[b, r, 0, i]).astype(object)
                      + ks_ref.negacyclic(ch["s"], out[b, r, 1, i], m)
                      - ks_ref.negacyclic(s2, xr[i], m)) % m for i, m in enumerate(q)]
            e = _crt(np.stack(limbs)[None], q)[0]
            es.append([int(v) - Q if int(v) > Q // 2 else int(v) for v in e])
    return es


# ---------------------------------------------------------------------------------------------
# The mirror
# ---------------------------------------------------------------------------------------------

def l1_of(n):
    return MC.l1_of(n)


def sequence(n, bits):
    """tmd.hip dispatch: the launches of one sub-batch, in order.  The inverse half is mdntt.hip's
    (and above n = 4096 rnsmp.hip's column pass); the forward half is k_tmd_fwd up to n = 4096,
    k_tmd_cols_fwd followed by mdntt.hip's k_mdntt_rows above."""
    assert n in ALL_N, "n > 65536 is NTTMUL_EUNSUPPORTED"
    cls, io = ("Arith32P", "u32") if bits == 32 else ("Arith64", "u64")
    if n <= 4096:
        logn = n.bit_length() - 1
        return [f"k_mdntt_inv<{cls},{io},{logn}>", f"k_tmd_fwd<{cls},{io},{logn}>"]
    l1 = l1_of(n)
    return [f"k_mdntt_inv_rows<{cls},{io},{l1}>", f"k_rnsmp_cols_inv<{cls},{io},{l1}>",
            f"k_tmd_cols_fwd<{cls},{io},{l1}>", f"k_mdntt_rows<{cls},{io},{l1}>"]


def kernel_name(n, bits):
    """What nttmul_tmd_kernel_name returns."""
    return " + ".join(sequence(n, bits))


def chunks(case):
    """tmd.cpp run / tmd_plan.hpp tmd_shape: mdntt's sub-batches."""
    return MC.chunks(md_case(case))


def kernels_of(case):
    """The kernel_keys `case` launches, in launch order."""
    io = "u32" if case.bits == 32 else "u64"
    return ([f"k_rns_check_range<{io}>"] if case.validate else []) + \
        sequence(case.n, case.bits) * len(chunks(case))


def units_per_block(case):
    """mdntt_cases.units_per_block under this library's kernel names."""
    seq = sequence(case.n, case.bits)
    md = MC.units_per_block(md_case(case))
    return dict(zip(seq, (md[k] for k in MC.sequence(case.n, case.bits))))


def grid_rows(case):
    """{kernel_key: limbs the launch covers}: K for the inverse's kernels, L for the forward's."""
    seq = sequence(case.n, case.bits)
    inv = seq[:1] if case.n <= 4096 else seq[:2]
    return {k: case.K if k in inv else case.L for k in seq}


bpu = MC.bpu

# Kernels of libnttmul_tmd.so beyond libnttmul_ctlin.so's that no case launches: {kernel_key:
# reason}.  None: tmd.hip instantiates only what dispatch reaches, and parity_cases, identity_cases
# and degree_cases between them reach every degree.
EXEMPT = {}


# ---------------------------------------------------------------------------------------------
# The code object's metadata (the AMDGPU note of each gfx950 ELF: a MessagePack map)
# ---------------------------------------------------------------------------------------------

def _unpack(b, i):
    """One MessagePack value of b at i: (value, next position).  The forms the metadata uses."""
    import struct
    c = b[i]
    if c < 0x80:
        return c, i + 1
    if c >= 0xe0:
        return c - 256, i + 1
    if 0x80 <= c <= 0x8f or c in (0xde, 0xdf):
        if c == 0xde:
            n, i = struct.unpack_from(">H", b, i + 1)[0], i + 3
        elif c == 0xdf:
            n, i = struct.unpack_from(">I", b, i + 1)[0], i + 5
        else:
            n, i = c & 15, i + 1
        out = {}
        for _ in range(n):
            k, i = _unpack(b, i)
            out[k], i = _unpack(b, i)
        return out, i
    if 0x90 <= c <= 0x9f or c in (0xdc, 0xdd):
        if c == 0xdc:
            n, i = struct.unpack_from(">H", b, i + 1)[0], i + 3
        elif c == 0xdd:
            n, i = struct.unpack_from(">I", b, i + 1)[0], i + 5
        else:
            n, i = c & 15, i + 1
        out = []
        for _ in range(n):
            v, i = _unpack(b, i)
            out.append(v)
        return out, i
    if 0xa0 <= c <= 0xbf:
        n = c & 31
        return b[i + 1:i + 1 + n].decode(), i + 1 + n
    if c in (0xd9, 0xda, 0xdb, 0xc4, 0xc5, 0xc6):
        w = {0xd9: 1, 0xda: 2, 0xdb: 4, 0xc4: 1, 0xc5: 2, 0xc6: 4}[c]
        n = int.from_bytes(b[i + 1:i + 1 + w], "big")
        raw = b[i + 1 + w:i + 1 + w + n]
        return (raw.decode() if c >= 0xd9 else raw), i + 1 + w + n
    if c == 0xc0:
        return None, i + 1
    if c in (0xc2, 0xc3):
        return c == 0xc3, i + 1
    if c in (0xcc, 0xcd, 0xce, 0xcf):
        w = 1 << (c - 0xcc)
        return int.from_bytes(b[i + 1:i + 1 + w], "big"), i + 1 + w
    if c in (0xd0, 0xd1, 0xd2, 0xd3):
        w = 1 << (c - 0xd0)
        return int.from_bytes(b[i + 1:i + 1 + w], "big", signed=True), i + 1 + w
    if c in (0xca, 0xcb):
        w = 4 if c == 0xca else 8
        return struct.unpack_from(">f" if w == 4 else ">d", b, i + 1)[0], i + 1 + w
    raise ValueError(f"MessagePack form {c:#x} at {i}")


def kernel_metadata(path):
    """{kernel_key: the kernel's metadata map (".vgpr_count", ".private_segment_fixed_size",
    ...)} of every kernel in the gfx950 code objects of the library at `path`."""
    import struct
    import nttmul
    out = {}
    for co in nttmul._amdgcn_elfs(path):
        note = nttmul._elf_sections(co).get(".note", b"")
        i = 0
        while i + 12 <= len(note):
            namesz, descsz, typ = struct.unpack_from("<III", note, i)
            name = note[i + 12:i + 12 + namesz]
            d0 = i + 12 + (namesz + 3) // 4 * 4
            if typ == 32 and name.rstrip(b"\0") == b"AMDGPU":
                meta, _ = _unpack(note[d0:d0 + descsz], 0)
                for k in meta.get("amdhsa.kernels", []):
                    out[nttmul.kernel_key(k[".name"])] = k
            i = d0 + (descsz + 3) // 4 * 4
    return out
