"""Scale cases: rows of the existing case tables whose every launch fills the GPU twice over, the
rule they are held to, and the sample rule of tests/test_gpu_scale.py.  Plain data and arithmetic
(no GPU, no library, no oracle); tests/test_scale_ledger.py holds all of it.

The rule is derived, not measured.  A compute unit holds at most CU_WAVES = 32 waves (8 per SIMD)
and dispatch_cases.MI355X_CUS is 256; registers and LDS can only lower that, so RESIDENT_WAVES =
256 * 32 = 8192 bounds what is resident at once.  Nobody has measured the real residency of these
kernels.  Every launch of a scale case

* holds at least MIN_WAVES = 2 * RESIDENT_WAVES waves, so at least half of its workgroups start in
  a slot another workgroup has left, several workgroups share a compute unit, its LDS and its
  SIMDs, and the L2 of every XCD is contended for;
* ends in a partial last workgroup where the kernel takes several units per workgroup and a batch
  exists that leaves one: dispatch_cases.FP_ALWAYS_WHOLE does not list the kernel, and the units
  of one polynomial are no multiple of the units of a workgroup.

Workgroups, units per workgroup and units of a launch are the case modules' own units_per_block;
what those tuples do not carry is restated here once: the threads of a workgroup (block_threads),
the second grid dimension (limbs or digits), and the workgroups per unit of the kernels that
spread one unit over several (`bpu`).  A sub-batched row (scratch_mb lowered) must meet the wave
rule in every sub-batch but the ragged last.

The batch of a row is not written down: fit() takes the smallest batch that meets the rule, so
a row follows the mirrors when a kernel's workgroup shape changes."""
import functools
import re
from collections import namedtuple

import bconv_cases as B
import dispatch_cases as D
import galois_cases as G
import hoist_cases as H
import ks_cases as K
import mac_cases as MC
import macn_cases as N
import rns_cases as R
import rnsmp_cases as M

WAVE = 64
CU_WAVES = 32                                # 8 waves on each of the four SIMDs
RESIDENT_WAVES = D.MI355X_CUS * CU_WAVES     # 8192: an upper bound on the waves resident at once
MIN_WAVES = 2 * RESIDENT_WAVES

# family: the case module of the row; alias: "" or "out=in" (a transform in place); sub: the row
# runs in sub-batches (its case carries the lowered scratch_mb; for "plain", `sub` is that value)
Scale = namedtuple("Scale", "family case alias sub", defaults=("", 0))

# One launch.  per / units: units per workgroup and units of the launch in one grid row, as
# units_per_block gives them; rows: the second grid dimension; bpu: workgroups per unit group
# (16 for the limb-aware column passes, the rotations for k_rns_hoist); upp / unit0: unit u of the
# launch belongs to polynomial (unit0 + u) // upp of the call's batch.
Launch = namedtuple("Launch", "key per units rows threads bpu upp unit0")


def block_threads(key, n):
    """Threads of a workgroup: rows_threads(10) = 64 for the fused products at n = 1024
    (csrc/kernels_dev.hpp, csrc/rns.hip rows), a thread per four staged words up to 1024 for the
    coefficient-order automorphism (csrc/galois.hip coeff), 256 everywhere else."""
    if re.fullmatch(r"k_rows<\w+,u\d+,u\d+,10,0,\w+>|k_rns_rows<\w+,u\d+,10>", key):
        return 64
    m = re.fullmatch(r"k_galois_coeff<u\d+,(\d)>", key)
    if m:
        return min(1024, max(n >> int(m[1]), G.STAGE_WORDS) // 4)
    return 256


def blocks_x(l):
    return -(-l.units // l.per) * l.bpu


def waves(l):
    return blocks_x(l) * l.rows * (l.threads // WAVE)


def always_whole(key):
    return any(re.fullmatch(p, key) for p, _ in D.FP_ALWAYS_WHOLE)


def wants_partial(l):
    """The kernel takes several units per workgroup and some batch leaves a partial last one."""
    return l.per > 1 and not always_whole(l.key) and l.upp % l.per != 0


def block_polys(l, x):
    """The polynomials of the call's batch workgroup blockIdx.x = x of the launch works on."""
    u0 = x // l.bpu * l.per
    u1 = min(l.units, u0 + l.per) - 1
    return range((l.unit0 + u0) // l.upp, (l.unit0 + u1) // l.upp + 1)


def second_wave_block(l):
    """blockIdx.x of the first workgroup past RESIDENT_WAVES waves in launch order (x fastest),
    or None when the launch is smaller."""
    g = -(-RESIDENT_WAVES // (l.threads // WAVE))
    bx = blocks_x(l)
    return g % bx if g < bx * l.rows else None


def _mk(key, tup, n, polys, rows=1, bpu=1, upp=None, unit0=0):
    per, units, _ = tup
    return Launch(key, per, units, rows, block_threads(key, n), bpu,
                  upp if upp is not None else units // polys, unit0)


# ---------------------------------------------------------------------------------------------
# The launches of a row, family by family, from the modules' units_per_block
# ---------------------------------------------------------------------------------------------

def _plain(s):
    c, out, p = s.case, [], 0
    for cnt in D.chunks(c, s.sub):
        for key, tup in D.units_per_block(c._replace(batch=cnt)).items():
            l = _mk(key, tup, c.n, cnt)
            out.append(l._replace(unit0=p * l.upp))
        p += cnt
    return out


def _mac(s):
    c = s.case
    return [_mk(k, t, c.n, c.batch) for k, t in MC.units_per_block(c).items()]


def _rns(s):
    c = s.case
    return [_mk(k, t, c.n, c.batch, rows=len(c.moduli)) for k, t in R.units_per_block(c).items()]


def _mp_cols(key):
    """The limb-aware column passes spread a polynomial over 4096 / 256 = 16 workgroups
    (rnsmp_cases.units_per_block, csrc/rnsmp.hip cols_fwd / cols_inv)."""
    return 16 if key.startswith("k_rnsmp_cols") else 1


def _rnsmp(s):
    c, out, p = s.case, [], 0
    for cnt in M.chunks(c):
        for key, tup in M.units_per_block(c._replace(batch=cnt)).items():
            l = _mk(key, tup, c.n, cnt, rows=len(c.moduli), bpu=_mp_cols(key))
            out.append(l._replace(unit0=p * l.upp))
        p += cnt
    return out


def _mp_pass(which, n, moduli, units, polys, rows):
    """One column pass of a multi-pass mac over `units` polynomials: rnsmp_cases' own tuple."""
    (key, tup), = [(k, t) for k, t in M.units_per_block(M.Case("mac", n, moduli, units)).items()
                   if k.startswith(which)]
    return _mk(key, tup, n, polys, rows=rows, bpu=_mp_cols(key))


def _macn(s):
    c, L = s.case, len(s.case.moduli)
    if N.family(c.n) == "rns":
        return [_mk(k, t, c.n, c.batch, rows=L) for k, t in N.units_per_block(c).items()]
    out, p = [], 0
    for cnt in N.chunks(c):
        ls = [_mp_pass("k_rnsmp_cols_fwd", c.n, c.moduli, cnt * c.terms, cnt, L)]
        ls += [_mk(k, t, c.n, cnt, rows=L)
               for k, t in N.units_per_block(c._replace(batch=cnt)).items()]
        ls.append(_mp_pass("k_rnsmp_cols_inv", c.n, c.moduli, cnt * c.comps, cnt, L))
        out += [l._replace(unit0=p * l.upp) for l in ls]
        p += cnt
    return out


def _hoist(s):
    c, L, rots = s.case, len(s.case.moduli), len(s.case.ks)
    if H.family(c.n) == "rns":
        return [_mk(k, t, c.n, c.batch, rows=L, bpu=rots) for k, t in H.units_per_block(c).items()]
    # sub-batches of output units (p, r); a unit of the row kernel is one row of one output unit,
    # a unit of the column pass one of its comps polynomials
    l1, out, u0 = M.l1_of(c.n), [], 0
    (key, _), = H.units_per_block(c).items()
    for cnt in H.chunks(c):
        out.append(Launch(key, 1, cnt << l1, L, block_threads(key, c.n), 1, rots << l1, u0 << l1))
        inv = _mp_pass("k_rnsmp_cols_inv", c.n, c.moduli, cnt * c.comps, 1, L)
        out.append(inv._replace(upp=rots * c.comps, unit0=u0 * c.comps))
        u0 += cnt
    return out


def _bconv(s):
    c = s.case
    return [_mk(k, t, c.n, c.batch) for k, t in B.units_per_block(c).items()]


def _galois(s):
    # (above one residue class the sibling workgroups of a polynomial are interleaved in groups
    # of eight polynomials, csrc/galois.hip coeff: block_polys is exact to within such a group)
    c = s.case
    return [_mk(k, t, c.n, c.batch, rows=len(c.moduli)) for k, t in G.units_per_block(c).items()]


def _ks(s):
    c = s.case
    rows = K.dnum(c) if c.op == "modup" else 1
    return [_mk(k, t, c.n, c.batch, rows=rows) for k, t in K.units_per_block(c).items()]


FAMILIES = {"plain": (D, _plain), "mac": (MC, _mac), "rns": (R, _rns), "rnsmp": (M, _rnsmp),
            "macn": (N, _macn), "hoist": (H, _hoist), "bconv": (B, _bconv), "galois": (G, _galois),
            "ks": (K, _ks)}


def launches(s):
    """Every kernel launch of a row, in launch order, sub-batch by sub-batch."""
    return FAMILIES[s.family][1](s)


def kernels_of(s):
    """The mirror's kernel_keys of the row (dispatch_cases names one sub-batch of a plain call)."""
    keys = FAMILIES[s.family][0].kernels_of(s.case)
    return keys * len(D.chunks(s.case, s.sub)) if s.family == "plain" else keys


def batch_of(s):
    return s.case.batch


def sub_batches(s):
    """The polynomial counts (output units for hoist) of the row's sub-batches."""
    c = s.case
    if s.family == "plain":
        return D.chunks(c, s.sub)
    if s.family in ("rnsmp", "macn", "hoist"):
        return FAMILIES[s.family][0].chunks(c)
    return [c.batch]


def last_sub_batch_launches(s):
    """How many launches at the end of launches(s) belong to the ragged last sub-batch."""
    subs = sub_batches(s)
    return len(launches(s)) // len(subs) if s.sub and len(subs) > 1 else 0


def violations(s, mirror=True):
    """What the rule finds wrong with a row: a list of strings, empty when it meets the rule.
    mirror: also hold the launches to the module's kernels_of (ks_cases' looks its primes up,
    which loads lib/libnttmul.so: not while a GPU test module is collected)."""
    out, ls = [], launches(s)
    keys = kernels_of(s) if mirror else [l.key for l in ls]
    if [l.key for l in ls] != keys:
        out.append(f"launches {[l.key for l in ls]} are not the mirror's {keys}")
    held = ls[:len(ls) - last_sub_batch_launches(s)]
    for l in held:
        if waves(l) < MIN_WAVES:
            out.append(f"{l.key}: {waves(l)} waves < {MIN_WAVES}")
    for l in (held if s.sub else ls):
        if wants_partial(l) and l.units % l.per == 0:
            out.append(f"{l.key}: {l.units} units end in a whole workgroup of {l.per}")
    if s.sub and len(sub_batches(s)) < 3:
        out.append(f"{len(sub_batches(s))} sub-batches, fewer than three")
    return out


def fit(make, family, alias="", sub=0):
    """The smallest batch whose row make(batch) meets the rule (make: batch -> case)."""
    def bad(b):
        return violations(Scale(family, make(b), alias, sub), mirror=False)
    lo, hi = 0, 1
    # (steps of a tenth: past the default scratch a call splits, and its ragged last sub-batch
    # falls below the rule again)
    while any("waves" in v for v in bad(hi)):
        lo, hi = hi, hi + max(1, hi // 10)
        assert hi < 1 << 24
    while hi - lo > 1:                       # within one sub-batch the waves grow with the batch
        mid = (lo + hi) // 2
        if any("waves" in v for v in bad(mid)):
            lo = mid
        else:
            hi = mid
    for b in range(hi, hi + 64):
        if not bad(b):
            return b
    raise AssertionError(f"no batch from {hi} meets the rule: {bad(hi)}")


# ---------------------------------------------------------------------------------------------
# The sample rule of tests/test_gpu_scale.py
# ---------------------------------------------------------------------------------------------

SAMPLE_LEAST = 256
SAMPLE_STRIDES = 64


def sample(ls, batch):
    """The polynomials a sampled comparison always holds, sorted: polynomial 0, the last one,
    every polynomial of a partial last workgroup, the first workgroup past RESIDENT_WAVES waves of
    every launch, one from each 1 / 64 of the batch; at least 256, or all of a smaller batch."""
    if batch <= SAMPLE_LEAST:
        return list(range(batch))
    out = {0, batch - 1}
    out.update(i * batch // SAMPLE_STRIDES for i in range(SAMPLE_STRIDES))
    for l in ls:
        if l.units % l.per:
            out.update(block_polys(l, blocks_x(l) - 1))
        x = second_wave_block(l)
        if x is not None:
            out.update(block_polys(l, x))
    out = {p for p in out if 0 <= p < batch}
    i = 0
    while len(out) < SAMPLE_LEAST:           # top up, evenly spread
        out.add((i * batch // SAMPLE_LEAST + i % 7) % batch)
        i += 1
    return sorted(out)


def mismatching(got, want, polys):
    """The entries of `polys` at which got[i] != want[i] (array-likes indexed by the position in
    the sample, one entry per polynomial)."""
    return [p for i, p in enumerate(polys) if not (got[i] == want[i]).all()]


# ---------------------------------------------------------------------------------------------
# The tables
# ---------------------------------------------------------------------------------------------

# both word classes: a 32-bit Plantard modulus on 32-bit words, a 62-bit one on 64-bit words
PLAIN_CLASSES = ((D.Q31, 32), (D.Q62, 64))
# the ends of the two template ranges, and n = 1024, where k_rows and k_xform change shape; on
# 64-bit arithmetic n = 65536 is the square split, so 32768 is the upper end of the 2^L1 x 4096 one
PLAIN_N = {32: (256, 1024, 4096, 8192, 65536), 64: (256, 1024, 4096, 8192, 32768, 65536)}
PLAIN_REORDER_N = (4096, 8192)               # mode 2: k_bitrev and k_bitrev_inplace
PLAIN_SUB = (8192, D.Q31, 32)                # a product in three sub-batches
FUSED_N = (256, 4096)
MULTIPASS_N = (8192, 65536)
TERMS, COMPS, ROTS = 3, 2, 3
BCONV_SHAPE = (4, 5)                         # crosses the fold cadence, leaves a padded tile
KS_SHAPE = (4, 2, 2)
GALOIS_COUNT = 4
# coeff: one and several polynomials per workgroup, 1024 threads, and the n at which a polynomial
# is staged in two (32-bit at 65536, 64-bit at 32768) and four (64-bit at 65536) residue classes
GALOIS_COEFF_N = {32: (256, 4096, 65536), 64: (256, 4096, 32768, 65536)}
GALOIS_NTT_N = (256, 65536)


def plain_ops(n, q, w):
    """(case maker, alias) of one chain of the plain library: the fill, the product, forward and
    inverse (both also in place) and the pointwise product."""
    xf = lambda mode: (lambda b: D.Case("transform", n, q, w, b, mode=mode))   # noqa: E731
    return [(lambda b: D.Case("fill", n, q, w, b), ""),
            (lambda b: D.Case("multiply", n, q, w, b), ""),
            (xf(0), ""), (xf(0), "out=in"), (xf(3), ""), (xf(3), "out=in"),
            (lambda b: D.Case("pointwise", n, q, w, b), "")]


def plain_batch(n, q, w):
    """One batch for the whole chain: the smallest at which every operation meets the rule."""
    ops = plain_ops(n, q, w)
    b = max(fit(make, "plain", alias) for make, alias in ops)
    for b in range(b, b + 64):
        if not any(violations(Scale("plain", make(b), alias), False) for make, alias in ops):
            return b
    raise AssertionError((n, q, w))


def _sub_row(family, make, poly_bytes):
    """(scratch_mb, polynomials per sub-batch) of a row in three sub-batches: the fewest MiB whose
    sub-batch meets the wave rule on its own (make: batch, scratch_mb -> case; poly_bytes: what
    the family's sub-batch rule charges per polynomial).  The row's batch is two such sub-batches
    and one polynomial more."""
    one = fit(lambda b: make(b, 0), family)
    mb = -(-one * poly_bytes >> 20)
    chunk = (mb << 20) // poly_bytes
    return mb, chunk


@functools.lru_cache(maxsize=None)
def scale_cases():
    out = []
    S = Scale
    # libnttmul.so
    for q, w in PLAIN_CLASSES:
        for n in PLAIN_N[w]:
            b = plain_batch(n, q, w)
            out += [S("plain", make(b), alias) for make, alias in plain_ops(n, q, w)]
        for n in PLAIN_REORDER_N:
            make = lambda b: D.Case("transform", n, q, w, b, mode=2)             # noqa: E731
            b = fit(make, "plain")
            out += [S("plain", make(b)), S("plain", make(b), "out=in")]
    n, q, w = PLAIN_SUB
    mb, chunk = _sub_row("plain", lambda b, mb: D.Case("multiply", n, q, w, b),
                         n * (D.native_bits(q) // 8))
    out.append(S("plain", D.Case("multiply", n, q, w, 2 * chunk + 1), "", mb))
    # libnttmul_mac.so
    for n in FUSED_N:
        for q, w in ((MC.PLANTARD_AT[n], 32), (D.Q62, 64)):
            for shared in (False, True):
                make = lambda b: MC.Case(n, q, w, TERMS, shared, b)             # noqa: E731
                out.append(S("mac", make(fit(make, "mac"))))
    # rns / rnsmp, L = 3
    for fam, T, ns in (("rns", R, FUSED_N), ("rnsmp", M, MULTIPASS_N)):
        for n in ns:
            for basis in T.BASES:
                for op in T.OPS:
                    make = lambda b: T.Case(op, n, basis, b, TERMS if op == "mac" else 1)  # noqa: E731
                    out.append(S(fam, make(fit(make, fam))))
    # macn and hoist over both families
    for n in FUSED_N + MULTIPASS_N:
        for basis in N.cases_of(n).BASES:
            make = lambda b: N.Case(n, basis, b, TERMS, COMPS, True)            # noqa: E731
            out.append(S("macn", make(fit(make, "macn"))))
            ks = H.draw(n, ROTS, 1)
            make = lambda b: H.Case(n, basis, b, TERMS, COMPS, ks)              # noqa: E731
            out.append(S("hoist", make(fit(make, "hoist"))))
    # one multi-pass row per limb-aware family in three sub-batches
    n, basis = 8192, M.BASIS32
    poly = len(basis) * n * 4
    make = lambda b, mb: M.Case("multiply", n, basis, b, scratch_mb=mb)          # noqa: E731
    mb, chunk = _sub_row("rnsmp", make, poly)
    out.append(S("rnsmp", make(2 * chunk + 1, mb), "", mb))
    make = lambda b, mb: N.Case(n, basis, b, TERMS, COMPS, True, False, mb)      # noqa: E731
    mb, chunk = _sub_row("macn", make, poly * max(TERMS, COMPS))
    out.append(S("macn", make(2 * chunk + 1, mb), "", mb))
    ks = H.draw(n, ROTS, 1)
    make = lambda b, mb: H.Case(n, basis, b, TERMS, COMPS, ks, False, mb)        # noqa: E731
    one = fit(lambda b: make(b, 0), "hoist")
    mb = -(-one * ROTS * COMPS * poly >> 20)
    chunk = (mb << 20) // (COMPS * poly)      # output units per sub-batch
    out.append(S("hoist", make(-(-(2 * chunk + 1) // ROTS), mb), "", mb))
    # bconv
    L, Kp = BCONV_SHAPE
    for bits in (32, 64):
        for n in FUSED_N:
            for op in B.OPS:
                make = lambda b: B.Case(op, bits, n, b, L, Kp)                  # noqa: E731
                out.append(S("bconv", make(fit(make, "bconv"))))
    # galois
    for basis in G.BASES:
        bits = G.word_bits(basis)
        for n in GALOIS_COEFF_N[bits]:
            make = lambda b: G.Case("coeff", n, basis, b, (G.ref.element(n, 1),))   # noqa: E731
            out.append(S("galois", make(fit(make, "galois"))))
        for n in GALOIS_NTT_N:
            make = lambda b: G.Case("ntt", n, basis, b, (G.ref.element(n, 1),))  # noqa: E731
            out.append(S("galois", make(fit(make, "galois"))))
            make = lambda b: G.Case("ntt_many", n, basis, b, G.many_ks(n, GALOIS_COUNT))  # noqa: E731
            out.append(S("galois", make(fit(make, "galois"))))
    # ks
    for bits in (32, 64):
        for n in (256, 65536):
            for op in K.OPS:
                make = lambda b: K.Case(op, bits, n, b, *KS_SHAPE)              # noqa: E731
                out.append(S("ks", make(fit(make, "ks"))))
    return tuple(out)


def rows_of(family):
    return [s for s in scale_cases() if s.family == family]


def cases_of(family):
    """The rows of one family as plain cases, for the family's all_cases()."""
    return [s.case for s in rows_of(family)]


# ---------------------------------------------------------------------------------------------
# Kernels no scale case launches: (regular expression over the kernel_key, reason).  The first
# matching rule names a kernel's reason.
# ---------------------------------------------------------------------------------------------

SCALE_EXEMPT = (
    (r"k_server<.*>",
     "one resident workgroup by design: it never shares a compute unit with itself"),
    (r"k_(rns_)?check_range<.*>",
     "one word per thread, no LDS and no cross-lane step"),
    (r"k_rows<\w+,u\d+,u\d+,\d+,0,true>",
     "launched only while the whole batch is resident at once (at most 16 waves per compute unit, "
     "dispatch_cases.rows_prio): a launch of 2 * 8192 waves takes the other kernel; both sides of "
     "the threshold are held by test_issue_priority_variants"),
    (r"k_\w+<Arith32W,.*>",
     "the template covered as Arith32P and Arith64 with another modular multiply: thread layout, "
     "LDS exchanges and barriers do not depend on the arithmetic class"),
    (r"k_\w+<Arith32P3?,u64.*>|k_cols_(fwd|inv)<Arith32P,u64,.*>|k_xform<Arith32P,u32,u64,.*>"
     r"|k_pointwise<Arith32,u64>",
     "64-bit caller words on a 32-bit modulus: the template covered on 32-bit words, only its "
     "global loads and stores widen; both widths of the addressing are covered by the Arith64 rows"),
    (r"k_rns(mp)?_hoist<\w+,u\d+,\d+,1>",
     "comps = 1 of the template covered with comps = 2: one accumulator set fewer, the same "
     "exchanges and barriers"),
    (r"k_(rows|xform)<\w+,u\d+,u\d+,(9|11),0,\w+>|k_mac<\w+,u\d+,u\d+,(9|10|11)>"
     r"|k_rns_(rows|mac)<\w+,u\d+,(9|10|11)>|k_rns_xform<\w+,u\d+,(9|10|11),[01]>"
     r"|k_rns_(macn|hoist)<\w+,u\d+,(9|10|11),[12]>",
     "a degree strictly between two covered degrees of the same template"),
    # (n = 16384 and 32768 on 32-bit arithmetic; n = 16384 on 64-bit arithmetic, whose 2^L1 x 4096
    # split ends at 32768 in libnttmul.so)
    (r"k_cols_fwd<Arith32P,u32,[23],[12]>|k_cols_inv<Arith32P,u32,[23]>"
     r"|k_(rows|xform)<Arith32P,u32,u32,12,[23],\w+>"
     r"|k_cols_fwd<Arith64,u64,2,[12]>|k_cols_inv<Arith64,u64,2>"
     r"|k_(rows|xform)<Arith64,u64,u64,12,2,\w+>|k_rnsmp_rows<\w+,[23]>"
     r"|k_rnsmp_(cols_fwd|xform|macn|hoist)<\w+,u\d+,[23],[012]>|k_rnsmp_(cols_inv|mac)<\w+,u\d+,[23]>",
     "a degree strictly between two covered degrees of the same template"),
)


def exempt_reason(key):
    for pattern, reason in SCALE_EXEMPT:
        if re.fullmatch(pattern, key):
            return reason
    return None
