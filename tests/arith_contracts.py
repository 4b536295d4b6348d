"""The range contracts of the device arithmetic (csrc/modarith.hpp, csrc/mac_dev.hpp), as data.

One `Row` per op of lib/libnttmul_probe.so (tests/probe/arith_probe.hip), i.e. per primitive in
each template instantiation the kernels use:

* the input domain of every operand, as the comment of the primitive states it;
* the value every output must have: a congruence mod q, or an exact integer for csub, mulhi64,
  mullo64 and canon*;
* the range every output must lie in.

tests/test_gpu_arith_probe.py runs the ops on the tuples `tuples()` builds and asserts value and
range; tests/test_arith_probe_ledger.py holds the rows against the header text and the library's
op list.  Everything here is plain data and Python-integer arithmetic (numpy object arrays of
Python ints, so that one expression serves 32- and 64-bit classes): no GPU, no library.

Operand domains (q the modulus, W the class's word width):
  word    any W-bit word                      canon   [0, q)
  lazy2   [0, 2q)                             lazy4   [0, 4q)
  signed  an int32 in (-q, q), passed as its two's-complement word
  csub    the pair (x, m) of a conditional subtraction: m in {q, 2q}, x a word in [0, 2m)
  tw_u / tw_s   a twiddle as Arith32P's Plantard pair, unsigned / signed-input form
  tw_m    a twiddle in Arith32W's Montgomery form (w 2^32 mod q, that times -q^-1 mod 2^32)
  tw_h    a twiddle as Arith64's Shoup pair (w, floor(w 2^64 / q))
A twiddle operand is two words to the op and its plain value w to the reference.
"""
import itertools
import random
from collections import namedtuple

import numpy as np

import dispatch_cases as D

M32, M64 = 1 << 32, 1 << 64
N_RANDOM = 4096          # random tuples per (op, q)
N_RANDOM_BASE = 2048     # random vectors per base multiplication
CROSS_CAP = 120_000      # value-edge tuples x twiddles above this: the table twiddles rotate
TW_DOMS = ("tw_u", "tw_s", "tw_m", "tw_h")

# kind: "exact" (the integer) | "cong" (congruent mod q).  lo, hi: the half-open range, callables
# of (q, operands).  signed: the word is read as int32.  minus: index of a reference operand the
# output carries as an addend mod 2^W (Arith64::shoup's acc), subtracted before the checks
Out = namedtuple("Out", "kind lo hi signed minus", defaults=(False, None))
# base: 0, or B for a base multiplication (operands a[B], b[B] of domain operands[0][1], then z)
Row = namedtuple("Row", "op operands ref outs base")


def _zero(q, o):
    return 0


def _q(q, o):
    return q


def _2q(q, o):
    return 2 * q


def _4q(q, o):
    return 4 * q


def canon_out(kind="cong"):
    return Out(kind, _zero, _q)


def lazy2_out():
    return Out("cong", _zero, _2q)


def lazy4_out():
    return Out("cong", _zero, _4q)


# ---------------------------------------------------------------------------------------------
# References (object arrays of Python ints; % is the non-negative residue)
# ---------------------------------------------------------------------------------------------

def _rinv(q, bits):
    return pow(1 << bits, -1, q)


def _csub(q, x, m):
    return (np.where(x >= m, x - m, x),)


def _base_ref(B, neg, bits):
    """a b R^-1 in Z_q[x] / (x^B - z), z = -w when neg (R = 2^bits)."""
    def ref(q, *v):
        a, b, w = v[:B], v[B:2 * B], v[2 * B]
        z = -w if neg else w
        ri = _rinv(q, bits)
        out = []
        for k in range(B):
            s = 0
            for i in range(B):
                s = s + (a[i] * b[k - i] if i <= k else a[i] * b[B + k - i] * z)
            out.append(s * ri)
        return tuple(out)
    return ref


def _ct_ref(q, X, Y, w):
    return (X + Y * w, X - Y * w)


def _gs_ref(q, X, Y, w):
    return (X + Y, (X - Y) * w)


def _gs_scaled_ref(q, X, Y, f, wf):
    return ((X + Y) * f, (X - Y) * wf)


def _mont_ref(bits):
    return lambda q, a, b: (a * b * _rinv(q, bits),)


def _mulw(q, x, w):
    return (x * w,)


def _ident(q, x):
    return (x % q,)


def _add(q, a, b):
    return (a + b,)


# ---------------------------------------------------------------------------------------------
# The table
# ---------------------------------------------------------------------------------------------

def _rows():
    T, F = True, False
    rows = []

    def row(op, operands, ref, outs, base=0):
        rows.append(Row(op, tuple(operands), ref, tuple(outs), base))

    csub_out = [Out("exact", _zero, lambda q, o: o[1])]   # x in [0, 2m) -> [0, m)
    for cls in ("Arith32", "Arith32P", "Arith64"):
        row(f"{cls}.csub", [("xm", "csub")], _csub, csub_out)

    # Arith32: "inputs in [0, 2q), output in [0, 2q)"; "lazy -> [0, q)"
    row("Arith32.mont", [("a", "lazy2"), ("b", "lazy2")], _mont_ref(32), [lazy2_out()])
    row("Arith32.canon", [("x", "lazy2")], _ident, [canon_out("exact")])
    row("Arith32.canon_inv", [("x", "lazy2")], _ident, [canon_out("exact")])

    # Arith32P
    row("Arith32P.cadd", [("x", "signed")], _ident, [canon_out("exact")])   # (-q, q) -> [0, q)
    row("Arith32P.pmul", [("x", "word"), ("w", "tw_u")], _mulw, [canon_out()])
    row("Arith32P.shoup", [("x", "word"), ("w", "tw_u")], _mulw, [canon_out()])
    row("Arith32P.pmul_s", [("x", "signed"), ("w", "tw_s")], _mulw, [canon_out()])
    row("Arith32P.pmul_diff", [("x", "canon"), ("y", "canon"), ("w", "tw_s")],
        lambda q, x, y, w: ((x - y) * w,), [canon_out()])
    # "X in [0, 2q) (XC: canonical; XN: signed in (-q, q)), Y any -> X' in [0, 2q), Y' in (0, 2q)
    # (YN: x - t signed in (-q, q))"; "an N-type X comes with an N-type Y and a signed-form pair"
    for xc, xn, yn in ((T, F, F), (T, F, T), (F, F, F), (F, F, T), (F, T, F), (F, T, T)):
        name = "Arith32P.ct<%s,%s,%s>" % tuple("T" if v else "F" for v in (xc, xn, yn))
        xdom = "canon" if xc else "signed" if xn else "lazy2"
        yout = (Out("cong", lambda q, o: 1 - q, _q, signed=True) if yn
                else Out("cong", lambda q, o: 1, _2q))
        row(name, [("X", xdom), ("Y", "signed" if xn else "word"), ("w", "tw_s" if xn else "tw_u")],
            _ct_ref, [lazy2_out(), yout])
    # "X, Y canonical -> outputs canonical"
    row("Arith32P.gs", [("X", "canon"), ("Y", "canon"), ("w", "tw_s")], _gs_ref,
        [canon_out(), canon_out()])
    row("Arith32P.gs_scaled", [("X", "canon"), ("Y", "canon"), ("f", "tw_u"), ("wf", "tw_s")],
        _gs_scaled_ref, [canon_out(), canon_out()])
    row("Arith32P.mont", [("a", "lazy2"), ("b", "lazy2")], _mont_ref(32), [canon_out()])
    row("Arith32P.canon", [("x", "lazy2")], _ident, [canon_out("exact")])
    row("Arith32P.canon_inv", [("x", "lazy2")], _ident, [canon_out("exact")])
    # "a, b in [0, 2q) from the forward transform (a -w block: signed)", "reduced to [0, q)";
    # ZC: "the z pair is in signed form"
    for cls, B in (("Arith32P", 4), ("Arith32P3", 8)):
        for neg in (F, T):
            for zc in (F, T):
                row("%s.basemul<%d,%s,%s>" % (cls, B, "FT"[neg], "FT"[zc]),
                    [("ab", "signed" if neg else "lazy2"), ("z", "tw_s" if zc else "tw_u")],
                    _base_ref(B, neg, 32), [canon_out()] * B, base=B)
    for neg in (F, T):
        row("Arith32P.basemul4_lane<%s>" % "FT"[neg],
            [("ab", "signed" if neg else "lazy2"), ("z", "tw_s")],
            _base_ref(4, neg, 32), [canon_out()] * 4, base=4)

    # Arith32W: "values stay canonical in [0, q) and every sum / difference / product is reduced
    # completely"
    c2 = [("a", "canon"), ("b", "canon")]
    row("Arith32W.addmod", c2, _add, [canon_out()])
    row("Arith32W.submod", c2, lambda q, a, b: (a - b,), [canon_out()])
    row("Arith32W.shoup", [("x", "canon"), ("w", "tw_m")], _mulw, [canon_out()])
    row("Arith32W.mont", c2, _mont_ref(32), [canon_out()])
    row("Arith32W.ct", [("X", "canon"), ("Y", "canon"), ("w", "tw_m")], _ct_ref,
        [canon_out(), canon_out()])
    row("Arith32W.gs", [("X", "canon"), ("Y", "canon"), ("w", "tw_m")], _gs_ref,
        [canon_out(), canon_out()])
    row("Arith32W.gs_scaled", [("X", "canon"), ("Y", "canon"), ("f", "tw_m"), ("wf", "tw_m")],
        _gs_scaled_ref, [canon_out(), canon_out()])
    row("Arith32W.canon", [("x", "canon")], _ident, [canon_out("exact")])
    row("Arith32W.canon_inv", [("x", "canon")], _ident, [canon_out("exact")])

    # Arith64
    any2 = [("x", "word"), ("s", "word")]
    top = lambda q, o: M64
    for m in "FT":
        row(f"Arith64.mulhi64<{m}>", any2, lambda q, x, s: ((x * s) >> 64,), [Out("exact", _zero, top)])
    row("Arith64.mullo64", any2, lambda q, x, s: ((x * s) % M64,), [Out("exact", _zero, top)])
    # "acc + (x * w mod q, in [0, 2q)) mod 2^64 for any 64-bit x"
    for m in "TF":
        row(f"Arith64.shoup<{m}>", [("x", "word"), ("w", "tw_h"), ("acc", "word")],
            lambda q, x, w, acc: (x * w,), [Out("cong", _zero, _2q, minus=2)])
    # "X in [0, 4q), any Y -> outputs in [0, 4q)"; XC skips csub(X, 2q): X in [0, 2q)
    row("Arith64.ct<F>", [("X", "lazy4"), ("Y", "word"), ("w", "tw_h")], _ct_ref,
        [lazy4_out(), lazy4_out()])
    row("Arith64.ct<T>", [("X", "lazy2"), ("Y", "word"), ("w", "tw_h")], _ct_ref,
        [lazy4_out(), lazy4_out()])
    # "X, Y in [0, 2q) -> outputs in [0, 2q)"
    row("Arith64.gs", [("X", "lazy2"), ("Y", "lazy2"), ("w", "tw_h")], _gs_ref,
        [lazy2_out(), lazy2_out()])
    row("Arith64.gs_scaled", [("X", "lazy2"), ("Y", "lazy2"), ("f", "tw_h"), ("wf", "tw_h")],
        _gs_scaled_ref, [lazy2_out(), lazy2_out()])
    row("Arith64.canon", [("x", "lazy4")], _ident, [canon_out("exact")])      # [0, 4q) -> [0, q)
    row("Arith64.canon_inv", [("x", "lazy2")], _ident, [canon_out("exact")])  # [0, 2q) -> [0, q)
    # "a, b lazy (< kLazy q) -> [0, 2q)"
    row("Arith64.mont", [("a", "lazy4"), ("b", "lazy4")], _mont_ref(64), [lazy2_out()])
    for neg in (F, T):
        row("Arith64.basemul<4,%s>" % "FT"[neg], [("ab", "lazy4"), ("z", "tw_h")],
            _base_ref(4, neg, 64), [lazy2_out()] * 4, base=4)

    # mac_add: "acc + m mod q in the range the class's inverse butterflies read"
    row("mac_add.Arith32P", c2, _add, [canon_out()])
    row("mac_add.Arith32W", c2, _add, [canon_out()])
    row("mac_add.Arith64", [("acc", "lazy2"), ("m", "lazy2")], _add, [lazy2_out()])
    return rows


ROWS = _rows()
BY_OP = {r.op: r for r in ROWS}

# __device__ members without a row: (struct, function) -> reason
EXEMPT = {
    ("Arith32W", "basemul"): "empty: kBaseD = 0, the class runs complete transforms",
    ("Arith32W", "redc"): "its second operand is implied by the first; shoup and mont are its rows",
    ("Arith32P3", "outputs"): "the recursion of basemul<8, ...>, whose rows run it",
}


def op_class(op):
    """The arithmetic class an op runs in: 'Arith32P.ct<T,F,F>' and 'mac_add.Arith32P' alike."""
    head, tail = op.split(".", 1)
    return tail if head == "mac_add" else head


def op_function(op):
    """(struct, function) as the headers spell them; mac_add's struct is its class argument."""
    head, tail = op.split(".", 1)
    if head == "mac_add":
        return (tail, "mac_add")
    return (head, tail.split("<")[0])


def word_bits(cls):
    return 64 if cls == "Arith64" else 32


# ---------------------------------------------------------------------------------------------
# Moduli: primes q == 1 (mod 512), so that make_plan(256, q) accepts them
# ---------------------------------------------------------------------------------------------

P31, P32, P62 = 2147483137, 4294962689, 4611686018427379201   # nttmul.find_prime(256, bits)
W_FIRST, L_FIRST = 2147484161, 4294968833     # the smallest such primes >= 2^31 and >= 2^32
_PLANTARD = (7681, 12289, D.Q31LO, D.Q31, D.Q31HI, P31)
# plain data, so that collecting the tests loads no library; test_arith_probe_ledger.py holds
# the searched entries against nttmul.find_prime / nttmul.is_prime
MODULI = {
    "Arith32": _PLANTARD, "Arith32P": _PLANTARD,
    "Arith32P3": tuple(q for q in _PLANTARD if D.p3_fold_ok(q)),
    "Arith32W": (W_FIRST, P32),
    "Arith64": (L_FIRST, D.Q33, D.Q62, P62),
}


# ---------------------------------------------------------------------------------------------
# Twiddles
# ---------------------------------------------------------------------------------------------

def plantard_pair(w, q, signed=False):
    """planner.cpp tw_pair, Arith32P: BR = (-w 2^64 mod q) q^-1 mod 2^64 as (low, high) words;
    signed-input form: the high word absorbs the sign of the low one."""
    br = ((-w * pow(2, 64, q)) % q) * pow(q, -1, M64) % M64
    b0, b1 = br % M32, br >> 32
    return (b0, (b1 + (b0 >> 31)) % M32) if signed else (b0, b1)


def mont_pair(w, q):
    """planner.cpp tw_pair, Arith32W: (w 2^32 mod q, that times -q^-1 mod 2^32)."""
    w1 = (w << 32) % q
    return (w1, w1 * (-pow(q, -1, M32)) % M32)


def shoup_pair(w, q):
    """planner.cpp tw_pair, Arith64: (w, floor(w 2^64 / q))."""
    return (w, (w << 64) // q)


def pair_of(form, w, q):
    return {"tw_u": lambda: plantard_pair(w, q), "tw_s": lambda: plantard_pair(w, q, True),
            "tw_m": lambda: mont_pair(w, q), "tw_h": lambda: shoup_pair(w, q)}[form]()


def edge_twiddles(q):
    return sorted({1, 2, q - 2, q - 1, (q - 1) // 2, (q + 1) // 2})


def table_forms(q, fw_signed):
    """The form of each entry of the plan's forward and inverse pair tables (entry 0 unused)."""
    if q < (1 << 31):
        return (["tw_s" if s else "tw_u" for s in fw_signed], ["tw_s"] * len(fw_signed))
    form = "tw_m" if q < (1 << 32) else "tw_h"
    return ([form] * len(fw_signed),) * 2


def twiddle_lists(q, fw_pairs, iw_pairs, fw_signed, fw_plain, iw_plain):
    """{form: [(w, value word, companion word)]}: every pair of the plan's two tables under the
    form the planner stored it in, then the edge twiddles in each form of q's class."""
    fforms, iforms = table_forms(q, fw_signed)
    out = {}
    for forms, pairs, plain in ((fforms, fw_pairs, fw_plain), (iforms, iw_pairs, iw_plain)):
        for i in range(1, len(forms)):
            out.setdefault(forms[i], []).append((int(plain[i]), int(pairs[i][0]), int(pairs[i][1])))
    for form in (("tw_u", "tw_s") if q < (1 << 31) else ("tw_m",) if q < (1 << 32) else ("tw_h",)):
        out.setdefault(form, [])
        out[form] += [(w,) + pair_of(form, w, q) for w in edge_twiddles(q)]
    return out


def python_twiddle_lists(q, count=16, seed=5):
    """twiddle_lists without a library: `count` seeded residues in place of the plan's tables."""
    rng = random.Random(seed ^ q)
    out = {}
    for form in (("tw_u", "tw_s") if q < (1 << 31) else ("tw_m",) if q < (1 << 32) else ("tw_h",)):
        ws = [rng.randrange(1, q) for _ in range(count)] + edge_twiddles(q)
        out[form] = [(w,) + pair_of(form, w, q) for w in ws]
    return out


# ---------------------------------------------------------------------------------------------
# Operand values
# ---------------------------------------------------------------------------------------------

def _halves(hi_bound):
    """64-bit words below hi_bound with an all-zero or all-ones 32-bit half, and with an all-ones
    or all-zero low 31-bit limb (the splits of mulhi64 / mullo64 / shoup and of basemul)."""
    out = {M32 - 1, M32, M32 + 1, (1 << 31) - 1, 1 << 31}
    top = (hi_bound - 1) >> 32
    for h in {1, top // 2, max(top - 1, 0), top}:
        out |= {h << 32, (h << 32) | (M32 - 1), ((h << 32) - 1) % M64}
    top31 = (hi_bound - 1) >> 31
    for h in {1, top31 // 2, top31}:
        out |= {h << 31, (h << 31) - 1}
    return {v for v in out if 0 <= v < hi_bound}


def domain_bounds(dom, q, bits):
    """[lo, hi) of a value domain, as integers (signed: the int32 values)."""
    return {"word": (0, 1 << bits), "canon": (0, q), "lazy2": (0, 2 * q), "lazy4": (0, 4 * q),
            "signed": (1 - q, q)}[dom]


def edges(dom, q, bits):
    """Both ends of the domain, their neighbours, and the points where a conditional subtraction
    or a carry flips."""
    lo, hi = domain_bounds(dom, q, bits)
    if dom == "signed":
        h = q // 2
        return sorted({0, 1, -1, q - 1, 1 - q, q - 2, 2 - q, h, -h, h + 1, -h - 1})
    pts = set()
    for k in range(0, 5):
        pts |= {k * q - 1, k * q, k * q + 1}
    pts |= {q // 2, q // 2 + 1, q - 2, 2 * q - 2, 4 * q - 2, 2}
    pts |= {(1 << 31) - 1, 1 << 31, M32 - 1}
    if bits == 32:
        # where the 33-bit sums of Arith32W carry: a + b = 2^32 against a, b near q - 1 and 2^32 - q
        pts |= {M32 - q - 1, M32 - q, M32 - q + 1}
    else:
        pts |= {(1 << 63) - 1, 1 << 63, M64 - 1, M64 - 2} | _halves(hi)
    return sorted(v for v in pts if lo <= v < hi)


def rand_value(dom, q, bits, rng):
    lo, hi = domain_bounds(dom, q, bits)
    return rng.randrange(lo, hi)


def _csub_pairs(q, bits, rng):
    out = []
    for m in (q, 2 * q):
        top = min(2 * m, 1 << bits)      # x in [0, 2m), as far as the word reaches
        xs = {0, 1, m - 1, m, m + 1, 2 * m - 2, 2 * m - 1, m // 2, top - 1}
        if bits == 64:
            xs |= _halves(top)
        out += [(x, m) for x in sorted(xs) if 0 <= x < top]
        out += [(rng.randrange(top), m) for _ in range(N_RANDOM // 2)]
    return out


def _base_vectors(dom, q, bits, B, rng):
    """Patterned (a, b) vector pairs of a base multiplication, then the random ones."""
    lo, hi = domain_bounds(dom, q, bits)
    mn, mx = lo, hi - 1
    fill = lambda v: [v] * B

    def hot(p, v, rest=0):
        return [v if i == p else rest for i in range(B)]

    def alt(u, v):
        return [u if i % 2 == 0 else v for i in range(B)]

    pats = [(fill(mn), fill(mn)), (fill(mx), fill(mx)), (fill(mn), fill(mx)), (fill(mx), fill(mn)),
            (fill(q - 1), fill(q - 1)), (fill(0), fill(mx)), (fill(1), fill(1))]
    if dom == "signed":
        pats += [(fill(1 - q), fill(q - 1)), (fill(-1), fill(-1))]
    else:
        pats += [(fill(q), fill(q)), (fill(q - 1), fill(2 * q - 1)), (fill(2 * q - 1), fill(q - 1))]
    for p in range(B):
        pats += [(hot(p, mx), fill(mx)), (fill(mx), hot(p, mx)), (hot(p, mx), hot(B - 1 - p, mx)),
                 (hot(p, q - 1), hot(p, q - 1)), (hot(p, mn, mx), hot(p, mx, mn))]
    for u, v in ((mx, mn), (mn, mx), (mx, 0), (0, mx), (q - 1, 0), (0, q - 1)):
        pats += [(alt(u, v), alt(u, v)), (alt(u, v), alt(v, u))]
    if bits == 64:
        # canonical values with an all-ones low 31-bit limb, reached from every lazy copy, and
        # with an all-zero one
        ones = (((q - 1) >> 31) << 31) - 1
        zero = ((q - 1) >> 31) << 31
        small = (1 << 31) - 1
        for v in (ones, zero, small):
            copies = [v + k * q for k in range(4) if v + k * q < hi]
            pats += [(fill(v), fill(v)), (fill(copies[-1]), fill(copies[len(copies) // 2])),
                     (alt(v, copies[-1]), alt(copies[-1], v))]
    rnd = [([rng.randrange(lo, hi) for _ in range(B)], [rng.randrange(lo, hi) for _ in range(B)])
           for _ in range(N_RANDOM_BASE)]
    return pats, rnd


def tuples(row, q, tw, seed=1):
    """(words, values) for `row` at q: words[k] = the uint64 array of the op's operand word k,
    values[j] = the object array of reference operand j (a twiddle: its plain value).  tw: the
    twiddle lists (twiddle_lists or python_twiddle_lists)."""
    bits = word_bits(op_class(row.op))
    rng = random.Random(f"{seed}/{q}/{row.op}")
    cols = []          # one list of reference values per reference operand, twiddles as triples

    if row.base:
        B = row.base
        dom, form = row.operands[0][1], row.operands[1][1]
        pats, rnd = _base_vectors(dom, q, bits, B, rng)
        zs = tw[form]
        recs = [(a, b, z) for a, b in pats for z in zs]
        recs += [(a, b, zs[rng.randrange(len(zs))]) for a, b in rnd]
        vals = [[r[0][i] for r in recs] for i in range(B)] + [[r[1][i] for r in recs] for i in range(B)]
        return _pack(vals + [[r[2] for r in recs]], [dom] * (2 * B) + [form], bits)

    if row.operands[0][1] == "csub":
        recs = _csub_pairs(q, bits, rng)
        return _pack([[r[0] for r in recs], [r[1] for r in recs]], ["word", "word"], bits)

    doms = [d for _, d in row.operands]
    vdoms = [d for d in doms if d not in TW_DOMS]
    tdoms = [d for d in doms if d in TW_DOMS]
    vcross = list(itertools.product(*[edges(d, q, bits) for d in vdoms]))
    # twiddle operands: one -> every twiddle; two (gs_scaled) -> the edge twiddles crossed, and the
    # two lists zipped
    if len(tdoms) == 1:
        tws = [(t,) for t in tw[tdoms[0]]]
        n_edge = len(edge_twiddles(q))
    elif len(tdoms) == 2:
        e = len(edge_twiddles(q))
        la, lb = tw[tdoms[0]], tw[tdoms[1]]
        tws = list(itertools.product(la[-e:], lb[-e:]))
        n_edge = len(tws)
        tws = [(la[i % len(la)], lb[(7 * i + 3) % len(lb)]) for i in range(max(len(la), len(lb)))] + tws
    else:
        tws, n_edge = [()], 1
    recs = []
    if len(vcross) * len(tws) <= CROSS_CAP:
        recs = [v + t for v in vcross for t in tws]
    else:
        # the edge twiddles (the tail of the list) meet every value tuple; the table's pairs take
        # the value tuples in rotation, at least 16 each
        recs = [v + t for v in vcross for t in tws[-n_edge:]]
        per = max(16, CROSS_CAP // len(tws))
        for i, t in enumerate(tws[:-n_edge]):
            recs += [vcross[(i * per + j) % len(vcross)] + t for j in range(per)]
    for _ in range(N_RANDOM):
        recs.append(tuple(rand_value(d, q, bits, rng) for d in vdoms)
                    + (tws[rng.randrange(len(tws))] if tdoms else ()))
    # back into the row's operand order
    order, vi, ti = [], 0, len(vdoms)
    for d in doms:
        if d in TW_DOMS:
            order.append(ti)
            ti += 1
        else:
            order.append(vi)
            vi += 1
    return _pack([[r[j] for r in recs] for j in order], doms, bits)


def _pack(cols, doms, bits):
    mask = (1 << bits) - 1
    words, values = [], []
    for col, dom in zip(cols, doms):
        if dom in TW_DOMS:
            values.append(np.array([t[0] for t in col], dtype=object))
            words.append(np.array([t[1] for t in col], dtype=np.uint64))
            words.append(np.array([t[2] for t in col], dtype=np.uint64))
        else:
            values.append(np.array(col, dtype=object))
            words.append(np.array([v & mask for v in col], dtype=np.uint64))
    return words, values


def check(row, q, values, outs):
    """Assert the contract of `row` on the op's outputs (uint64 arrays, one per output)."""
    bits = word_bits(op_class(row.op))
    want = row.ref(q, *values)
    assert len(want) == len(outs) == len(row.outs), row.op
    for k, (spec, w, got) in enumerate(zip(row.outs, want, outs)):
        g = got.astype(object)
        if spec.minus is not None:
            g = (g - values[spec.minus]) % (1 << bits)
        if spec.signed:
            g = np.where(g >= (1 << (bits - 1)), g - (1 << bits), g)
        lo, hi = spec.lo(q, values), spec.hi(q, values)
        bad = ~((g >= lo) & (g < hi))
        if spec.kind == "exact":
            wrong = g != w
        else:
            wrong = (g - w) % q != 0
        for what, mask in (("value", wrong), ("range", bad)):
            mask = np.asarray(mask, dtype=bool)
            if mask.any():
                i = int(np.flatnonzero(mask)[0])
                at = lambda v: int(v) if isinstance(v, int) else int(v[i])
                raise AssertionError(
                    f"{row.op} q={q} output {k}: wrong {what} at tuple {i} of {len(g)} "
                    f"({int(mask.sum())} wrong): operands {[int(v[i]) for v in values]}, "
                    f"got {int(g[i])}, want {spec.kind} "
                    f"{int(w[i]) % q if spec.kind == 'cong' else int(w[i])} "
                    f"in [{at(lo)}, {at(hi)})")
