"""One rule for the expected value of the eight NTT-domain libraries (mdntt, ksntt, lintrans, ctmul,
xconv, level, ctlin, tmd): the CPU reference of every output word, at every degree the GPU tests
run (n = 256 .. 65536).

reference(library, op, *inputs) calls the definitions where they are -- tests/mdntt_ref.py,
ksntt_ref.py, lintrans_ref.py, ctmul_ref.py, ctlin_ref.py, xconv_ref.py, tmd_ref.py, over the
oracle's transforms of tests/hoist_ref.py -- and nothing of nttmul that launches a kernel or runs
a host form (bconv_ref imports nttmul.is_prime for its bases, as before).  What makes the heavy
ones cheap enough to run ungated lives beside the definitions: exact uint64 products on 32-bit
words and the oracle's C pointwise product on 64-bit words (hoist_ref.mulmod, ksntt_ref.mac).

The comparison is on the NTT-domain output itself, bit for bit, on every word: equal().  The
coefficient-domain comparison on xconv_cases.sample_indices that the conversions were held to
above n = 512 is kept as sampled_equal() for the scale files, whose batches exist to fill the
machine, and for tests/test_full_ref.py, which shows what it does not see.

SUBSET names the cases whose reference is held on whole polynomials of a part of the batch only
(entry 0 and the last entry, the first and the last rotation or pair).  It is empty: after the
speed-ups the slowest single reference is below two seconds (README, testing)."""
import numpy as np

import bconv_ref as B
import ctlin_ref
import ctmul_ref
import hoist_ref as H
import ksntt_ref
import lintrans_ref
import mdntt_ref
import tmd_ref
import xconv_ref

LIBRARIES = ("mdntt", "ksntt", "lintrans", "ctmul", "xconv", "level", "ctlin", "tmd")

# {library: ((predicate over a case, reason, measured seconds), ..)}: the cases held on a subset.
# At most one case in ten per library, never the only case that launches some kernel
# (tests/test_*_ledger.py count only the cases outside it).
SUBSET = {lib: () for lib in LIBRARIES}


def on_subset(library, case):
    """Whether `case` is held on whole polynomials of a part of its batch only."""
    return any(pred(case) for pred, _, _ in SUBSET[library])


def conversion(library, op, x_hat, q, p, t=1, with_input=False):
    """(coefficients, transforms) of the three conversions between an inverse and a forward
    transform: the definition's coefficient-order output [batch, L, n] and its forward transform
    over Q, both in x_hat's dtype.  mdntt: bconv_ref.moddown with from = P, to = Q (the floor);
    xconv: extend or moddown (the rounding, exact outside the guard band); tmd: moddown.
    with_input: the oracle's inverse of x_hat in front, a triple."""
    q, p = tuple(q), tuple(p)
    x_hat = np.asarray(x_hat)
    assert op == "moddown" or (library, op) == ("xconv", "extend")
    x = mdntt_ref.inverse(x_hat, p if op == "extend" else q + p)
    if library == "mdntt":
        assert t == 1
        coef = B.moddown(x, p, q)
    elif library == "xconv":
        coef = getattr(xconv_ref, op + "_coeff")(x, q, p, t)
    else:
        assert library == "tmd"
        coef = tmd_ref.moddown_coeff(x, q, p, t)
    hat = H.forward(coef, q)
    return (x, coef, hat) if with_input else (coef, hat)


def reference(library, op, *inputs):
    """The CPU reference of every output word of one call, in the operands' dtype.

    mdntt   moddown   x_hat, q, p
    ksntt   modup     x_hat, q, p, alpha
            mac       a_hat, b_hat, ks, ext
    lintrans apply    a_hat, b_hat, ks, q, p, w_hat or None, c0_hat or None
    ctmul   high      x_hat, y_hat, q
            relin     up_hat, key_hat, x_hat, y_hat, q, p
    xconv   extend, moddown   x_hat, q, p, t
    tmd     moddown   x_hat, q, p, t
    ctlin   combine   terms, q, shape, dtype
            tensor    x_hat, y_hat, q
    level   mac, lintrans, relin   the dense call's operands (the key and the weights gathered by
                      level_ref.gather): ksntt mac, lintrans apply, ctmul relin"""
    if library == "level":
        library, op = {"mac": ("ksntt", "mac"), "lintrans": ("lintrans", "apply"),
                       "relin": ("ctmul", "relin")}[op]
    if library in ("mdntt", "xconv", "tmd"):
        return conversion(library, op, *inputs)[1]
    fn = {("ksntt", "modup"): ksntt_ref.modup, ("ksntt", "mac"): ksntt_ref.mac,
          ("lintrans", "apply"): lintrans_ref.apply,
          ("ctmul", "high"): ctmul_ref.high, ("ctmul", "relin"): ctmul_ref.relin,
          ("ctlin", "combine"): ctlin_ref.combine, ("ctlin", "tensor"): ctlin_ref.tensor}
    return fn[library, op](*inputs)


def equal(got, want):
    """The full comparison: every word of the NTT-domain output, bit for bit."""
    got, want = np.asarray(got), np.asarray(want)
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(got, want)


def mismatches(got, want):
    """Where a full comparison fails: the index tuples of up to eight differing words and their
    count, for the assertion's message."""
    bad = np.argwhere(np.asarray(got) != np.asarray(want))
    return len(bad), [tuple(int(v) for v in row) for row in bad[:8]]


def assert_equal(got, want, where=""):
    assert equal(got, want), (where, "words that differ from the CPU reference (count, first):",
                              mismatches(got, want) if np.shape(got) == np.shape(want)
                              else (np.shape(got), np.shape(want)))


def sampled_equal(got_hat, want_coef, q, idx, inverse=None):
    """The comparison the conversions were held to above n = 512: the inverse transform of the
    output over Q against the coefficient-order reference, on the coefficients idx alone.
    inverse: the transform to use (a library context's), the oracle's by default."""
    back = mdntt_ref.inverse(got_hat, tuple(q)) if inverse is None else inverse(got_hat)
    return np.array_equal(np.asarray(back)[:, :, idx], np.asarray(want_coef)[:, :, idx])
