"""End-to-end inputs that saturate a stage boundary (tests/saturation.py).

S(m, v), v in the first m coefficients and 0 elsewhere, is its own residue in every block of m
coefficients, so it steers chosen values to a stage boundary of the real kernels: S(m, q - 1)
puts canonical q - 1 in every position there, with m = 2^D in both operands every base block of
a fused product is all q - 1 (the worst case of the basemul folds and of Arith32P3's halfway
fold), and with m = 1 the whole NTT-domain operand is q - 1.  Uniform random operands, monomials
and the all-(q - 1) polynomial (m = n, the one member the suite had) reach none of that.

Expected products come from the closed form (tests/test_saturation_closed_form.py holds it
against the oracle on the CPU); random partners and transforms from the oracle."""
import numpy as np
import pytest

import dispatch_cases as D
import mac_cases as M
import nttmul
import rns_cases as R
import saturation as S
from oracle import oracle as O
from test_gpu_parity import _xf_expected, torch_cuda  # noqa: F401
from test_gpu_mac import _mac_device
from test_gpu_rns import _call as _rns_call

pytestmark = pytest.mark.gpu


def _dt(bits):
    return np.uint32 if bits == 32 else np.uint64


def _saturating(n, q):
    """[S(m, q - 1) for m = 1, 2, ..., n]."""
    return np.stack([S.poly(n, m, q - 1) for m in S.sizes(n)])


def _differ(got, want):
    return np.flatnonzero((got.astype(np.uint64) != want).any(axis=1))


# ---------------------------------------------------------------------------------------------
# products
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,q,bits", D.sat_products())
def test_products_over_the_family(n, q, bits, torch_cuda):
    """One launch per (n, q, words): every (m, m) pair with values (q - 1, q - 1) and (q - 1, 1)
    against the closed form, and S(m, q - 1) times one random operand against the oracle."""
    dt = _dt(bits)
    a, b, c = S.family(n, q)
    sat = _saturating(n, q)
    rnd = np.broadcast_to(O.fill_inputs(n, q, 11, 1)[0][0], sat.shape)
    want = np.concatenate([c, O.Plan(n, q).product_batch(sat, rnd)[0].reshape(sat.shape)])
    a, b = np.concatenate([a, sat]), np.concatenate([b, rnd])
    assert len(a) == D.sat_batch(n)
    ctx = nttmul.Context(n, q, small_server=-1)
    got = ctx.multiply(a.astype(dt), b.astype(dt), dtype=dt)
    assert list(nttmul.dispatched_kernel_hashes(ctx.kernel_name(bits, len(a)))) == \
        D.product_keys(D.Case("multiply", n, q, bits, len(a)))
    bad = _differ(got, want)
    assert bad.size == 0, f"{bad.size} of {len(a)} products differ, first row {bad[0]}"
    # and with the operands exchanged (a and b take different paths through the base blocks)
    bad = _differ(ctx.multiply(b.astype(dt), a.astype(dt), dtype=dt), want)
    assert bad.size == 0, f"exchanged: {bad.size} products differ, first row {bad[0]}"
    ctx.close()


def test_server_path_over_the_family(torch_cuda):
    """The resident server (n = 256, one product per call) on the same family, call by call."""
    n, q = D.SAT_SERVER
    assert D.kernels_of(D.Case("multiply", n, q, 32, 1, path="server")) == ["k_server<Arith32P,8>"]
    a, b, c = S.family(n, q)
    sat = _saturating(n, q)
    rnd = O.fill_inputs(n, q, 11, 1)[0][0]
    P = O.Plan(n, q)
    srv = nttmul.Context(n, q)
    for i in range(len(a)):
        got = srv.multiply(a[i].astype(np.uint32), b[i].astype(np.uint32))
        assert srv.last_host_path() == 3, i
        assert np.array_equal(got.astype(np.uint64), c[i]), i
    for i in range(len(sat)):
        got = srv.multiply(sat[i].astype(np.uint32), rnd.astype(np.uint32))
        assert srv.last_host_path() == 3
        assert np.array_equal(got.astype(np.uint64), P.product_merged(sat[i], rnd)), i
    assert srv.server_status() == (0, "")
    srv.close()


# ---------------------------------------------------------------------------------------------
# transforms
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,q", [(n, q) for n in D.SAT_N for q in D.sat_moduli(n)])
def test_transforms_over_the_family(n, q, torch_cuda):
    """forward(S(m, q - 1)) is the oracle's transform; forward(S(1, v)) is v in every word,
    exactly; inverse(forward(x)) == x over the family."""
    dt = _dt(D.native_bits(q))
    P = O.Plan(n, q)
    ctx = nttmul.Context(n, q)
    sat = _saturating(n, q)
    fwd = ctx.forward(sat.astype(dt), dtype=dt)
    want = np.stack([_xf_expected(P, x, 0, False, n, q) for x in sat])
    bad = _differ(fwd, want)
    assert bad.size == 0, f"forward: {bad.size} of {len(sat)} differ, first m = 2^{bad[0]}"
    assert np.array_equal(ctx.inverse(fwd, dtype=dt).astype(np.uint64), sat)
    vs = [1, 2, q - 1, q - 2, (q - 1) // 2, (q + 1) // 2, int(O.fill_inputs(n, q, 3, 1)[0][0][0])]
    const = np.stack([S.poly(n, 1, v) for v in vs])
    got = ctx.forward(const.astype(dt), dtype=dt).astype(np.uint64)
    assert np.array_equal(got, np.repeat(np.array(vs, dtype=np.uint64)[:, None], n, axis=1))
    # the inverse of a constant NTT-domain vector is S(1, v) again
    assert np.array_equal(ctx.inverse(got.astype(dt), dtype=dt).astype(np.uint64), const)
    ctx.close()


# ---------------------------------------------------------------------------------------------
# mac and RNS
# ---------------------------------------------------------------------------------------------

def _mac_operands(n, top, batch, terms):
    """a = S(1, q_l - 1) in every term, b_hat all q_l - 1; top: [limbs] of q_l - 1."""
    top = np.asarray(top, dtype=np.uint64)
    a = np.zeros((batch, terms, len(top), n), dtype=np.uint64)
    a[..., 0] = top
    b_hat = np.ascontiguousarray(np.broadcast_to(top[None, None, :, None], a.shape))
    return a, b_hat


@pytest.mark.parametrize("n,q", [(n, q) for n in D.SAT_MAC_N for q in D.sat_moduli(n)])
def test_mac_of_saturated_operands(n, q, torch_cuda):
    """k_mac: forward(S(1, q - 1)) is q - 1 in every word, each product with b_hat = q - 1 is 1,
    so seven terms give exactly [7 mod q, 0, 0, ...]; every accumulator input is at its top."""
    bits, batch, terms = D.native_bits(q), M.RANGE_BATCH, D.SAT_MAC_TERMS
    assert M.Case(n, q, bits, terms, False, batch) in M.all_cases()
    a, b_hat = _mac_operands(n, [q - 1], batch, terms)
    a, b_hat = a[:, :, 0], b_hat[:, :, 0]
    want = np.stack([S.poly(n, 1, terms % q)] * batch)
    ctx = nttmul.MacContext(n, q)
    for shared in (False, True):
        got, _, _ = _mac_device(torch_cuda, ctx, a, b_hat[0] if shared else b_hat, shared, bits)
        assert np.array_equal(got, want), shared
    ctx.close()


@pytest.mark.parametrize("n", D.SAT_MAC_N)
@pytest.mark.parametrize("moduli", R.BASES)
def test_rns_mac_of_saturated_operands(n, moduli, torch_cuda):
    """k_rns_mac, one basis per class: limb l of the result is exactly [7 mod q_l, 0, 0, ...]."""
    batch, terms = R.RANGE_BATCH, D.SAT_MAC_TERMS
    assert R.Case("mac", n, moduli, batch, terms, False) in R.all_cases()
    a, b_hat = _mac_operands(n, [q - 1 for q in moduli], batch, terms)
    want = np.stack([np.stack([S.poly(n, 1, terms % q) for q in moduli])] * batch)
    ctx = nttmul.RnsContext(n, moduli)
    for shared in (False, True):
        got, _ = _rns_call(torch_cuda, ctx, "mac", a, b_hat[0] if shared else b_hat, shared=shared)
        assert np.array_equal(got, want), shared
    ctx.close()
