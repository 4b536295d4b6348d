"""Why a level view is sound (include/nttmul_level.h), in Python integers only: the gadget factors
of a key made for the whole chain, restricted to the limbs and terms a view selects, are the
gadget factors of the key made at that level.  Every word of a key is a_d (uniform, per limb) or
b_d = -a_d s + gadget_d s' + e, limb by limb, so equal gadget rows mean equal keys for the same a
and e.  Also tests/level_ref.gather, the definition the GPU tests hold the view calls to.  No GPU."""
import numpy as np
import pytest

import basis_cases as BC
import ks_ref
import level_ref as LR

L_TOP = BC.MAX_SHAPE[0]
PROFILES = tuple(p for bits in (32, 64) for p in BC.CHAINS[bits])


@pytest.mark.parametrize("K", (1, 2))
@pytest.mark.parametrize("alpha", (1, 2, 3, 4, 5))
@pytest.mark.parametrize("profile", PROFILES)
def test_the_view_of_a_top_level_gadget_is_the_gadget_of_the_level(profile, alpha, K):
    q, p = BC.basis(profile, L_TOP, K)
    g_top = np.array(ks_ref.gadget(q, p, alpha), dtype=object)      # [top_terms][L_top + K]
    top_terms = LR.terms_of(L_TOP, alpha)
    assert g_top.shape == (top_terms, L_TOP + K)
    for L in range(1, L_TOP + 1):                                   # includes L < alpha and alpha ∤ L
        a = min(alpha, L)                                           # a digit is never wider than Q
        terms = LR.terms_of(L, alpha)
        assert terms == LR.terms_of(L, a) or L < alpha
        g_level = ks_ref.gadget(q[:L], p, a)
        assert len(g_level) == terms
        got = LR.gather(g_top[..., None], (L_TOP, top_terms), L, terms)[..., 0]
        assert got.tolist() == g_level, (profile, alpha, K, L)
        # the rows themselves: P mod q_i on the digit's own limbs of Q, 0 elsewhere in Q u P
        P = 1
        for m in p:
            P *= m
        for d, D in enumerate(ks_ref.digits(L, a)):
            for i, m in enumerate(tuple(q[:L]) + tuple(p)):
                assert g_level[d][i] == (P % m if i in D else 0)


def test_terms_above_the_level_hold_nothing_the_level_needs():
    """The terms ceil(L / alpha) .. top_terms - 1 of a top-level key have gadget 0 on every limb a
    level-L context reads: dropping them drops only a_d s-cancelling noise-free zero terms."""
    q, p = BC.basis("chain64", L_TOP, 2)
    for alpha in (1, 2, 3):
        g_top = ks_ref.gadget(q, p, alpha)
        for L in range(1, L_TOP):
            idx = LR.limbs(L, 2, L_TOP)
            for d in range(LR.terms_of(L, alpha), len(g_top)):
                assert all(g_top[d][m] == 0 for m in idx)


def test_gather_is_the_definition_of_the_view():
    rng = np.random.default_rng(5)
    L_top, K, top_terms, n = 5, 2, 3, 4
    key = rng.integers(0, 1 << 30, size=(3, 2, top_terms, L_top + K, n), dtype=np.uint64)
    diag = rng.integers(0, 1 << 30, size=(3, L_top + K, n), dtype=np.uint64)
    for L, terms in ((5, 3), (4, 2), (3, 2), (1, 1)):
        assert LR.limbs(L, K, L_top) == list(range(L)) + [L_top, L_top + 1]
        got = LR.gather(key, (L_top, top_terms), L, terms)
        assert got.shape == (3, 2, terms, L + K, n) and got.flags.c_contiguous
        for m in range(L + K):
            assert np.array_equal(got[:, :, :, m], key[:, :, :terms, LR.top(m, L, L_top)])
        gd = LR.gather(diag, (L_top, top_terms), L, None)
        assert gd.shape == (3, L + K, n)
        for m in range(L + K):
            assert np.array_equal(gd[:, m], diag[:, LR.top(m, L, L_top)])
        mask = LR.selected(key.shape, (L_top, top_terms), L, terms)
        assert mask.sum() == got.size and np.array_equal(key[mask], got.ravel())
        assert LR.selected(diag.shape, (L_top, top_terms), L, None).sum() == gd.size
    # the identity view
    assert np.array_equal(LR.gather(key, (L_top, top_terms), L_top, top_terms), key)
    assert LR.selected(key.shape, (L_top, top_terms), L_top, top_terms).all()
