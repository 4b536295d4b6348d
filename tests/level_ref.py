"""The definition of a level view (include/nttmul_level.h) and the helpers the level tests share.
No GPU and no library load at import.

A viewed operand has the axes [..., top_terms, top_q_limbs + K, n] (a key) or
[..., top_q_limbs + K, n] (a diagonal set, terms = None).  A context of L limbs of Q and K of P
reads limb m of term t at limb top(m) of term t: top(m) = m for m < L and m + (top_q_limbs - L)
for m >= L.  gather is that sentence on an array; the dense call on gather(operand) is what a view
call must equal bit for bit."""
import numpy as np


def top(m, L, top_q_limbs):
    """The operand's limb behind limb m of a context of L limbs of Q."""
    return m if m < L else m + (top_q_limbs - L)


def limbs(L, K, top_q_limbs):
    """top(0) .. top(L + K - 1)."""
    assert 1 <= L <= top_q_limbs and K >= 1
    return [top(m, L, top_q_limbs) for m in range(L + K)]


def gather(top_operand, view, L, terms):
    """The dense operand a context of L limbs of Q reads through view = (top_q_limbs, top_terms):
    [..., top_terms, top_q_limbs + K, n] -> [..., terms, L + K, n]; terms = None for an operand
    without a term index, [..., top_q_limbs + K, n] -> [..., L + K, n].  numpy arrays and torch
    tensors alike; the result is a contiguous copy."""
    top_q_limbs, top_terms = view
    K = top_operand.shape[-2] - top_q_limbs
    idx = limbs(L, K, top_q_limbs)
    if terms is not None:
        assert top_operand.shape[-3] == top_terms and 1 <= terms <= top_terms
        top_operand = top_operand[..., :terms, :, :]
    out = top_operand[..., idx, :]
    return np.ascontiguousarray(out) if isinstance(out, np.ndarray) else out.contiguous()


def selected(shape, view, L, terms):
    """Boolean numpy mask over an operand of `shape`: True on the words the view selects."""
    top_q_limbs, top_terms = view
    K = shape[-2] - top_q_limbs
    mask = np.zeros(shape, dtype=bool)
    idx = limbs(L, K, top_q_limbs)
    if terms is None:
        mask[..., idx, :] = True
    else:
        mask[..., :terms, idx, :] = True
    return mask


def terms_of(L, alpha):
    """ceil(L / alpha): the digits, and so the terms, of a level of L limbs."""
    return -(-L // alpha)
