"""BGV's plaintext-preserving ModDown on bases of mixed limb sizes (tests/basis_cases.py), at
n = 256 and n = 8192, in both directions: P above the limbs of Q (chain64, chain32) and P below
every q (chain64_rev, chain32_rev: a conversion from the smallest limbs into the largest), at
t = 3 and t = 65537; the references of tests/test_gpu_tmd.py (every coefficient in Python integers
at n = 256, the identity with the floor form at both)."""
import numpy as np
import pytest

import nttmul
import tmd_cases as C
from tmd_gpu import call, check

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _id(c):
    return f"{c.moduli}-n{c.n}-{c.L}.{c.K}-t{c.t}"


@pytest.mark.parametrize("case", C.bases_cases(), ids=_id)
def test_mixed_size_bases(case, torch_cuda):
    q, p = C.moduli_of(case)
    assert not all(a > b for a, b in zip(q, q[1:])) or case.moduli.endswith("_rev")
    x = C.bases_input(case)                            # the ends of every limb's range among them
    with nttmul.NttPlainModDown(case.n, q, p, case.t) as tm:
        assert (tm.q, tm.p, tm.word_bits) == (tuple(q), tuple(p), case.bits)
        got = call(torch_cuda, tm, x)
    check(case.n, q, p, case.t, x, got)
    assert got.dtype == np.dtype(np.uint32 if case.bits == 32 else np.uint64)
