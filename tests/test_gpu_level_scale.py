"""The view kernels under full occupancy, by the rule of tests/scale_cases.py: the launch of a scale
case (tests/level_cases.py scale_cases: level 3 of the five-limb chain, two components; k_level_mac
at n = 256 with three rotations, k_level_lintrans at n = 4096 with three rotations, weights and
c_0, k_level_relin at n = 4096 with two pairs; both word classes) holds at least 2 * 8192 waves,
with the smallest batch that meets it and ends in a partial last workgroup.  Inputs are made on the
device, the output is preset to a sentinel no canonical word equals, and every word is compared on
the device with the dense call of the same context on level_ref.gather of the key.

The batches here exist to fill the machine (at least 16384 waves per launch), so an integer
reference of every output word would be minutes of CPU: this file keeps its sampled check.  The CPU
reference of every output word, at every degree, is held in test_gpu_level.py (tests/full_ref.py)."""
import pytest

import level_cases as C
import level_gpu as G
import scale_cases as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.mark.parametrize("case", C.scale_cases(), ids=G.case_id)
def test_full_occupancy(case, torch_cuda):
    torch = torch_cuda
    (name, waves), = C.launch_waves(case).items()
    assert name == C.kernel_name(case) and waves >= S.MIN_WAVES and C.ends_partial(case)
    ops = G.operands(torch, case, seed=3)
    key, w = G.gathered(case, ops)
    with G.context(case) as ctx:
        got = G.call(torch, ctx, case, ops, C.VIEW)
        want = G.call(torch, ctx, case, ops, None, key=key, w=w)
    assert not bool((got == -1).any())
    bad = torch.nonzero((got != want).reshape(case.batch, -1).any(dim=1)).reshape(-1)
    assert bad.numel() == 0, f"{bad.numel()} entries differ, first {int(bad[0])}"
