"""Anchor of tests/dispatch_cases.py's dispatch mirror to the library's own dispatch.

The library can be asked which kernels a product call launches (nttmul_kernel_name_batch, a dry
run of the launching statements) and which the last product call did launch
(nttmul_last_kernel_name).  Transforms, pointwise products, fills and range checks have no name
query, so that part of the mirror rests on reading csrc/kernels.hip and is checked only through
tests/test_kernel_ledger.py (every name it produces is a kernel of the library) and the parity
tests that run those cases."""
import pytest

import dispatch_cases as D
import nttmul
from test_gpu_parity import torch_cuda  # noqa: F401

pytestmark = pytest.mark.gpu


def _product_cases(cus):
    seen, out = set(), []
    for case in D.all_cases(cus):
        # (prio_ok = 0 is the state after a launch on another stream: no dry-run query for it;
        # test_issue_priority_follows_streams pins those names)
        if case.op != "multiply" or case.path != "device" or not case.prio_ok:
            continue
        key = (case.n, case.q, case.word_bits, case.batch, case.prio)
        if key not in seen:
            seen.add(key)
            out.append(case)
    return out


def _keys(names):
    return [nttmul.dispatch_key(k) for k in names.split("+")]


def test_mirror_agrees_with_the_library_dispatch(torch_cuda):
    """For each product case of the tables, nttmul_kernel_name_batch mapped through dispatch_key
    equals kernels_of(case) (with this device's compute-unit count in the priority rule); and for
    one case per distinct kernel list, the smallest, a launch reports the same kernels."""
    torch = torch_cuda
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    cases = _product_cases(cus)
    assert len(cases) > 100
    ctxs, smallest = {}, {}
    for case in cases:
        ck = (case.n, case.q, case.prio)
        if ck not in ctxs:
            ctxs[ck] = nttmul.Context(case.n, case.q, issue_prio=case.prio)
        want = D.product_keys(case, cus)
        assert _keys(ctxs[ck].kernel_name(case.word_bits, case.batch)) == want, case
        best = smallest.get(tuple(want))
        if best is None or case.batch * case.n < best.batch * best.n:
            smallest[tuple(want)] = case
    s = torch.cuda.current_stream().cuda_stream
    for want, case in smallest.items():
        # a fresh context: its first product launch has no previous stream to differ from
        ctx = nttmul.Context(case.n, case.q, issue_prio=case.prio)
        dt = torch.int32 if case.word_bits == 32 else torch.int64
        a = torch.empty(case.batch * case.n, dtype=dt, device="cuda")
        b, c = torch.empty_like(a), torch.empty_like(a)
        ctx.fill_random_device(a, b, 0, case.batch, case.word_bits, stream=s)
        ctx.multiply_device(c, a, b, case.batch, case.word_bits, stream=s)
        assert _keys(ctx.last_kernel_name()) == list(want), case
        torch.cuda.synchronize()
        ctx.close()
