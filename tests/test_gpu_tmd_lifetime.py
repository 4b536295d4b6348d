"""One long-lived nttmul_tmd context from its first call to its last, in the style of
tests/limb_lifetime_cases.py's sequences: csrc/tmd.cpp carries a fifth written-out copy of the
scratch state machine of csrc/mdntt.cpp (grow a buffer after an event synchronise on the last use,
a stream wait when the stream changes, sub-batches through the scratch, the event recorded after
the launches, the host form on the context's own stream), so the states a single call never
reaches are walked here: the first use, a change of stream with the scratch in use, growth while
in use, a call split into sub-batches after a whole one, the host form between device forms, a
refused call (NTTMUL_ERANGE) between two good ones, and a smaller call after a larger.  Every step
runs on inputs of its own and is held to the identity of tests/tmd_gpu.py."""
import numpy as np
import pytest

import nttmul
import tmd_cases as C
from tmd_gpu import check, to_dev

pytestmark = pytest.mark.gpu

# (place, batch, status): device operands on caller stream "A", "B" or the "null" stream; "host":
# the host form.  scratch_mb = 1 at n = 8192, (L, K) = (3, 2): 10 polynomials per sub-batch on
# 32-bit words, 5 on 64-bit words
STEPS = (("A", 1, "OK"), ("B", 3, "OK"), ("B", 23, "OK"), ("host", 2, "OK"), ("A", 4, "ERANGE"),
         ("null", 11, "OK"), ("A", 1, "OK"), ("host", 12, "OK"), ("B", 23, "OK"))
N, SHAPE, T = 8192, (3, 2), 65537


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.mark.parametrize("bits", (32, 64))
def test_sequence_on_one_context(bits, torch_cuda):
    torch = torch_cuda
    L, K = SHAPE
    q, p = C.moduli_of(C.Case(bits, N, 1, L, K, T))
    streams = {"A": torch.cuda.Stream(), "B": torch.cuda.Stream()}
    dtype = torch.int32 if bits == 32 else torch.int64
    assert len(C.chunks(C.Case(bits, N, 23, L, K, T, False, 1))) >= 3        # sub-batched steps
    pending = []
    with nttmul.NttPlainModDown(N, q, p, T, validate=True, scratch_mb=1) as tm:
        for i, (place, batch, status) in enumerate(STEPS):
            x = C.seeded_input(C.Case(bits, N, batch, L, K, T), seed=1000 + 17 * i + bits)
            if status == "ERANGE":
                x[batch - 1, L, N - 1] = p[0]
            if place == "host":
                pending.append((x, tm.moddown(x)))
                continue
            s = streams[place].cuda_stream if place in streams else 0
            out = torch.full((batch, L, N), -1, dtype=dtype, device="cuda")
            xd = to_dev(torch, x, bits)
            if place in streams:          # the operands were made on the null stream
                streams[place].wait_stream(torch.cuda.current_stream())
            if status == "ERANGE":
                with pytest.raises(nttmul.NttmulError) as ei:
                    tm.moddown_device(out, xd, batch, stream=s)
                assert ei.value.status == nttmul.NTTMUL_ERANGE
                torch.cuda.synchronize()
                assert bool((out == -1).all())
                continue
            # no synchronise between the steps: the scratch is handed from stream to stream
            tm.moddown_device(out, xd, batch, stream=s)
            pending.append((x, (out, xd)))
        torch.cuda.synchronize()
    for x, got in pending:
        if isinstance(got, tuple):
            got = got[0].cpu().numpy().view(x.dtype).reshape(x.shape[0], L, N)
        check(N, q, p, T, x, got)
