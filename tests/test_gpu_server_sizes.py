"""The resident device server (csrc/kernels_dev.hpp k_server) at every size it serves and over
the whole Plantard range, negacyclic and cyclic."""
import numpy as np
import pytest

import dispatch_cases as D
import nttmul
from oracle import oracle as O
from test_gpu_parity import _random_primes, torch_cuda  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("cyclic", [False, True])
@pytest.mark.parametrize("n,batch", D.SERVER_SHAPES)
def test_server_every_size_and_modulus(n, batch, cyclic, torch_cuda):
    """test_small_server_two_wave_path's sweep on the other server kernels: n = 512 with one
    product (the split lane-group path) and two (two products per wave), n = 1024 (the paired
    two-wave path), n = 256 with 2, 3 and 4 products (the waves past the count only keep the
    barriers).  Random primes of every Plantard width (2n | q - 1) plus 12289, the benchmark
    modulus and both ends of (2^30, 2^31), where the typed butterflies' bounds are tightest;
    operands random, a all q - 1, both all q - 1, and b = x^(n-1).  Every call is served by the
    server (path 3, no setup failure) and equals the oracle's product -- the restated reference
    product, or the schoolbook product in cyclic mode -- and the launch-per-call context's.
    run_server's twiddle-count condition declines none of these cases: the planner's tables
    hold exactly n pairs for every (n, q), so no case takes the documented launch path."""
    step = (2 * n).bit_length() - 1
    assert D.kernels_of(D.Case("multiply", n, D.Q31, 32, batch, path="server")) == \
        [f"k_server<Arith32P,{step - 1}>"]
    for q in _random_primes(list(D.SERVER_BITS), step, seed=n + cyclic) + list(D.SERVER_NAMED):
        P = O.Plan(n, q)
        srv = nttmul.Context(n, q, cyclic=cyclic)
        launch = nttmul.Context(n, q, cyclic=cyclic, small_server=-1)
        for pattern in range(4):
            a, b = O.fill_inputs(n, q, 7 * pattern + (q & 0xFF), batch)
            if pattern in (1, 2):
                a[:] = q - 1
            if pattern == 2:
                b[:] = q - 1
            if pattern == 3:
                b[:] = 0
                b[:, n - 1] = 1
            a32, b32 = a.astype(np.uint32), b.astype(np.uint32)
            got = srv.multiply(a32, b32).astype(np.uint64)
            assert srv.last_host_path() == 3, (q, pattern)
            for i in range(batch):
                exp = (O.cyclic_schoolbook(a[i], b[i], n, q) if cyclic
                       else P.product_merged(a[i], b[i]))
                assert np.array_equal(got[i], exp), (q, cyclic, pattern, i)
            assert np.array_equal(launch.multiply(a32, b32).astype(np.uint64), got), (q, pattern)
            assert launch.last_host_path() == 2
        assert srv.server_status() == (0, "")
        srv.close()
        launch.close()
