"""The resident device server's failure and retry paths, and the compat shims under concurrent
callers.

The sequences are lifetime_cases.SERVER_SEQUENCES on contexts of the diagnostic library
(lib/libnttmul_diag.so, include/nttmul_diag.h): a step arms failure points, each of which replaces
one host-side runtime call by an error once (nothing is injected on the device), or lets the
resident kernel leave through its idle exit before the request is posted.  After every step of
every sequence:

* the status, nttmul_last_host_path and nttmul_last_kernel_name are what the model of
  lifetime_cases.py derives from the state before the step;
* nttmul_server_status gives the model's failure count and the fixed parts of the reason;
* nttmul_diag_server_state gives the model's state, and the two invariants hold: the go word
  equals the last one served (a kernel launched now would serve nothing), and neither half of the
  mailbox is held as a host pointer without its device pointer;
* no error text appears but the staged range failure's.

After the sequence every product is compared bit for bit with the oracle, the products of the
calls that carried a failure included (test_gpu_lifetime.Run: outputs preset to a sentinel inside
guarded arenas, inputs unchanged)."""
import os
import threading

import numpy as np
import pytest

import dispatch_cases as D
import lifetime_cases as L
import nttmul
from oracle import oracle as O
from test_gpu_lifetime import STATUS, Run, torch_cuda  # noqa: F401

pytestmark = pytest.mark.gpu

HIP_ERROR = {L.ENOMEM: nttmul.HIP_ERROR_OUT_OF_MEMORY, L.EINVAL: nttmul.HIP_ERROR_INVALID_VALUE,
             None: 0}
STATUS_CODE = {"ENOMEM": nttmul.NTTMUL_ENOMEM, "EHIP": nttmul.NTTMUL_EHIP}
# the runtime call each site stands in for, as HIP_TRY's text names it
SITE_CALL = {"BOX_ALLOC": "hipHostMalloc(", "REQ_ALLOC": "hipHostMalloc(",
             "BOX_MAP": "hipHostGetDevicePointer(", "REQ_MAP": "hipHostGetDevicePointer(",
             "STREAM": "hipStreamCreateWithFlags(", "LAUNCH": "launch_server("}


class FailRun(Run):
    """Run over a sequence of SERVER_SEQUENCES: the model is walked step by step beside the
    calls, with what the machine did about the request half's placement (req_in_vram)."""

    def execute(self):
        ctx, cp = self.ctx, self.cp
        st = L.new_state(cp)
        in_vram, err_before = True, b""
        assert ctx.server_status() == (0, "") and ctx.diag_server_state()["go"] == 0
        self.trace = []
        for i, (step, io) in enumerate(zip(self.steps, self.io)):
            where = (self.name, i, step)
            for site, error, skip in step.arm:
                ctx.diag_server_failpoint(site, HIP_ERROR[error], skip)
            status = self._host_call(step, io)
            dev = ctx.diag_server_state()
            if not st["server"]["allocated"]:
                in_vram = bool(dev["req_in_vram"])
            w = L.walk(cp, st, step, in_vram)
            self.trace.append(w)
            st, S = w.state, w.state["server"]
            # the call
            assert STATUS.get(status, status) == step.status, where
            err = ctx._lib.nttmul_last_error(ctx._h)
            if step.status == "ERANGE":
                assert b"coefficient >= q" in err, where
            elif any(t.startswith("server.unavailable") for t in w.tags):
                assert err == b"", (where, err)      # the call itself succeeded
            else:
                assert err == err_before, (where, err)
            err_before = err
            assert ctx.last_host_path() == st["last_path"], where
            self._check_last_product(st["last_prod"], where)
            # the status pair
            failures, reason = ctx.server_status()
            assert failures == S["failures"] == dev["failures"], (where, failures, reason)
            if S["reason"] is None:
                assert reason == "", (where, reason)
            else:
                k, code, retry, site = S["reason"]
                assert reason.startswith(f"failure {k} ({nttmul.strerror(STATUS_CODE[code])}): "), \
                    (where, reason)
                assert SITE_CALL[site] in reason, (where, reason)
                tail = f"; retried after {L.RETRY_CALLS} calls" if retry else "; launch path from now on"
                assert reason.endswith(tail), (where, reason)
            # the state, and the two invariants
            assert dev["go"] == dev["served"], (where, dev)
            pair = 2 if S["allocated"] else 0
            assert (dev["box_pair"], dev["req_pair"]) == (pair, pair), (where, dev)
            if pair:
                assert dev["done"] == dev["served"] and dev["req_in_vram"] == int(in_vram), (where, dev)
            assert dev["running"] == int(S["running"]), (where, dev)
            assert dev["cooldown"] == S["cooldown"], (where, dev)
            assert dev["small_server"] == (-1 if S["disabled"] else 0), (where, dev)
            if S["served"]:
                assert dev["served"] & 0xFF == S["last_batch"] and dev["served"] >> 8 <= dev["seq"], \
                    (where, dev)
            else:
                assert dev["served"] == 0, (where, dev)
            # launches: the model's, plus one for every stop the host's idle margin added (the
            # time between two calls decides those); relaunches in the spin loop exactly
            assert dev["spin_relaunches"] == S["spin"], (where, dev)
            extra = dev["stops"] - S["stops"]
            assert extra >= 0 and dev["launches"] == S["launches"] + extra, (where, dev, S)


def _run(torch, name, salt):
    run = FailRun(torch, name, salt)
    run.prepare()
    try:
        run.execute()
        run.verify()
    finally:
        torch.cuda.synchronize()
        run.close()
    return run


@pytest.mark.parametrize("name", [n for n in L.SERVER_SEQUENCES if not n.startswith("S6")])
def test_server_failure_sequence(name, torch_cuda):
    """S1 the relaunch inside the spin loop; S2 a relaunch refused in the middle of a request,
    the cool-down and the retry, at the three server kernels' sizes; S3 the cap; S4 an error that
    is not out of memory; S5 a setup that fails at each of its runtime calls."""
    run = _run(torch_cuda, name, salt=20000 + 1000 * list(L.SERVER_SEQUENCES).index(name))
    S = run.trace[-1].state["server"]
    if name == "S1":
        assert S["spin"] == 2 and S["failures"] == 0 and all(w.path == 3 for w in run.trace)
    if name.startswith("S2") or name.startswith("S5"):
        assert run.trace[-1].path == 3 and run.trace[-2].path == 3 and not S["disabled"]
    if name in ("S3", "S4"):
        assert S["disabled"] and all(w.path != 3 for w in run.trace)
        assert S["failures"] == (L.MAX_FAILURES if name == "S3" else 1)


@pytest.mark.parametrize("name", ["S6_cool", "S6_off"])
def test_destroy_after_failure_then_a_fresh_context_serves(name, torch_cuda):
    """S6: nttmul_destroy on a context in cool-down (its mailbox allocated, its kernel gone) and
    on one switched to the launch path for good after a setup that was rolled back; a fresh
    context on the same device then serves, exactly."""
    run = _run(torch_cuda, name, salt=40000)
    S = run.trace[-1].state["server"]
    assert (S["cooldown"] > 0, S["disabled"]) == ((True, False) if name == "S6_cool" else (False, True))
    fresh = _run(torch_cuda, "S6_fresh", salt=41000)
    assert [w.path for w in fresh.trace] == [3, 3]
    assert fresh.trace[-1].state["server"]["failures"] == 0


# ---------------------------------------------------------------------------------------------
# The compat shims from several threads (production libnttmul.so)
# ---------------------------------------------------------------------------------------------

THREADS, CALLS = 8, 100
PRODUCTS = ("ntt256_product4", "ntt_red256_product1")
# NTT/ntt256.h:20-69: two cyclic and two negacyclic wrappers -> (ntt.C loop, ntt256 table)
WRAPPERS = {"ntt256_ct_std2rev": ("ntt_ct_std2rev", "omega_powers_rev"),
            "intt256_gs_rev2std": ("ntt_gs_rev2std", "inv_omega_powers_rev"),
            "mulntt256_ct_std2rev": ("mulntt_ct_std2rev", "mixed_powers_rev"),
            "inttmul256_gs_rev2std": ("nttmul_gs_rev2std", "inv_mixed_powers_rev")}
SENTINEL = np.int32(-1)


def _shim_plan(golden_dir, k):
    """Thread k's calls, in its own seeded order: (entry, inputs, expected).  Products take the
    reference's coefficient files (expected: the compiled reference's, tests/golden/ref256.npz) or
    random polynomials below 12289 (the oracle's product); wrappers take rows of the reference's
    wrapper fixture (expected: ref256_wrappers.npz) or random polynomials (the oracle's loop)."""
    g = np.load(os.path.join(golden_dir, "ref256.npz"))
    gw = np.load(os.path.join(golden_dir, "ref256_wrappers.npz"))
    fa = nttmul.read_coefficients(os.path.join(golden_dir, "coeficientes_a.txt"), 256)
    fb = nttmul.read_coefficients(os.path.join(golden_dir, "coeficientes_b.txt"), 256)
    assert np.array_equal(fa, g["a"][0]) and np.array_equal(fb, g["b"][0])
    P = O.Plan(256, D.Q0, 1002)
    rng = np.random.default_rng(9000 + k)
    names = PRODUCTS + tuple(WRAPPERS)
    plan = []
    for _ in range(CALLS):
        name = names[rng.integers(len(names))]
        fixture = rng.integers(4) == 0
        if name in PRODUCTS:
            if fixture:
                a, b, exp = fa, fb, g[name][0]
            else:
                a, b = rng.integers(0, D.Q0, 256), rng.integers(0, D.Q0, 256)
                exp = P.product4(a, b)
            plan.append((name, (a.astype(np.int32), b.astype(np.int32)), exp.astype(np.int32)))
        else:
            if fixture:
                row = rng.integers(len(gw["x"]))
                x, exp = gw["x"][row], gw[name][row]
            else:
                x = rng.integers(0, D.Q0, 256)
                fn, table = WRAPPERS[name]
                exp = P.transform(fn, x.astype(np.uint64), table)
            plan.append((name, (x.astype(np.int32),), np.asarray(exp).astype(np.int32)))
    return plan


def test_compat_shims_from_eight_threads(golden_dir, torch_cuda):
    """Eight host threads, started together, each 100 calls over ntt256_product4,
    ntt_red256_product1 and four of the transform wrappers in an order of its own: the shims
    share the library's two n = 256 contexts (and the resident server behind the products), so
    every call must still see its own operands and get its own result.  Each thread has buffers
    of its own, preset to a sentinel, and every result is compared bit for bit."""
    plans = [_shim_plan(golden_dir, k) for k in range(THREADS)]
    assert {p[0] for plan in plans for p in plan} == set(PRODUCTS) | set(WRAPPERS)
    barrier, errors = threading.Barrier(THREADS), [None] * THREADS

    def body(k):
        try:
            a, b, c = (np.empty(256, dtype=np.int32) for _ in range(3))
            barrier.wait(timeout=60)
            for i, (name, ins, exp) in enumerate(plans[k]):
                if name in PRODUCTS:
                    a[:], b[:], c[:] = ins[0], ins[1], SENTINEL
                    getattr(nttmul, name)(c, a, b)
                    assert np.array_equal(a, ins[0]) and np.array_equal(b, ins[1]), (k, i, name)
                    assert np.array_equal(c, exp), (k, i, name)
                else:
                    a[:] = ins[0]
                    nttmul.ntt256_transform(name, a)
                    assert np.array_equal(a, exp), (k, i, name)
        except BaseException as e:          # noqa: BLE001 (re-raised by the main thread)
            errors[k] = e
            barrier.abort()
    threads = [threading.Thread(target=body, args=(k,)) for k in range(THREADS)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    torch_cuda.cuda.synchronize()
    for e in errors:
        if e is not None:
            raise e
