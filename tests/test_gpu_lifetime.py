"""Long-lived contexts: the call sequences of tests/lifetime_cases.py, each on one context from
its first call to its last.

What makes a stale buffer, a missed ordering or a lost copy visible:

* every step draws inputs no earlier step of its sequence used (counter positions of its own);
* every output buffer holds the sentinel (all bits set, no canonical value) before the sequence
  starts, host outputs inside guarded arenas (tests/guarded.py);
* every result is compared bit for bit with the oracle, and every input with its copy, after the
  sequence: device steps are enqueued with no host synchronisation between them and checked after
  the one synchronise at the end, so the library's own ordering is what is under test;
* after every step nttmul_last_host_path and nttmul_last_kernel_name must say what the model of
  lifetime_cases.py derived from the state before the step.

Contexts are closed only after the final synchronise (include/nttmul.h: nttmul_destroy does not
wait for the caller's streams).
"""
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import bconv_ref as BR
import dispatch_cases as D
import guarded as G
import lifetime_cases as L
import nttmul
import rns_cases as R
from oracle import oracle as O

pytestmark = pytest.mark.gpu

STATUS = {nttmul.NTTMUL_OK: "OK", nttmul.NTTMUL_ERANGE: "ERANGE"}
# oracle loops of the four (direction, order) pairs, negacyclic (test_gpu_parity._xf_expected)
XF_LOOPS = {0: ("mulntt_ct_std2rev", "mixed_powers_rev"), 2: ("mulntt_ct_rev2std", "mixed_powers"),
            1: ("nttmul_gs_std2rev", "inv_mixed_powers"), 3: ("nttmul_gs_rev2std", "inv_mixed_powers_rev")}


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _udt(bits):
    return np.uint32 if bits == 32 else np.uint64


def _mulmod(x, y, q):
    """x * y mod q for canonical uint64 arrays (y may be a Python integer)."""
    if q < (1 << 32):               # the product of two residues fits 64 bits
        return x * np.asarray(y, dtype=np.uint64) % np.uint64(q)
    return ((x.astype(object) * np.asarray(y).astype(object)) % q).astype(np.uint64)


def _oracle_products(P, q, a, b):
    """Row by row a * b mod (x^n + 1, q): the oracle's whole-batch product."""
    if q < (1 << 31):
        return P.fast_batch_u32(a.astype(np.uint32), b.astype(np.uint32))[0].astype(np.uint64)
    return P.product_batch(a, b)[0]


def _oracle_transforms(P, x, mode):
    """The oracle's loop of `mode` over every row of x (uint64 [rows, n])."""
    fn, tab = XF_LOOPS[mode & 3]
    with ThreadPoolExecutor(max(1, min(16, len(x)))) as ex:
        y = np.stack(list(ex.map(lambda row: P.transform(fn, row, tab), x)))
    if mode & nttmul.XF_INVERSE and not mode & nttmul.XF_UNSCALED:
        y = _mulmod(y, pow(P.n, P.q - 2, P.q), P.q)
    return y


def _to_device(torch, x, bits):
    x = np.ascontiguousarray(x, dtype=_udt(bits)).reshape(-1)
    return torch.from_numpy(x.view(np.int32 if bits == 32 else np.int64)).cuda()


def _from_device(t, bits):
    return t.cpu().numpy().view(_udt(bits)).astype(np.uint64)


class Run:
    """One sequence on one context: prepare() builds the context and every step's operands,
    execute() makes the calls, verify() compares everything the calls left behind."""

    def __init__(self, torch, name, salt):
        self.torch, self.name, self.salt = torch, name, salt
        self.cp, self.steps = L.ALL_SEQUENCES[name]
        self.trace = L.model(name)
        self.cus = torch.cuda.get_device_properties(0).multi_processor_count

    # ---- operands -----------------------------------------------------------------------------

    def prepare(self):
        torch, cp = self.torch, self.cp
        cls = nttmul.MacContext if cp.lib == "mac" else nttmul.Context
        lib = {"_lib": nttmul.load_diag_library()} if cp.lib == "diag" else {}
        self.ctx = cls(cp.n, cp.q, scratch_mb=cp.scratch_mb, validate=cp.validate, ndev=cp.ndev,
                       share_devices=cp.share_devices, **lib)
        self.P = O.Plan(cp.n, cp.q)
        self.streams = {"A": torch.cuda.Stream(), "B": torch.cuda.Stream()}
        self.io, p0 = [], self.salt
        for step in self.steps:
            polys = step.batch * max(1, step.terms)
            self.io.append(self._operands(step, p0, polys))
            p0 += polys
        torch.cuda.synchronize()

    def _operands(self, step, p0, polys):
        torch, n, q, bits = self.torch, self.cp.n, self.cp.q, step.bits
        op = L.op_of(step)
        if step.entry == "shim256":
            n, q = 256, D.Q0
        a, b = O.fill_inputs(n, q, p0, polys)
        io = {"p0": p0, "a": a, "b": b}
        if step.status == "ERANGE":
            a[step.bad, 5] = q
        if step.entry == "mac":
            # b_hat: the forward transform of b, as the oracle computes it
            io["b_hat"] = _oracle_transforms(self.P, b, 0)
        ins = {"a": a}
        if op in ("multiply", "pointwise"):
            ins["b"] = b
        elif op == "mac":
            ins["b"] = io["b_hat"]
        if step.entry == "fill":
            ins = {}
        outs = ("a", "b") if step.entry == "fill" else ("c",)
        out_words = step.batch * n
        if step.place in L.HOST_PLACES:
            io["arena"] = G.HostArena(bits, G.guard_words(n * max(1, step.terms)),
                                      pinned=step.place == "pinned", **ins, c=out_words)
        else:
            io["dev"] = {k: _to_device(torch, v, bits) for k, v in ins.items()}
            dt = torch.int32 if bits == 32 else torch.int64
            for k in outs:
                io["dev"][k] = torch.full((out_words,), -1, dtype=dt, device="cuda")
        return io

    # ---- calls --------------------------------------------------------------------------------

    def _host_call(self, step, io):
        lib, h, ar = self.ctx._lib, self.ctx._h, io["arena"]
        w, ptr = f"u{step.bits}", lambda k: ar[k].ctypes.data
        if step.entry == "multiply":
            return getattr(lib, f"nttmul_multiply_batch_{w}")(h, ptr("c"), ptr("a"), ptr("b"), step.batch)
        if step.entry == "multiply_one":
            return getattr(lib, f"nttmul_multiply_{w}")(h, ptr("c"), ptr("a"), ptr("b"))
        if step.entry == "pointwise":
            return getattr(lib, f"nttmul_pointwise_batch_{w}")(h, ptr("c"), ptr("a"), ptr("b"), step.batch)
        if step.entry in ("forward", "inverse"):
            return getattr(lib, f"nttmul_{step.entry}_batch_{w}")(h, ptr("c"), ptr("a"), step.batch)
        if step.entry == "transform":
            return getattr(lib, f"nttmul_transform_batch_{w}")(h, step.mode, ptr("c"), ptr("a"), step.batch)
        if step.entry == "mac":
            return getattr(lib, f"nttmul_mac_ntt_{w}")(h, ptr("c"), ptr("a"), ptr("b"), step.batch,
                                                       step.terms, 0)
        assert step.entry == "shim256"
        nttmul.ntt256_product1(*(ar[k].view(np.int32) for k in ("c", "a", "b")))
        return nttmul.NTTMUL_OK

    def _device_call(self, step, io):
        ctx, t, bits, batch = self.ctx, io["dev"], step.bits, step.batch
        s = 0 if step.place == "null" else self.streams[step.place].cuda_stream
        try:
            if step.entry == "multiply":
                ctx.multiply_device(t["c"], t["a"], t["b"], batch, bits, stream=s)
            elif step.entry == "pointwise":
                ctx.pointwise_device(t["c"], t["a"], t["b"], batch, bits, stream=s)
            elif step.entry == "forward":
                ctx.forward_device(t["c"], t["a"], batch, bits, stream=s)
            elif step.entry == "inverse":
                ctx.inverse_device(t["c"], t["a"], batch, bits, stream=s)
            elif step.entry == "transform":
                ctx.transform_device(t["c"], t["a"], step.mode, batch, bits, stream=s)
            elif step.entry == "mac":
                ctx.mac_ntt_device(t["c"], t["a"], t["b"], batch, step.terms, bits, stream=s)
            else:
                assert step.entry == "fill"
                ctx.fill_random_device(t["a"], t["b"], io["p0"], batch, bits, stream=s)
        except nttmul.NttmulError as e:
            return e.status
        return nttmul.NTTMUL_OK

    def execute(self):
        for i, (step, io, w) in enumerate(zip(self.steps, self.io, self.trace)):
            host = step.place in L.HOST_PLACES
            st = self._host_call(step, io) if host else self._device_call(step, io)
            where = (self.name, i, step)
            assert STATUS.get(st, st) == step.status, where
            if step.status == "ERANGE":
                assert b"coefficient >= q" in self.ctx._lib.nttmul_last_error(self.ctx._h), where
            assert self.ctx.last_host_path() == w.state["last_path"], where
            if self.cp.ndev == 1:       # (slices note their products from their own threads)
                self._check_last_product(w.state["last_prod"], where)
        self.torch.cuda.synchronize()

    def _check_last_product(self, last, where):
        name = self.ctx.last_kernel_name()
        if last is None:
            assert name == "", where
            return
        batch, bits, prio_ok = last
        case = D.Case("multiply", self.cp.n, self.cp.q, bits, batch, prio_ok=prio_ok)
        assert [nttmul.dispatch_key(k) for k in name.split("+")] == D.product_keys(case, self.cus), where

    # ---- results ------------------------------------------------------------------------------

    def _expected(self, step, io):
        n, q, P = self.cp.n, self.cp.q, self.P
        a, b, op = io["a"], io["b"], L.op_of(step)
        if step.entry == "shim256":
            return O.Plan(256, D.Q0).product_merged(a[0], b[0])[None]
        if op == "multiply":
            return _oracle_products(P, q, a, b)
        if op == "pointwise":
            return _mulmod(a, b, q)
        if op == "transform":
            return _oracle_transforms(P, a, L.mode_of(step))
        assert op == "mac" and q < (1 << 31)
        prods = _oracle_products(P, q, a, b).reshape(step.batch, step.terms, n)
        return prods.sum(axis=1) % np.uint64(q)

    def verify(self):
        for i, (step, io) in enumerate(zip(self.steps, self.io)):
            where = (self.name, i, step)
            failed = step.status != "OK"
            n = 256 if step.entry == "shim256" else self.cp.n
            if "arena" in io:
                try:
                    io["arena"].check()         # guards, inputs unchanged, every output word written
                except G.GuardError as e:
                    # (nothing is promised about c after a failed call)
                    if not (failed and e.kind == "output not written"):
                        raise AssertionError(f"{where}: {e}") from e
                got = {"c": io["arena"].get("c", (step.batch, n)).astype(np.uint64)}
            else:
                got = {k: _from_device(t, step.bits).reshape(-1, n) for k, t in io["dev"].items()}
                ins = () if step.entry == "fill" else ("a", "b") if "b" in got else ("a",)
                for k in ins:
                    want = io["b_hat"] if (k == "b" and step.entry == "mac") else io[k]
                    assert np.array_equal(got[k], want), (where, "input changed", k)
            if failed:
                continue
            if step.entry == "fill":
                want = {"a": io["a"], "b": io["b"]}
            else:
                want = {"c": self._expected(step, io)}
            for k, exp in want.items():
                bad = np.flatnonzero((got[k] != exp).any(axis=1))
                assert bad.size == 0, (where, k, f"{bad.size} rows differ, first {bad[:4]}")

    def close(self):
        self.ctx.close()


@pytest.mark.parametrize("name", list(L.SEQUENCES))
def test_sequence(name, torch_cuda):
    """One sequence, one context, one thread."""
    run = Run(torch_cuda, name, salt=1000)
    run.prepare()
    try:
        run.execute()
        run.verify()
    finally:
        torch_cuda.cuda.synchronize()
        run.close()


@pytest.mark.parametrize("pair", L.THREAD_PAIRS, ids="+".join)
def test_two_threads_two_contexts(pair, torch_cuda):
    """Two host threads, a context and caller streams each, started together: "separate contexts
    are independent" (include/nttmul.h).  The second pair both copy through the process-wide
    CopyPool.  Each thread checks its own results and keeps its own exception."""
    runs = [Run(torch_cuda, name, salt=5000 + 100000 * k) for k, name in enumerate(pair)]
    for r in runs:
        r.prepare()
    barrier, errors = threading.Barrier(len(runs)), [None] * len(runs)

    def body(k):
        try:
            barrier.wait(timeout=60)
            runs[k].execute()
            runs[k].verify()
        except BaseException as e:          # noqa: BLE001 (reported by the main thread)
            errors[k] = e
            barrier.abort()
    threads = [threading.Thread(target=body, args=(k,)) for k in range(len(runs))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    torch_cuda.cuda.synchronize()
    for r in runs:
        r.close()
    for name, e in zip(pair, errors):
        if e is not None:
            raise AssertionError(f"thread of sequence {name}: {e!r}") from e


def test_one_stream_through_the_four_libraries(torch_cuda):
    """libnttmul.so fills, libnttmul_rns.so transforms and multiplies-accumulates, and
    libnttmul_bconv.so converts and ModDowns, all on one caller stream with no synchronisation
    between the calls, each output the next call's input: stream order alone carries the data
    from one library's kernels to the next's.  Every stage is compared after the one synchronise."""
    torch = torch_cuda
    n, batch, terms = L.CHAIN
    Bq = R.BASIS32
    Cq = tuple(p for p in BR.primes_below(1 << 31, BR.STEP, 8) if p not in Bq)[:2]
    Lb, K = len(Bq), len(Cq)
    fill_q = min(Bq)                    # canonical for every limb
    p0, count = 777, batch * terms * Lb
    plain = nttmul.Context(n, fill_q)
    rns = nttmul.RnsContext(n, Bq)
    conv = nttmul.BaseConverter(n, Bq, Cq)
    assert rns.word_bits == conv.word_bits == 32

    def empty(polys):
        return torch.full((polys * n,), -1, dtype=torch.int32, device="cuda")
    a, key, a_hat, key_hat = empty(count), empty(count), empty(count), empty(terms * Lb)
    c, cv, x, md = empty(batch * Lb), empty(batch * K), empty(batch * (K + Lb)), empty(batch * K)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    s = stream.cuda_stream
    plain.fill_random_device(a, key, p0, count, 32, stream=s)
    rns.forward_device(a_hat, a, batch * terms, stream=s)
    rns.forward_device(key_hat, key, terms, stream=s)
    rns.mac_ntt_device(c, a_hat, key_hat, batch, terms, shared=True, stream=s)
    conv.convert_device(cv, c, batch, stream=s)
    with torch.cuda.stream(stream):     # [batch][K + L][n]: the converted limbs, then limbs of B
        xv = x.view(batch, K + Lb, n)
        xv[:, :K].copy_(cv.view(batch, K, n))
        xv[:, K:].copy_(a_hat.view(batch, terms, Lb, n)[:, 0])
    conv.moddown_device(md, x, batch, stream=s)
    torch.cuda.synchronize()

    ea, ek = O.fill_inputs(n, fill_q, p0, count)
    ea, ek = ea.reshape(batch, terms, Lb, n), ek[:terms * Lb].reshape(terms, Lb, n)
    plans = [O.Plan(n, q) for q in Bq]
    ea_hat, ek_hat, ec = np.empty_like(ea), np.empty_like(ek), np.empty((batch, Lb, n), np.uint64)
    for l, (q, P) in enumerate(zip(Bq, plans)):
        ea_hat[:, :, l] = _oracle_transforms(P, ea[:, :, l].reshape(-1, n), 0).reshape(batch, terms, n)
        ek_hat[:, l] = _oracle_transforms(P, ek[:, l], 0)
        # INTT(sum_t NTT(a_hat_t) o NTT(key_t)) = sum_t a_hat_t * key_t
        left = ea_hat[:, :, l].reshape(-1, n)
        right = np.broadcast_to(ek[:, l], (batch, terms, n)).reshape(-1, n)
        ec[:, l] = _oracle_products(P, q, left, right).reshape(batch, terms, n).sum(axis=1) % np.uint64(q)
    ecv = BR.convert(ec.astype(np.uint32), Bq, Cq).astype(np.uint64)
    ex = np.concatenate([ecv, ea_hat[:, 0]], axis=1)
    emd = BR.moddown(ex.astype(np.uint32), Bq, Cq).astype(np.uint64)
    stages = [("fill a", a, ea), ("fill key", key[:terms * Lb * n], ek), ("forward a", a_hat, ea_hat),
              ("forward key", key_hat, ek_hat), ("mac", c, ec), ("convert", cv, ecv),
              ("assembled", x, ex), ("moddown", md, emd)]
    for what, got, want in stages:
        assert np.array_equal(_from_device(got, 32).reshape(want.shape), want), what
    assert emd.any()
    for ctx in (plain, rns, conv):
        ctx.close()
