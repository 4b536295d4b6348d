"""Long-lived contexts of the limb-aware libraries: the call sequences of
tests/limb_lifetime_cases.py, each on one context from its first call to its last, through the
scratch state of csrc/rnsmp.cpp, mdntt.cpp, ksntt.cpp and xconv.cpp.  The rules are
tests/test_gpu_lifetime.py's:

* every step draws inputs no other step used;
* every output buffer holds the sentinel (all bits set, no canonical value) before the sequence
  starts, host outputs inside guarded arenas (tests/guarded.py);
* device steps are enqueued with no host synchronisation between them and checked after the one
  synchronise at the end, so the libraries' own ordering is what is under test;
* every result is compared bit for bit with a value computed before the sequence and never by
  the context under test, and every input with its copy;
* every status is the step's; after NTTMUL_ERANGE the output still holds the sentinel and
  last_error the range check's text.

Expected values: the CPU references of limb_lifetime_cases.expected, every output word at every n
(the oracle per limb for every rnsmp entry, exact integers for the key mac, tests/full_ref.py for
the conversions).  At n = 8192 what each library's own parity test compares beside it is held to
the same values before the sequence starts: the device compositions of test_gpu_mdntt.py and
test_gpu_ksntt.py through fresh contexts of other libraries, and for xconv the library's inverse
of the output against the reference arithmetic on the library's inverse of the input, on every
coefficient.

Contexts are closed only after the final synchronise: destroy does not wait for caller streams."""
import ctypes
import threading
import time

import numpy as np
import pytest

import guarded as G
import ksntt_ref
import limb_lifetime_cases as L
import mdntt_ref
import nttmul
import xconv_gpu as XG
import xconv_ref
from test_gpu_ksntt import _compose_modup
from test_gpu_mdntt import _compose as _compose_moddown

pytestmark = pytest.mark.gpu

STATUS = {nttmul.NTTMUL_OK: "OK", nttmul.NTTMUL_ERANGE: "ERANGE"}


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _context(cp, plain_ks=False):
    kw = dict(ndev=cp.ndev, validate=cp.validate, share_devices=cp.share_devices,
              scratch_mb=cp.scratch_mb)
    m = L.moduli_of(cp)
    if cp.lib == "rnsmp":
        return nttmul.RnsMpHoistContext(cp.n, m, **kw)
    q, p = m
    if cp.lib == "mdntt":
        return nttmul.NttModDown(cp.n, q, p, **kw)
    if cp.lib == "xconv":
        return nttmul.NttExactConv(cp.n, q, p, scale=cp.shape[2], **kw)
    cls = nttmul.NttKeySwitch if plain_ks else nttmul.NttLevelKeySwitch
    return cls(cp.n, q, p, cp.shape[2], **kw)


def _signed(bits):
    return np.int32 if bits == 32 else np.int64


def _to_device(torch, x, bits, dev=0):
    x = np.ascontiguousarray(x, dtype=G.dtype_of(bits)).reshape(-1)
    return torch.from_numpy(x.view(_signed(bits))).to(f"cuda:{dev}")


def _from_device(t, bits):
    return t.cpu().numpy().view(G.dtype_of(bits))


def _karr(ks):
    return (ctypes.c_uint32 * max(1, len(ks)))(*ks)


class Run:
    """One sequence on one context: prepare() builds the context, every step's operands and every
    expected value, execute() makes the calls, verify() compares everything the calls left."""

    def __init__(self, torch, name, salt):
        self.torch, self.name, self.salt = torch, name, salt
        self.cp, self.steps = L.MODEL_SEQUENCES[name]
        self.trace = L.model(name)

    # ---- operands and expected values -------------------------------------------------------

    def prepare(self):
        torch, cp = self.torch, self.cp
        self.ctx = _context(cp)
        assert self.ctx.info.ndev == cp.ndev and self.ctx.word_bits == cp.bits
        if cp.scratch_mb:
            assert self.ctx.info.scratch_mb == cp.scratch_mb
        devs = sorted({s.dev for s in self.steps})
        self.streams = {d: {k: torch.cuda.Stream(device=d) for k in "AB"} for d in devs}
        self.io = []
        for i, step in enumerate(self.steps):
            ins = L.inputs(self.name, i, self.salt)
            ops = L.device_operands(cp, step, ins)
            io = {"ops": ops, "want": L.expected(cp, step, ins), "shape": L.shapes(cp, step)[1]}
            self.io.append(io)
        self._compose()
        for step, io in zip(self.steps, self.io):
            self._place(step, io)
        for d in devs:
            torch.cuda.synchronize(d)

    def _compose(self):
        """Beside the CPU references, above n = 512: the device compositions the libraries' own
        parity tests keep, all steps of a kind in one batch.  They are held to the CPU reference
        here, before the sequence; for xconv verify() makes the second half."""
        torch, cp = self.torch, self.cp
        todo = [(s, io) for s, io in zip(self.steps, self.io)
                if s.status == "OK" and cp.n > 512 and cp.lib in ("mdntt", "ksntt", "xconv")
                and s.entry in ("moddown", "modup", "extend")]
        if not todo:
            return
        q, p = L.moduli_of(cp)
        for entry in sorted({s.entry for s, _ in todo}):
            group = [io for s, io in todo if s.entry == entry]
            x = np.concatenate([io["ops"]["a"] for io in group])
            if cp.lib == "mdntt":
                comp = _compose_moddown(torch, cp.n, q, p, x)
            elif cp.lib == "ksntt":
                comp = _compose_modup(torch, cp.n, q, p, cp.shape[2], x)
            else:
                with XG.ctx(cp.n)(cp.n, tuple(p) if entry == "extend" else tuple(q) + tuple(p)) as wide:
                    coef = wide.inverse(x)
                comp = getattr(xconv_ref, entry + "_coeff")(coef, q, p, cp.shape[2])
            at = 0
            for io in group:
                b = io["ops"]["a"].shape[0]
                if cp.lib == "xconv":
                    io["coef"] = comp[at:at + b]
                else:
                    assert np.array_equal(comp[at:at + b], io["want"]), (self.name, entry, "composition")
                at += b

    def _place(self, step, io):
        torch, bits = self.torch, self.cp.bits
        words = int(np.prod(io["shape"]))
        if step.place == "host":
            entry = [v.size // v.shape[0] for v in io["ops"].values()] + [words // step.batch]
            io["arena"] = G.HostArena(bits, G.guard_words(*entry), **io["ops"], c=words)
            return
        io["dev"] = {k: _to_device(torch, v, bits, step.dev) for k, v in io["ops"].items()}
        if step.entry == "inverse_inplace":
            io["dev"]["c"] = io["dev"].pop("a")
        else:
            io["dev"]["c"] = torch.full((words,), -1, dtype=torch.int32 if bits == 32 else torch.int64,
                                        device=f"cuda:{step.dev}")

    # ---- calls ------------------------------------------------------------------------------

    def _host_call(self, step, io):
        c, h, ar = self.ctx._c, self.ctx._h, io["arena"]
        ptr = lambda k: ar[k].ctypes.data                   # noqa: E731
        b, e = step.batch, step.entry
        if self.cp.lib == "rnsmp":
            if e == "multiply":
                return c.multiply(h, ptr("c"), ptr("a"), ptr("b"), b)
            if e in ("forward", "inverse"):
                return getattr(c, e)(h, ptr("c"), ptr("a"), b)
            if e == "mac":
                return c.mac_ntt(h, ptr("c"), ptr("a"), ptr("b"), b, step.terms, 0)
            if e == "macn":
                return c.macn_ntt(h, ptr("c"), ptr("a"), ptr("b"), b, step.terms, step.comps, 1)
            assert e == "hoist"
            return c.hoist_ntt(h, ptr("c"), ptr("a"), ptr("b"), _karr(L.ks_of(self.cp, step)),
                               step.rots, b, step.terms, step.comps)
        if e != "mac":                                      # moddown, extend, modup
            return getattr(c, e)(h, ptr("c"), ptr("a"), b)
        args = (h, ptr("c"), ptr("a"), ptr("b"), _karr(L.ks_of(self.cp, step)), step.rots, b,
                step.terms, step.comps)
        if step.view:
            return c.mac_view(*args, ctypes.byref(nttmul.LevelView(*step.view)))
        return c.mac(*args)

    def _device_call(self, step, io):
        ctx, t, b, e = self.ctx, io["dev"], step.batch, step.entry
        s = 0 if step.place == "null" else self.streams[step.dev][step.place].cuda_stream
        on = dict(dev=step.dev, stream=s)
        try:
            if e == "multiply":
                ctx.multiply_device(t["c"], t["a"], t["b"], b, **on)
            elif e == "forward":
                ctx.forward_device(t["c"], t["a"], b, **on)
            elif e == "inverse":
                ctx.inverse_device(t["c"], t["a"], b, **on)
            elif e == "inverse_inplace":
                ctx.inverse_device(t["c"], t["c"], b, **on)
            elif e == "macn":
                ctx.macn_ntt_device(t["c"], t["a"], t["b"], b, step.terms, step.comps, shared=True, **on)
            elif e == "hoist":
                ctx.hoist_ntt_device(t["c"], t["a"], t["b"], L.ks_of(self.cp, step), b, step.terms,
                                     step.comps, **on)
            elif e == "mac" and self.cp.lib == "rnsmp":
                ctx.mac_ntt_device(t["c"], t["a"], t["b"], b, step.terms, shared=False, **on)
            elif e == "mac":
                ctx.mac_device(t["c"], t["a"], t["b"], L.ks_of(self.cp, step), b, step.terms,
                               step.comps, view=step.view, **on)
            else:                                           # moddown, extend, modup
                getattr(ctx, e + "_device")(t["c"], t["a"], b, **on)
        except nttmul.NttmulError as err:
            return err.status
        return nttmul.NTTMUL_OK

    def execute(self):
        torch = self.torch
        for i, (step, io) in enumerate(zip(self.steps, self.io)):
            host = step.place == "host"
            st = self._host_call(step, io) if host else self._device_call(step, io)
            where = (self.name, i, step)
            assert STATUS.get(st, st) == step.status, where
            if step.status == "ERANGE":
                text = L.ERANGE_TEXT[self.cp.lib, self.cp.lib == "ksntt" and step.entry == "mac"]
                assert self.ctx._c.last_error(self.ctx._h).decode() == text, where
            assert torch.cuda.current_device() == 0, where
        for d in self.streams:
            torch.cuda.synchronize(d)

    # ---- results ----------------------------------------------------------------------------

    def verify(self):
        cp, bits = self.cp, self.cp.bits
        sentinel = G.dtype_of(bits)(G.sentinel(bits))
        low = None
        for i, (step, io) in enumerate(zip(self.steps, self.io)):
            where = (self.name, i, step)
            failed = step.status != "OK"
            if "arena" in io:
                try:
                    io["arena"].check()         # guards, inputs unchanged, every output word written
                except G.GuardError as e:
                    if not (failed and e.kind == "output not written"):
                        raise AssertionError(f"{where}: {e}") from e
                got = io["arena"].get("c", io["shape"])
            else:
                for k, t in io["dev"].items():
                    if k != "c":
                        assert np.array_equal(_from_device(t, bits), io["ops"][k].reshape(-1)), \
                            (where, "input changed", k)
                got = _from_device(io["dev"]["c"], bits).reshape(io["shape"])
            if failed:
                assert (got == sentinel).all(), (where, "output written by a failed call")
                continue
            want = io["want"]
            assert got.shape == want.shape and got.dtype == want.dtype, where
            rows = got.reshape(got.shape[0], -1) != want.reshape(want.shape[0], -1)
            bad = np.flatnonzero(rows.any(axis=1))
            assert bad.size == 0, (where, f"{bad.size} batch entries differ, first {bad[:4]}")
            if "coef" in io:                    # the composition's second half, every coefficient
                if low is None:
                    low = XG.ctx(cp.n)(cp.n, L.moduli_of(cp)[0])
                assert np.array_equal(low.inverse(got), io["coef"]), (where, "composition")
        if low is not None:
            low.close()

    def close(self):
        self.ctx.close()


def _run(torch, name):
    t0 = time.perf_counter()
    run = Run(torch, name, L.SALT)
    run.prepare()
    t1 = time.perf_counter()
    try:
        run.execute()
        t2 = time.perf_counter()
        run.verify()
    finally:
        torch.cuda.synchronize()
        run.close()
    print(f"limb lifetime {name}: prepare {t1 - t0:.2f} s, calls {t2 - t1:.2f} s, "
          f"verify {time.perf_counter() - t2:.2f} s")


@pytest.mark.parametrize("name", list(L.SEQUENCES))
def test_sequence(name, torch_cuda):
    """One sequence, one context, one thread."""
    _run(torch_cuda, name)


def test_calls_on_the_second_device_entry(torch_cuda):
    """G with device forms on device 1, operands allocated there while device 0 stays current:
    the second entry's own scratch, and the caller's device restored after every call."""
    if torch_cuda.cuda.device_count() < L.G_DEV1_DEVICES:
        pytest.skip("the dev = 1 steps of G need a second device")
    _run(torch_cuda, "G_dev1")


@pytest.mark.parametrize("pair", L.THREAD_PAIRS, ids="+".join)
def test_two_threads_two_contexts(pair, torch_cuda):
    """Two host threads, a limb context and caller streams each, started on a barrier.  Each
    thread checks its own results and keeps its own exception."""
    runs = [Run(torch_cuda, name, salt) for name, salt in zip(pair, L.THREAD_SALTS)]
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


def test_one_stream_through_modup_mac_and_moddown(torch_cuda):
    """CHAIN: three iterations of NttKeySwitch.modup -> mac -> NttModDown.moddown on one caller
    stream with no host synchronisation, batches 1, 5, 2, the same two contexts throughout, each
    output the next call's input.  Every stage of every iteration is compared with the
    Python-integer references after the one synchronise."""
    torch = torch_cuda
    cp = L.CHAIN_CTX["ks"]
    n, bits = cp.n, cp.bits
    q, p = L.moduli_of(cp)
    L_, K, alpha = cp.shape
    M, dn = L_ + K, L.CHAIN_MAC["terms"]
    ks = (L.CHAIN_K,)
    kn, md = _context(cp, plain_ks=True), _context(L.CHAIN_CTX["md"])
    assert kn.digits == dn and (md.q, md.p) == (kn.q, kn.p)
    stream = torch.cuda.Stream()
    its = []
    for it, b in enumerate(L.CHAIN_BATCHES):
        x = L.inputs("CHAIN_ks", 2 * it)["a"]
        key = L.inputs("CHAIN_ks", 2 * it + 1)["b"]
        assert x.shape == (b, L_, n) and key.shape == (1, 2, dn, M, n)
        full = lambda polys: torch.full((polys * n,), -1, dtype=torch.int32, device="cuda")  # noqa: E731
        its.append(dict(b=b, x=x, key=key, dx=_to_device(torch, x, bits), dkey=_to_device(torch, key, bits),
                        up=full(b * dn * M), c=full(b * 2 * M), out=full(b * 2 * L_)))
    torch.cuda.synchronize()
    s = stream.cuda_stream
    for v in its:
        kn.modup_device(v["up"], v["dx"], v["b"], stream=s)
        kn.mac_device(v["c"], v["up"], v["dkey"], ks, v["b"], dn, 2, stream=s)
        md.moddown_device(v["out"], v["c"], 2 * v["b"], stream=s)
    torch.cuda.synchronize()
    for it, v in enumerate(its):
        b = v["b"]
        up = ksntt_ref.modup(v["x"], q, p, alpha)
        c = ksntt_ref.mac(up, v["key"], ks, q + p)
        out = mdntt_ref.moddown(c.reshape(2 * b, M, n), q, p)
        assert np.array_equal(_from_device(v["dx"], bits), v["x"].reshape(-1)), it
        assert np.array_equal(_from_device(v["dkey"], bits), v["key"].reshape(-1)), it
        for what, got, want in (("modup", v["up"], up), ("mac", v["c"], c), ("moddown", v["out"], out)):
            assert np.array_equal(_from_device(got, bits).reshape(want.shape), want), (it, what)
        assert out.any()
    kn.close()
    md.close()
