"""What a call does to the caller's memory: footprint, alignment and aliasing of every entry point
that writes caller memory, on all four libraries.

Every operand of every call lives in a guarded arena (tests/guarded.py): one allocation laid out
[guard][operand][guard]...[guard], all words preset to the all-ones sentinel, every operand at an
address aligned to its word and to nothing larger.  Each case is checked three ways: the result
against the CPU reference its library's parity test uses (the oracle, tests/bconv_ref.py, plain
contexts per limb), bit for bit in the caller's word, and with arena.check(): no guard word
changed, no input changed, no output word left unwritten.

The cases are the Footprint rows of tests/dispatch_cases.py, mac_cases.py, rns_cases.py and
bconv_cases.py; groups() below deals them out to the tests, and tests/test_footprint_ledger.py
(no GPU) holds that every row is dealt exactly once, that every exported entry point has a row and
that every multi-unit kernel has a row with a partial last workgroup."""
import functools

import numpy as np
import pytest

import bconv_cases as B
import bconv_ref
import dispatch_cases as D
import guarded as G
import mac_cases as M
import nttmul
import rns_cases as R
from oracle import oracle as O
from test_gpu_parity import _oracle_batch, _xf_expected, torch_cuda  # noqa: F401

pytestmark = pytest.mark.gpu

HOST_PATH = {"staged": 0, "direct": 1, "zero_copy": 2, "server": 3}
FILL_P0 = 5


# ---------------------------------------------------------------------------------------------
# The deal: which test runs which Footprint rows
# ---------------------------------------------------------------------------------------------

def _plain(f):
    return not (f.host or f.alias or f.scratch_mb or f.case.validate)


def groups():
    """{test name: {parameter: [Footprint rows]}} over the four tables."""
    out = {k: {} for k in ("device", "subbatch", "validate", "in_place", "host", "mac", "rns",
                           "bconv")}
    for f in D.footprint_cases():
        c = f.case
        if f.host:
            key, param = "host", f.host
        elif f.scratch_mb:
            key, param = "subbatch", (c.n, c.q, c.word_bits, c.batch)
        elif c.validate:
            key, param = "validate", (c.n, c.q, c.word_bits)
        elif f.alias:
            key, param = "in_place", (c.n, c.q, f.cyclic)
        else:
            key, param = "device", (c.n, c.q, f.cyclic)
        out[key].setdefault(param, []).append(f)
    for f in M.footprint_cases():
        out["mac"].setdefault((f.case.n, f.case.q), []).append(f)
    for f in R.footprint_cases():
        out["rns"].setdefault((f.case.n, R.word_bits(f.case.moduli)), []).append(f)
    for f in B.footprint_cases():
        out["bconv"].setdefault((f.case.bits, f.case.op), []).append(f)
    return out


GROUPS = groups()


def _params(key):
    return pytest.mark.parametrize("param", list(GROUPS[key]), ids=str)


# ---------------------------------------------------------------------------------------------
# References, computed once per (n, q, cyclic, batch) and shared by every row that needs them
# ---------------------------------------------------------------------------------------------

def _mulmod(x, y, q):
    return ((x.astype(object) * y.astype(object)) % q).astype(np.uint64)


def _xf_rows(P, x, mode, cyclic, n, q):
    """The oracle's transform of every row of x: the unscaled loop, and n^-1 in Python integers
    for the scaled inverse."""
    inv = mode & nttmul.XF_INVERSE
    rows = np.stack([_xf_expected(P, r, mode | (nttmul.XF_UNSCALED if inv else 0), cyclic, n, q)
                     for r in x])
    if inv and not mode & nttmul.XF_UNSCALED:
        rows = _mulmod(rows, np.full(1, pow(n, q - 2, q), dtype=np.uint64), q)
    return rows


class _Ref:
    """Inputs (the oracle's counter-based fill; row 1 all q - 1, the last row x^(n-1)) and the
    oracle's results for them.  A batch of b uses the first b rows."""

    def __init__(self, n, q, cyclic, batch):
        self.n, self.q, self.cyclic, self.batch = n, q, cyclic, batch
        self.P = O.Plan(n, q)
        self.x, self.y = O.fill_inputs(n, q, 21, batch)
        if batch > 2:
            self.x[1] = q - 1
            self.y[1] = q - 1
            self.x[batch - 1] = 0
            self.x[batch - 1, n - 1] = 1
        for a in (self.x, self.y):
            a.setflags(write=False)
        self._xf = {}

    def xf(self, mode, rows=None):
        if rows is not None:
            return _xf_rows(self.P, rows, mode, self.cyclic, self.n, self.q)
        if mode not in self._xf:
            self._xf[mode] = _xf_rows(self.P, self.x, mode, self.cyclic, self.n, self.q)
        return self._xf[mode]

    @functools.cached_property
    def pointwise(self):
        return _mulmod(self.x, self.y, self.q)

    @functools.cached_property
    def product(self):
        if not self.cyclic:
            return _oracle_batch(self.P, self.q, self.x, self.y).reshape(self.batch, self.n)
        # x^n - 1: the oracle's cyclic transforms around a product in Python integers
        hat = _mulmod(self.xf(0), self.xf(0, self.y), self.q)
        return self.xf(3, hat)

    @functools.cached_property
    def fill(self):
        return O.fill_inputs(self.n, self.q, FILL_P0, self.batch)


@functools.lru_cache(maxsize=4)
def _ref(n, q, cyclic, batch):
    return _Ref(n, q, cyclic, batch)


def _context(n, q, cyclic, **kw):
    return nttmul.Context(n, q, psi=O.Plan(n, q).omega if cyclic else 0, cyclic=cyclic, **kw)


def _same(got, want, dt, what):
    """Bit for bit, in the caller's word."""
    assert got.dtype == dt, what
    want = np.ascontiguousarray(want)
    assert want.max() <= np.iinfo(dt).max
    bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1).astype(dt))
    assert bad.size == 0, (what, f"{bad.size} words differ, first at {bad[0]}")


def _strip_prio(keys):
    return [k.replace(",true>", ">").replace(",false>", ">") for k in keys]


# ---------------------------------------------------------------------------------------------
# libnttmul: one Footprint row on the device
# ---------------------------------------------------------------------------------------------

def _run_device(torch, ctx, f, ref):
    """Runs f on ctx out of a DeviceArena and checks it; returns the result rows."""
    c = f.case
    n, bits, batch = c.n, c.word_bits, c.batch
    dt = G.dtype_of(bits)
    guard = D.fp_guard_words(c)
    x, y = ref.x[:batch], ref.y[:batch]
    s = torch.cuda.current_stream().cuda_stream
    if c.op == "fill":
        assert f.entry == "nttmul_fill_random_device"
        arena = G.DeviceArena(torch, bits, guard, a=batch * n, b=batch * n)
        ctx.fill_random_device(arena["a"], arena["b"], FILL_P0, batch, bits, stream=s)
        out, want = ("a", "b"), (ref.fill[0][:batch], ref.fill[1][:batch])
    elif c.op == "multiply":
        assert f.entry == "nttmul_multiply_batch_device" and not f.alias
        arena = G.DeviceArena(torch, bits, guard, c=batch * n, a=x, b=y)
        ctx.multiply_device(arena["c"], arena["a"], arena["b"], batch, bits, stream=s)
        assert _strip_prio(nttmul.dispatch_key(k) for k in ctx.last_kernel_name().split("+")) == \
            _strip_prio(D.product_keys(c))
        out, want = ("c",), (ref.product[:batch],)
    elif c.op == "pointwise":
        assert f.entry == "nttmul_pointwise_batch_device"
        if f.alias:
            over = f.alias[-1]                                   # "c=a" / "c=b"
            arena = G.DeviceArena(torch, bits, guard, inplace=(over,), a=x, b=y)
            cbuf = arena[over]
        else:
            arena = G.DeviceArena(torch, bits, guard, c=batch * n, a=x, b=y)
            cbuf, over = arena["c"], "c"
        ctx.pointwise_device(cbuf, arena["a"], arena["b"], batch, bits, stream=s)
        out, want = (over,), (ref.pointwise[:batch],)
    else:
        assert c.op == "transform"
        if f.alias:
            assert f.alias == "out=in"
            arena = G.DeviceArena(torch, bits, guard, inplace=("x",), x=x)
            obuf, out = arena["x"], ("x",)
        else:
            arena = G.DeviceArena(torch, bits, guard, out=batch * n, x=x)
            obuf, out = arena["out"], ("out",)
        if f.entry == "nttmul_forward_batch_device":
            assert c.mode == 0
            ctx.forward_device(obuf, arena["x"], batch, bits, stream=s)
        elif f.entry == "nttmul_inverse_batch_device":
            assert c.mode == 3
            ctx.inverse_device(obuf, arena["x"], batch, bits, stream=s)
        else:
            assert f.entry == "nttmul_transform_device"
            ctx.transform_device(obuf, arena["x"], c.mode, batch, bits, stream=s)
        want = (ref.xf(c.mode)[:batch],)
    torch.cuda.synchronize()
    arena.check()
    got = [arena.get(name, (batch, n)) for name in out]
    for g, w, name in zip(got, want, out):
        _same(g, w, dt, (f, name))
    return got[0]


@_params("device")
def test_device_entry_points(param, torch_cuda):
    """multiply, forward, inverse, pointwise, transform in all six modes and fill_random, at every
    size, one modulus per arithmetic class in every word width, batch 1 and 33 (1 and 3 above
    n = 4096); negacyclic everywhere, cyclic at three sizes."""
    n, q, cyclic = param
    rows = GROUPS["device"][param]
    ref = _ref(n, q, cyclic, max(f.case.batch for f in rows))
    with _context(n, q, cyclic) as ctx:
        for f in rows:
            _run_device(torch_cuda, ctx, f, ref)


@_params("subbatch")
def test_sub_batched_calls(param, torch_cuda):
    """scratch_mb = 1: the product and the reordered transforms run in sub-batches through the
    scratch (32 + 32 + 1 and 2 + 2 + 1 polynomials), out of place and, the transforms in all six
    modes, in place."""
    n, q, bits, batch = param
    ref = _ref(n, q, False, batch)
    with _context(n, q, False, scratch_mb=1) as ctx:
        for f in GROUPS["subbatch"][param]:
            assert f.scratch_mb == 1 and f.case.batch == batch
            _run_device(torch_cuda, ctx, f, ref)


@_params("validate")
def test_validated_calls_read_no_guard_word(param, torch_cuda):
    """NTTMUL_FLAG_VALIDATE: every guard word is >= q, so a range check that read one would
    answer NTTMUL_ERANGE; the calls return OK (and are exact)."""
    n, q, bits = param
    rows = GROUPS["validate"][param]
    assert G.sentinel(bits) >= q
    ref = _ref(n, q, False, max(f.case.batch for f in rows))
    with _context(n, q, False, validate=True) as ctx:
        for f in rows:
            _run_device(torch_cuda, ctx, f, ref)


@_params("in_place")
def test_in_place(param, torch_cuda):
    """transform_device with out is in in all six modes, pointwise_device with c is a and c is b:
    the oracle's result, and the out-of-place result of the same call."""
    n, q, cyclic = param
    rows = GROUPS["in_place"][param]
    ref = _ref(n, q, cyclic, max(f.case.batch for f in rows))
    with _context(n, q, cyclic) as ctx:
        for f in rows:
            got = _run_device(torch_cuda, ctx, f, ref)
            apart = _run_device(torch_cuda, ctx, f._replace(alias=""), ref)
            assert np.array_equal(got, apart), f


# ---------------------------------------------------------------------------------------------
# libnttmul: host buffers, every host path
# ---------------------------------------------------------------------------------------------

def _run_host(ctx, f, ref, pinned):
    c = f.case
    n, bits, batch = c.n, c.word_bits, c.batch
    dt = G.dtype_of(bits)
    guard = D.fp_guard_words(c)
    x, y = ref.x[:batch], ref.y[:batch]
    fn = getattr(ctx._lib, f.entry)
    assert f.entry.endswith(f"_u{bits}")
    if c.op in ("multiply", "pointwise"):
        out = "a" if f.alias == "c=a" else "c"
        operands = dict(a=x, b=y) if f.alias else dict(c=batch * n, a=x, b=y)
        arena = G.HostArena(bits, guard, pinned=pinned, inplace=(out,) if f.alias else (), **operands)
        args = [arena[k].ctypes.data for k in (out, "a", "b")]
        if f.entry.startswith("nttmul_multiply_u"):            # the one-polynomial entry point
            assert batch == 1
            ctx._check(fn(ctx._h, *args))
        else:
            ctx._check(fn(ctx._h, *args, batch))
        want = (ref.product if c.op == "multiply" else ref.pointwise)[:batch]
    else:
        out = "x" if f.alias == "out=in" else "out"
        operands = dict(x=x) if f.alias else dict(out=batch * n, x=x)
        arena = G.HostArena(bits, guard, pinned=pinned, inplace=(out,) if f.alias else (), **operands)
        args = [arena[k].ctypes.data for k in (out, "x")]
        if f.entry.startswith("nttmul_transform_batch"):
            ctx._check(fn(ctx._h, c.mode, *args, batch))
        else:
            assert f.entry.startswith(f"nttmul_{'inverse' if c.mode else 'forward'}_batch")
            ctx._check(fn(ctx._h, *args, batch))
        want = ref.xf(c.mode)[:batch]
    assert f.alias in ("", "c=a", "out=in")
    assert ctx.last_host_path() == HOST_PATH[f.host], (f, ctx.last_host_path())
    arena.check()
    _same(arena.get(out, (batch, n)), want, dt, f)


@_params("host")
def test_host_buffer_entry_points(param, torch_cuda):
    """The host-buffer forms out of a HostArena through each of the four host paths
    (nttmul_last_host_path): staged through the pinned buffers (pageable memory, zero_copy_kb =
    -1; one batch large enough for the staging copy to split into unequal pieces), direct DMA
    (the arena in page-locked memory), zero-copy on the staging buffers (the default knob, small
    chunks) and the resident server; on the first three also a transform in place and a pointwise
    product over its first factor."""
    rows = GROUPS["host"][param]
    knobs = {"zero_copy_kb": -1} if param == "staged" else {}
    shapes = []
    for f in rows:
        key = (f.case.n, f.case.q)
        if key not in shapes:
            shapes.append(key)
    for n, q in shapes:
        mine = [f for f in rows if (f.case.n, f.case.q) == (n, q)]
        ref = _ref(n, q, False, max(f.case.batch for f in mine))
        with _context(n, q, False, **knobs) as ctx:
            for f in mine:
                _run_host(ctx, f, ref, pinned=param == "direct")
            if param == "server":
                assert ctx.server_status()[0] == 0


# ---------------------------------------------------------------------------------------------
# libnttmul_mac
# ---------------------------------------------------------------------------------------------

def _sum_mod(rows, q):
    acc = rows[0].astype(object)
    for r in rows[1:]:
        acc = acc + r.astype(object)
    return (acc % q).astype(np.uint64)


@_params("mac")
def test_mac(param, torch_cuda):
    """nttmul_mac_ntt_device and the host forms: terms 3, batch 1 and 33, shared and per-batch
    b_hat = forward(b), against the sum of the oracle's products."""
    torch = torch_cuda
    n, q = param
    rows = GROUPS["mac"][param]
    B_, T = max(f.case.batch for f in rows), M.FP_TERMS
    P = O.Plan(n, q)
    a, b = O.fill_inputs(n, q, 40, B_ * T)
    a, b = a.reshape(B_, T, n), b.reshape(B_, T, n)
    shared_b = np.ascontiguousarray(np.broadcast_to(b[0], b.shape))
    want = {s: _sum_mod([_oracle_batch(P, q, np.ascontiguousarray(a[:, t]),
                                       np.ascontiguousarray((shared_b if s else b)[:, t]))
                         .reshape(B_, n) for t in range(T)], q) for s in (False, True)}
    with nttmul.MacContext(n, q) as ctx:
        b_hat = {}
        for f in rows:
            c = f.case
            bits, batch, dt = c.word_bits, c.batch, G.dtype_of(c.word_bits)
            assert c.terms == T
            if bits not in b_hat:
                b_hat[bits] = ctx.forward(b.reshape(-1, n), dtype=dt).reshape(b.shape)
            bh = b_hat[bits][0] if c.shared else b_hat[bits][:batch]
            operands = dict(c=batch * n, a=a[:batch], b_hat=bh)
            guard = M.fp_guard_words(c)
            if f.host:
                arena = G.HostArena(bits, guard, **operands)
                fn = getattr(ctx._lib, f.entry)
                ctx._check(fn(ctx._h, *(arena[k].ctypes.data for k in ("c", "a", "b_hat")),
                              batch, T, int(c.shared)))
            else:
                assert f.entry == "nttmul_mac_ntt_device"
                arena = G.DeviceArena(torch, bits, guard, **operands)
                ctx.mac_ntt_device(arena["c"], arena["a"], arena["b_hat"], batch, T, bits,
                                   shared=c.shared,
                                   stream=torch.cuda.current_stream().cuda_stream)
                torch.cuda.synchronize()
            arena.check()
            _same(arena.get("c", (batch, n)), want[c.shared][:batch], dt, f)


# ---------------------------------------------------------------------------------------------
# libnttmul_rns
# ---------------------------------------------------------------------------------------------

@_params("rns")
def test_rns(param, torch_cuda):
    """Product, both transforms (also in place) and the mac over [batch][3][n] operands, batch 1
    and 33, and the host forms: products against the oracle per limb, transforms against plain
    contexts per limb."""
    torch = torch_cuda
    n, bits = param
    rows = GROUPS["rns"][param]
    moduli = rows[0].case.moduli
    L, T = len(moduli), R.FP_TERMS
    B_ = max(f.case.batch for f in rows)
    dt = G.dtype_of(bits)
    per = [O.fill_inputs(n, q, 40, B_ * T) for q in moduli]
    a = np.ascontiguousarray(np.stack([p[0].reshape(B_, T, n) for p in per], axis=2))
    b = np.ascontiguousarray(np.stack([p[1].reshape(B_, T, n) for p in per], axis=2))
    plans = [O.Plan(n, q) for q in moduli]

    def products(shared):
        """[B_, T, L, n]: the oracle's a[p][t][l] * b[shared ? 0 : p][t][l]."""
        return np.stack([np.stack([
            _oracle_batch(plans[l], q, np.ascontiguousarray(a[:, t, l]), np.ascontiguousarray(
                np.broadcast_to(b[0, t, l], (B_, n)) if shared else b[:, t, l])).reshape(B_, n)
            for l, q in enumerate(moduli)], axis=1) for t in range(T)], axis=1)

    prod = {s: products(s) for s in (False, True)}
    mac = {s: np.stack([_sum_mod([prod[s][:, t, l] for t in range(T)], q)
                        for l, q in enumerate(moduli)], axis=1) for s in (False, True)}
    plain = [nttmul.Context(n, q) for q in moduli]

    def per_limb(op, x):
        flat = x.reshape(-1, L, n)
        out = np.stack([getattr(plain[l], op)(np.ascontiguousarray(flat[:, l]), dtype=dt)
                        for l in range(L)], axis=1)
        return out.reshape(x.shape).astype(np.uint64)

    fwd, inv, b_hat = per_limb("forward", a[:, 0]), per_limb("inverse", a[:, 0]), per_limb("forward", b)
    with nttmul.RnsContext(n, moduli) as ctx:
        assert ctx.word_bits == bits
        for f in rows:
            c = f.case
            assert c.moduli == moduli and f.entry == R.ENTRY[c.op] + ("" if f.host else "_device")
            batch, words = c.batch, c.batch * L * n
            guard = R.fp_guard_words(c)
            if c.op == "mac":
                assert c.terms == T
                operands = dict(c=words, a=a[:batch], b=b_hat[0] if c.shared else b_hat[:batch])
                want, out = mac[c.shared][:batch], "c"
            elif c.op == "multiply":
                operands = dict(c=words, a=a[:batch, 0], b=b[:batch, 0])
                want, out = prod[False][:batch, 0], "c"
            else:
                operands = dict(out=words, x=a[:batch, 0])
                want, out = (fwd if c.op == "forward" else inv)[:batch], "out"
            inplace = ()
            if f.alias:
                assert f.alias == "out=in" and c.op in ("forward", "inverse")
                del operands["out"]
                inplace, out = ("x",), "x"
            if f.host:
                arena = G.HostArena(bits, guard, **operands)
                ptr = lambda k: arena[k].ctypes.data                           # noqa: E731
            else:
                arena = G.DeviceArena(torch, bits, guard, inplace=inplace, **operands)
                ptr = lambda k: arena[k]                                       # noqa: E731
            if f.host:
                fn = getattr(ctx._lib, f.entry)
                if c.op == "mac":
                    ctx._check(fn(ctx._h, ptr("c"), ptr("a"), ptr("b"), batch, T, int(c.shared)))
                elif c.op == "multiply":
                    ctx._check(fn(ctx._h, ptr("c"), ptr("a"), ptr("b"), batch))
                else:
                    ctx._check(fn(ctx._h, ptr("out"), ptr("x"), batch))
            else:
                s = torch.cuda.current_stream().cuda_stream
                if c.op == "mac":
                    ctx.mac_ntt_device(ptr("c"), ptr("a"), ptr("b"), batch, T, shared=c.shared,
                                       stream=s)
                elif c.op == "multiply":
                    ctx.multiply_device(ptr("c"), ptr("a"), ptr("b"), batch, stream=s)
                else:
                    getattr(ctx, f"{c.op}_device")(ptr(out), ptr("x"), batch, stream=s)
                torch.cuda.synchronize()
            arena.check()
            _same(arena.get(out, (batch, L, n)), want, dt, f)
    for p in plain:
        p.close()


# ---------------------------------------------------------------------------------------------
# libnttmul_bconv
# ---------------------------------------------------------------------------------------------

@_params("bconv")
def test_bconv(param, torch_cuda):
    """convert and moddown on both word sizes against tests/bconv_ref.py: n = 256 with batch 1 and
    5, n = 4096 with batch 1, (L, K) = (3, 2) and (1, 5), and the host forms."""
    torch = torch_cuda
    bits, op = param
    dt = G.dtype_of(bits)
    ref = bconv_ref.convert if op == "convert" else bconv_ref.moddown
    for f in GROUPS["bconv"][param]:
        c = f.case
        assert f.entry == f"nttmul_bconv_{op}" + ("" if f.host else "_device")
        from_q, to_q = B.bases(bits, c.L, c.K)
        moduli = from_q if op == "convert" else to_q + from_q
        x = bconv_ref.random_words(np.random.default_rng(1000 * c.n + 10 * c.L + c.K), moduli,
                                   c.batch, c.n, dt)
        guard = B.fp_guard_words(c)
        with nttmul.BaseConverter(c.n, from_q, to_q) as conv:
            if f.host:
                arena = G.HostArena(bits, guard, out=c.batch * c.K * c.n, x=x)
                fn = getattr(conv._lib, f.entry)
                conv._check(fn(conv._h, arena["out"].ctypes.data, arena["x"].ctypes.data, c.batch))
            else:
                arena = G.DeviceArena(torch, bits, guard, out=c.batch * c.K * c.n, x=x)
                getattr(conv, f"{op}_device")(arena["out"], arena["x"], c.batch,
                                              stream=torch.cuda.current_stream().cuda_stream)
                torch.cuda.synchronize()
        arena.check()
        _same(arena.get("out", (c.batch, c.K, c.n)), ref(x, from_q, to_q), dt, f)
