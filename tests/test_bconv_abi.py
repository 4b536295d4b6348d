"""lib/libnttmul_bconv.so (include/nttmul_bconv.h) without a GPU: the library is built, exports the
whole ABI of the four headers unmangled, leaves the three older libraries as they were, refuses bad
arguments before any device access, and its host planner (nttmul_bconv_plan) returns the constants
of tests/bconv_ref.py."""
import ctypes
import functools
import os
import subprocess

import pytest

import bconv_ref as R
import dispatch_cases as D
import nttmul


@functools.lru_cache(maxsize=None)
def _primes(bits):
    """Primes just below the top of a class (in a test's body: nttmul.is_prime loads the library,
    and no module of the suite loads one while it is collected)."""
    return tuple(R.primes_below(1 << bits, R.STEP, 20))


def _defined(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True,
                         check=True).stdout
    return out, {line.split()[-1] for line in out.splitlines() if " T " in line}


def test_bconv_library_is_built():
    assert os.path.exists(nttmul.BCONV_LIB_PATH), f"{nttmul.BCONV_LIB_PATH} not built"


def test_bconv_library_exports_all_four_headers():
    _, have = _defined(nttmul.BCONV_LIB_PATH)
    bconv = nttmul.bconv_exported_symbols()
    assert bconv == sorted([
        "nttmul_bconv_create", "nttmul_bconv_destroy", "nttmul_bconv_last_error",
        "nttmul_bconv_get_info", "nttmul_bconv_plan", "nttmul_bconv_convert_device",
        "nttmul_bconv_moddown_device", "nttmul_bconv_convert", "nttmul_bconv_moddown",
        "nttmul_bconv_kernel_name"])
    want = (set(nttmul.exported_symbols()) | set(nttmul.mac_exported_symbols())
            | set(nttmul.rns_exported_symbols()) | set(bconv))
    assert len(want) > 65
    assert sorted(want - have) == []
    assert sorted(s for s in have if s.startswith("nttmul_bconv_") and s not in bconv) == []
    assert not [s for s in bconv if s.startswith("nttmul_rns_")]


@pytest.mark.parametrize("path", ["LIB_PATH", "MAC_LIB_PATH", "RNS_LIB_PATH"])
def test_the_older_libraries_do_not_grow(path):
    out, _ = _defined(getattr(nttmul, path))
    assert "nttmul_bconv" not in out and "k_bconv" not in out
    assert not [k for k in nttmul.kernel_hashes(getattr(nttmul, path)) if "k_bconv" in k]


def _params(n, flags=0, q=0, psi=0):
    return nttmul._Params(n, q, psi, 1, 0, flags, 0, 0, 0, 0, 0)


def _arr(values):
    return (ctypes.c_uint64 * max(1, len(values)))(*values)


def _both(n, from_q, to_q, flags=0, q=0, psi=0, L=None, K=None):
    """The status of nttmul_bconv_plan and of nttmul_bconv_create for the same arguments: equal
    wherever the planner refuses; where it accepts, create goes on to look for a device."""
    lib = nttmul.load_bconv_library()
    prm = _params(n, flags, q, psi)
    L = len(from_q) if L is None else L
    K = len(to_q) if K is None else K
    inv, w, binv = _arr([0] * 64), _arr([0] * 64 * 64), _arr([0] * 64)
    st = lib.nttmul_bconv_plan(ctypes.byref(prm), ctypes.sizeof(prm), _arr(from_q), L, _arr(to_q),
                               K, inv, w, binv)
    h = ctypes.c_void_p()
    created = lib.nttmul_bconv_create(ctypes.byref(h), ctypes.byref(prm), ctypes.sizeof(prm),
                                      _arr(from_q), L, _arr(to_q), K)
    if created == nttmul.NTTMUL_OK:      # (only where a device is present)
        lib.nttmul_bconv_destroy(h)
    else:
        assert not h.value
    if st != nttmul.NTTMUL_OK:
        assert created == st
    else:
        assert created in (nttmul.NTTMUL_OK, nttmul.NTTMUL_ENODEV)
    return st


def test_refusals_come_before_any_device_access():
    EINVAL, EUNS, OK = nttmul.NTTMUL_EINVAL, nttmul.NTTMUL_EUNSUPPORTED, nttmul.NTTMUL_OK
    P32, P64 = _primes(31), _primes(62)
    n, f, t = 1024, P32[:3], P32[3:5]
    assert _both(n, f, t) == OK
    assert _both(n, f, t, L=0) == EINVAL and _both(n, f, t, K=0) == EINVAL
    many = list(range(3, 3 + nttmul.RNS_MAX_LIMBS + 1))
    assert _both(n, many, t) == EINVAL and _both(n, f, many) == EINVAL          # 65 limbs
    assert _both(n, (P32[0], P32[0] + 2), t) == EINVAL                           # composite
    assert _both(n, f, (P32[3] + 2,)) == EINVAL
    assert _both(4096, (D.Q31, D.Q0), t) == EINVAL                               # q != 1 mod 2n
    assert _both(4096, f, (D.Q0,)) == EINVAL
    assert _both(n, f, ((1 << 62) + 1,)) == EINVAL                               # q >= 2^62
    assert _both(1000, f, t) == EINVAL and _both(128, f, t) == EINVAL            # n
    assert _both(n, (P32[0], P32[1], P32[0]), t) == EINVAL                       # repeated in a basis
    assert _both(n, f, (P32[3], P32[3])) == EINVAL
    assert _both(n, f, (P32[3], P32[1])) == EINVAL                               # in both bases
    assert _both(n, f, t, q=D.Q31) == EINVAL and _both(n, f, t, psi=3) == EINVAL
    assert _both(n, f, P64[:2]) == EUNS and _both(n, P64[:2], t) == EUNS         # mixed classes
    assert _both(n, (P32[0], P64[0]), t) == EUNS
    assert _both(n, (D.Q32,), t) == EUNS and _both(n, f, (D.Q32,)) == EUNS       # [2^31, 2^32)
    wide = (D.Q31, D.Q31HI), (D.Q31LO,)                                          # 2^17 | q - 1
    assert _both(8192, *wide) == EUNS and _both(65536, *wide) == EUNS            # n above 4096
    assert _both(n, f, t, flags=nttmul.NTTMUL_FLAG_CYCLIC) == EUNS
    # an invalid modulus is EINVAL even where the converter would be unsupported anyway
    assert _both(8192, wide[0], (D.Q31LO + 2,)) == EINVAL
    assert _both(n, P64[:2], (P32[3] + 2,)) == EINVAL


def test_null_arguments():
    lib = nttmul.load_bconv_library()
    EINVAL = nttmul.NTTMUL_EINVAL
    P32 = _primes(31)
    prm, h = _params(1024), ctypes.c_void_p()
    size, f, t = ctypes.sizeof(prm), _arr(P32[:2]), _arr(P32[2:3])
    out = _arr([0] * 4)
    assert lib.nttmul_bconv_create(None, ctypes.byref(prm), size, f, 2, t, 1) == EINVAL
    assert lib.nttmul_bconv_create(ctypes.byref(h), None, size, f, 2, t, 1) == EINVAL
    assert lib.nttmul_bconv_create(ctypes.byref(h), ctypes.byref(prm), 4, f, 2, t, 1) == EINVAL
    assert lib.nttmul_bconv_create(ctypes.byref(h), ctypes.byref(prm), size, None, 2, t, 1) == EINVAL
    assert lib.nttmul_bconv_create(ctypes.byref(h), ctypes.byref(prm), size, f, 2, None, 1) == EINVAL
    assert not h.value
    plan = lib.nttmul_bconv_plan
    assert plan(None, size, f, 2, t, 1, out, out, out) == EINVAL
    assert plan(ctypes.byref(prm), 4, f, 2, t, 1, out, out, out) == EINVAL
    assert plan(ctypes.byref(prm), size, None, 2, t, 1, out, out, out) == EINVAL
    assert plan(ctypes.byref(prm), size, f, 2, None, 1, out, out, out) == EINVAL
    for k in range(3):
        args = [out, out, out]
        args[k] = None
        assert plan(ctypes.byref(prm), size, f, 2, t, 1, *args) == EINVAL
    one = (ctypes.c_uint32 * 1)()
    p = ctypes.addressof(one)
    for op in nttmul.BCONV_OPS:
        assert getattr(lib, f"nttmul_bconv_{op}_device")(None, p, p, 1, 0, None) == EINVAL
        assert getattr(lib, f"nttmul_bconv_{op}_device")(None, None, None, 0, 0, None) == EINVAL
        assert getattr(lib, f"nttmul_bconv_{op}")(None, p, p, 1) == EINVAL
    buf = ctypes.create_string_buffer(64)
    assert lib.nttmul_bconv_kernel_name(None, 0, buf, len(buf)) == EINVAL
    assert lib.nttmul_bconv_get_info(None, None) == EINVAL
    assert lib.nttmul_bconv_last_error(None) == b""
    lib.nttmul_bconv_destroy(None)


@pytest.mark.parametrize("bits,L,K", [
    (31, 5, 4),                   # a 32-bit pair at the top of the class
    (62, 17, 3),                  # a 64-bit pair just below 2^62
    (31, 1, 1), (62, 1, 1),       # L = 1 and K = 1
], ids=["u32_5to4", "u64_17to3", "u32_1to1", "u64_1to1"])
def test_plan_returns_the_reference_constants(bits, L, K):
    from_q, to_q = _primes(bits)[:L], _primes(bits)[L:L + K]
    assert nttmul.bconv_plan(256, from_q, to_q) == R.constants(from_q, to_q)


def test_plan_of_small_moduli():
    from_q, to_q = (7681, D.Q0), (D.Q20,)
    assert nttmul.bconv_plan(256, from_q, to_q) == R.constants(from_q, to_q)
    assert nttmul.bconv_plan(256, to_q, from_q) == R.constants(to_q, from_q)


def test_python_surface():
    for name in ("convert", "moddown", "convert_device", "moddown_device", "kernel_name", "close"):
        assert callable(getattr(nttmul.BaseConverter, name))
    assert isinstance(nttmul.BaseConverter.io_dtype, property)
    libs = (nttmul.load_library(), nttmul.load_mac_library(), nttmul.load_rns_library(),
            nttmul.load_bconv_library())
    assert len({id(x) for x in libs}) == 4
    assert libs[3]._name == nttmul.BCONV_LIB_PATH
    assert not hasattr(nttmul.load_rns_library(), "nttmul_bconv_create")
    P32, P64 = _primes(31), _primes(62)
    with pytest.raises(nttmul.NttmulError) as ei:
        nttmul.bconv_plan(1024, P32[:2], P32[1:3])
    assert ei.value.status == nttmul.NTTMUL_EINVAL
    with pytest.raises(nttmul.NttmulError) as ei:
        nttmul.BaseConverter(1024, P32[:2], P64[:1])
    assert ei.value.status == nttmul.NTTMUL_EUNSUPPORTED


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="checks the no-GPU behaviour")
def test_converter_without_a_device_fails_loudly():
    with pytest.raises(nttmul.NttmulError) as ei:
        nttmul.BaseConverter(4096, _primes(31)[:3], _primes(31)[3:5])
    assert ei.value.status == nttmul.NTTMUL_ENODEV
