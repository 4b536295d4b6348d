"""lib/libnttmul_rns.so (include/nttmul_rns.h) without a GPU: the library is built, exports the
whole ABI of nttmul.h, nttmul_mac.h and nttmul_rns.h unmangled, leaves the two older libraries as
they were, and refuses bad arguments before any device access."""
import ctypes
import os
import subprocess

import pytest

import dispatch_cases as D
import nttmul
import rns_cases as R


def _defined(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True,
                         check=True).stdout
    return out, {line.split()[-1] for line in out.splitlines() if " T " in line}


def test_rns_library_is_built():
    assert os.path.exists(nttmul.RNS_LIB_PATH), f"{nttmul.RNS_LIB_PATH} not built"


def test_rns_library_exports_all_three_headers():
    _, have = _defined(nttmul.RNS_LIB_PATH)
    rns = nttmul.rns_exported_symbols()
    assert rns == sorted([
        "nttmul_rns_create", "nttmul_rns_destroy", "nttmul_rns_last_error", "nttmul_rns_get_info",
        "nttmul_rns_limb_info", "nttmul_rns_multiply_device", "nttmul_rns_forward_device",
        "nttmul_rns_inverse_device", "nttmul_rns_mac_ntt_device", "nttmul_rns_multiply",
        "nttmul_rns_forward", "nttmul_rns_inverse", "nttmul_rns_mac_ntt",
        "nttmul_rns_kernel_name"])
    want = set(nttmul.exported_symbols()) | set(nttmul.mac_exported_symbols()) | set(rns)
    assert len(want) > 55
    assert sorted(want - have) == []
    assert sorted(s for s in have if s.startswith("nttmul_rns_") and s not in rns) == []


@pytest.mark.parametrize("path", ["LIB_PATH", "MAC_LIB_PATH"])
def test_the_older_libraries_do_not_grow(path):
    """libnttmul.so and libnttmul_mac.so keep their ABI and kernels: the new entry points and the
    k_rns_* kernels are in the third library only."""
    out, _ = _defined(getattr(nttmul, path))
    assert "nttmul_rns" not in out and "k_rns" not in out
    assert not [k for k in nttmul.kernel_hashes(getattr(nttmul, path)) if "k_rns" in k]


def _params(n, flags=0, q=0, psi=0):
    return nttmul._Params(n, q, psi, 1, 0, flags, 0, 0, 0, 0, 0)


def _create(lib, n, moduli, flags=0, q=0, psi=0, limbs=None):
    h = ctypes.c_void_p()
    prm = _params(n, flags, q, psi)
    qs = (ctypes.c_uint64 * max(1, len(moduli)))(*moduli)
    st = lib.nttmul_rns_create(ctypes.byref(h), ctypes.byref(prm), ctypes.sizeof(prm), qs,
                               len(moduli) if limbs is None else limbs)
    if st == nttmul.NTTMUL_OK:      # (only where a device is present)
        lib.nttmul_rns_destroy(h)
    else:
        assert not h.value
    return st


def test_create_refusals_come_before_any_device_access():
    lib = nttmul.load_rns_library()
    EINVAL, EUNS = nttmul.NTTMUL_EINVAL, nttmul.NTTMUL_EUNSUPPORTED
    n = 1024
    assert _create(lib, n, R.BASIS32, limbs=0) == EINVAL
    many = list(range(3, 3 + nttmul.RNS_MAX_LIMBS + 1))
    assert _create(lib, n, many) == EINVAL                                   # above the maximum
    assert _create(lib, n, (D.Q31, D.Q31 + 2)) == EINVAL                     # not prime
    assert _create(lib, 4096, (D.Q31, D.Q0)) == EINVAL                       # 2n does not divide q - 1
    assert _create(lib, n, (D.Q31, (1 << 62) + 1)) == EINVAL                 # q >= 2^62
    assert _create(lib, 1000, R.BASIS32) == EINVAL                           # n not a power of two
    assert _create(lib, 128, R.BASIS32) == EINVAL
    assert _create(lib, n, (D.Q31, D.Q31HI, D.Q31)) == EINVAL                # two equal primes
    assert _create(lib, n, R.BASIS32, q=D.Q31) == EINVAL                     # params->q
    assert _create(lib, n, R.BASIS32, psi=3) == EINVAL                       # params->psi
    assert _create(lib, 8192, R.BASIS32) == EUNS                             # a valid n above 4096
    assert _create(lib, 65536, R.BASIS64[:1]) == EUNS
    assert _create(lib, n, R.BASIS32, flags=nttmul.NTTMUL_FLAG_CYCLIC) == EUNS
    assert _create(lib, n, (D.Q31, D.Q62)) == EUNS                           # mixed classes
    assert _create(lib, n, (D.Q62, D.Q31)) == EUNS
    assert _create(lib, n, (D.Q32,)) == EUNS                                 # [2^31, 2^32)
    assert _create(lib, n, (D.Q31, D.Q32)) == EUNS
    h = ctypes.c_void_p()
    prm = _params(n)
    qs = (ctypes.c_uint64 * 1)(D.Q31)
    assert lib.nttmul_rns_create(None, ctypes.byref(prm), ctypes.sizeof(prm), qs, 1) == EINVAL
    assert lib.nttmul_rns_create(ctypes.byref(h), None, ctypes.sizeof(prm), qs, 1) == EINVAL
    assert lib.nttmul_rns_create(ctypes.byref(h), ctypes.byref(prm), 4, qs, 1) == EINVAL
    assert lib.nttmul_rns_create(ctypes.byref(h), ctypes.byref(prm), ctypes.sizeof(prm), None, 1) == EINVAL
    # an invalid modulus is EINVAL even where the context would be unsupported anyway
    assert _create(lib, 8192, (D.Q31, D.Q31 + 2)) == EINVAL


def test_call_refusals_come_before_any_device_access():
    lib = nttmul.load_rns_library()
    EINVAL = nttmul.NTTMUL_EINVAL
    one = (ctypes.c_uint32 * 1)()
    p = ctypes.addressof(one)
    assert lib.nttmul_rns_multiply_device(None, p, p, p, 1, 0, None) == EINVAL
    assert lib.nttmul_rns_multiply_device(None, None, None, None, 0, 0, None) == EINVAL
    assert lib.nttmul_rns_forward_device(None, p, p, 1, 0, None) == EINVAL
    assert lib.nttmul_rns_inverse_device(None, p, p, 1, 0, None) == EINVAL
    assert lib.nttmul_rns_mac_ntt_device(None, p, p, p, 1, 1, 0, 0, None) == EINVAL
    assert lib.nttmul_rns_mac_ntt_device(None, p, p, p, 1, 0, 0, 0, None) == EINVAL
    assert lib.nttmul_rns_multiply(None, p, p, p, 1) == EINVAL
    assert lib.nttmul_rns_forward(None, p, p, 1) == EINVAL
    assert lib.nttmul_rns_inverse(None, p, p, 1) == EINVAL
    assert lib.nttmul_rns_mac_ntt(None, p, p, p, 1, 0, 1) == EINVAL
    buf = ctypes.create_string_buffer(64)
    assert lib.nttmul_rns_kernel_name(None, 0, buf, len(buf)) == EINVAL
    assert lib.nttmul_rns_get_info(None, None) == EINVAL
    assert lib.nttmul_rns_limb_info(None, 0, None) == EINVAL
    assert lib.nttmul_rns_last_error(None) == b""
    lib.nttmul_rns_destroy(None)


def test_rns_context_is_its_own_class_on_its_own_library():
    for name in ("multiply_device", "forward_device", "inverse_device", "mac_ntt_device",
                 "multiply", "forward", "inverse", "mac_ntt", "kernel_name", "limb_info"):
        assert callable(getattr(nttmul.RnsContext, name))
    assert not issubclass(nttmul.RnsContext, nttmul.Context)
    # three separate images: loading one does not rebind the others
    libs = (nttmul.load_library(), nttmul.load_mac_library(), nttmul.load_rns_library())
    assert len({id(x) for x in libs}) == 3
    assert [x._name for x in libs] == [nttmul.LIB_PATH, nttmul.MAC_LIB_PATH, nttmul.RNS_LIB_PATH]
    assert not hasattr(nttmul.load_mac_library(), "nttmul_rns_create")


def test_python_refuses_what_the_library_refuses():
    with pytest.raises(nttmul.NttmulError) as ei:
        nttmul.RnsContext(1024, (D.Q31, D.Q31))
    assert ei.value.status == nttmul.NTTMUL_EINVAL
    with pytest.raises(nttmul.NttmulError) as ei:
        nttmul.RnsContext(1024, ())
    assert ei.value.status == nttmul.NTTMUL_EINVAL
    with pytest.raises(nttmul.NttmulError) as ei:
        nttmul.RnsContext(16384, R.BASIS32)
    assert ei.value.status == nttmul.NTTMUL_EUNSUPPORTED
    with pytest.raises(nttmul.NttmulError) as ei:
        nttmul.RnsContext(1024, R.BASIS32, cyclic=True)
    assert ei.value.status == nttmul.NTTMUL_EUNSUPPORTED


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="checks the no-GPU behaviour")
def test_rns_context_without_a_device_fails_loudly():
    with pytest.raises(nttmul.NttmulError) as ei:
        nttmul.RnsContext(4096, R.BASIS32)
    assert ei.value.status == nttmul.NTTMUL_ENODEV
