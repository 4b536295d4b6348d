"""lib/libnttmul_rnsmp.so (include/nttmul_rnsmp.h) without a GPU: the library is built, exports the
whole ABI of nttmul.h, nttmul_mac.h, nttmul_rns.h, nttmul_bconv.h and nttmul_rnsmp.h unmangled, and
refuses bad arguments before any device access."""
import ctypes
import os
import subprocess

import pytest

import dispatch_cases as D
import nttmul
import rnsmp_cases as R


def _defined(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True,
                         check=True).stdout
    return out, {line.split()[-1] for line in out.splitlines() if " T " in line}


def test_rnsmp_library_is_built():
    assert os.path.exists(nttmul.RNSMP_LIB_PATH), f"{nttmul.RNSMP_LIB_PATH} not built"


def test_rnsmp_library_exports_all_five_headers():
    _, have = _defined(nttmul.RNSMP_LIB_PATH)
    mp = nttmul.rnsmp_exported_symbols()
    assert mp == sorted([
        "nttmul_rnsmp_create", "nttmul_rnsmp_destroy", "nttmul_rnsmp_last_error",
        "nttmul_rnsmp_get_info", "nttmul_rnsmp_limb_info", "nttmul_rnsmp_multiply_device",
        "nttmul_rnsmp_forward_device", "nttmul_rnsmp_inverse_device",
        "nttmul_rnsmp_mac_ntt_device", "nttmul_rnsmp_multiply", "nttmul_rnsmp_forward",
        "nttmul_rnsmp_inverse", "nttmul_rnsmp_mac_ntt", "nttmul_rnsmp_kernel_name"])
    want = (set(nttmul.exported_symbols()) | set(nttmul.mac_exported_symbols())
            | set(nttmul.rns_exported_symbols()) | set(nttmul.bconv_exported_symbols()) | set(mp))
    assert len(want) > 95
    assert sorted(want - have) == []
    assert sorted(s for s in have if s.startswith("nttmul_rnsmp_") and s not in mp) == []
    # the other headers' parsers do not pick the new names up
    assert not [s for s in nttmul.rns_exported_symbols() + nttmul.bconv_exported_symbols()
                if "rnsmp" in s]


def _params(n, flags=0, q=0, psi=0):
    return nttmul._Params(n, q, psi, 1, 0, flags, 0, 0, 0, 0, 0)


def _create(lib, n, moduli, flags=0, q=0, psi=0, limbs=None):
    h = ctypes.c_void_p()
    prm = _params(n, flags, q, psi)
    qs = (ctypes.c_uint64 * max(1, len(moduli)))(*moduli)
    st = lib.nttmul_rnsmp_create(ctypes.byref(h), ctypes.byref(prm), ctypes.sizeof(prm), qs,
                                 len(moduli) if limbs is None else limbs)
    if st == nttmul.NTTMUL_OK:      # (only where a device is present)
        lib.nttmul_rnsmp_destroy(h)
    else:
        assert not h.value
    return st


def test_create_refusals_come_before_any_device_access():
    lib = nttmul.load_rnsmp_library()
    EINVAL, EUNS = nttmul.NTTMUL_EINVAL, nttmul.NTTMUL_EUNSUPPORTED
    n = 8192
    assert _create(lib, n, R.BASIS32, limbs=0) == EINVAL
    many = list(range(3, 3 + nttmul.RNS_MAX_LIMBS + 1))
    assert _create(lib, n, many) == EINVAL                                   # above the maximum
    assert _create(lib, n, (D.Q31, D.Q31 + 2)) == EINVAL                     # not prime
    assert _create(lib, n, (D.Q31, D.Q0)) == EINVAL                          # 2n does not divide q - 1
    assert _create(lib, 65536, (D.Q31, 2305843009213554689)) == EINVAL       # 2^13 | q - 1 only
    assert _create(lib, n, (D.Q31, (1 << 62) + 1)) == EINVAL                 # q >= 2^62
    assert _create(lib, 10000, R.BASIS32) == EINVAL                          # n not a power of two
    assert _create(lib, 128, R.BASIS32) == EINVAL
    assert _create(lib, n, (D.Q31, D.Q31HI, D.Q31)) == EINVAL                # two equal primes
    assert _create(lib, n, R.BASIS32, q=D.Q31) == EINVAL                     # params->q
    assert _create(lib, n, R.BASIS32, psi=3) == EINVAL                       # params->psi
    for small in (256, 1024, 4096):                                          # nttmul_rns_*'s sizes
        assert _create(lib, small, R.BASIS32) == EUNS
        assert _create(lib, small, R.BASIS64[:1]) == EUNS
    assert _create(lib, 131072, (D.Q31,)) == EUNS                            # a valid n above 65536
    assert _create(lib, 131072, (D.Q62,)) == EUNS
    assert _create(lib, n, R.BASIS32, flags=nttmul.NTTMUL_FLAG_CYCLIC) == EUNS
    assert _create(lib, n, (D.Q31, D.Q62)) == EUNS                           # mixed classes
    assert _create(lib, n, (D.Q62, D.Q31)) == EUNS
    assert _create(lib, n, (D.Q32,)) == EUNS                                 # [2^31, 2^32)
    assert _create(lib, n, (D.Q31, D.Q32)) == EUNS
    h = ctypes.c_void_p()
    prm = _params(n)
    qs = (ctypes.c_uint64 * 1)(D.Q31)
    assert lib.nttmul_rnsmp_create(None, ctypes.byref(prm), ctypes.sizeof(prm), qs, 1) == EINVAL
    assert lib.nttmul_rnsmp_create(ctypes.byref(h), None, ctypes.sizeof(prm), qs, 1) == EINVAL
    assert lib.nttmul_rnsmp_create(ctypes.byref(h), ctypes.byref(prm), 4, qs, 1) == EINVAL
    assert lib.nttmul_rnsmp_create(ctypes.byref(h), ctypes.byref(prm), ctypes.sizeof(prm), None, 1) == EINVAL
    # an invalid modulus is EINVAL even where the context would be unsupported anyway
    assert _create(lib, 4096, (D.Q31, D.Q31 + 2)) == EINVAL
    assert _create(lib, 131072, (D.Q31, D.Q31HI)) == EINVAL                  # 2^17 | q - 1 only
    # libnttmul_rns.so's answer at these sizes is unchanged, from this library too
    h = ctypes.c_void_p()
    prm = _params(8192)
    qs = (ctypes.c_uint64 * 3)(*R.BASIS32)
    assert lib.nttmul_rns_create(ctypes.byref(h), ctypes.byref(prm), ctypes.sizeof(prm), qs, 3) == EUNS


def test_call_refusals_come_before_any_device_access():
    lib = nttmul.load_rnsmp_library()
    EINVAL = nttmul.NTTMUL_EINVAL
    one = (ctypes.c_uint32 * 1)()
    p = ctypes.addressof(one)
    assert lib.nttmul_rnsmp_multiply_device(None, p, p, p, 1, 0, None) == EINVAL
    assert lib.nttmul_rnsmp_multiply_device(None, None, None, None, 0, 0, None) == EINVAL
    assert lib.nttmul_rnsmp_forward_device(None, p, p, 1, 0, None) == EINVAL
    assert lib.nttmul_rnsmp_inverse_device(None, p, p, 1, 0, None) == EINVAL
    assert lib.nttmul_rnsmp_mac_ntt_device(None, p, p, p, 1, 1, 0, 0, None) == EINVAL
    assert lib.nttmul_rnsmp_mac_ntt_device(None, p, p, p, 1, 0, 0, 0, None) == EINVAL
    assert lib.nttmul_rnsmp_multiply(None, p, p, p, 1) == EINVAL
    assert lib.nttmul_rnsmp_forward(None, p, p, 1) == EINVAL
    assert lib.nttmul_rnsmp_inverse(None, p, p, 1) == EINVAL
    assert lib.nttmul_rnsmp_mac_ntt(None, p, p, p, 1, 0, 1) == EINVAL
    buf = ctypes.create_string_buffer(64)
    assert lib.nttmul_rnsmp_kernel_name(None, 0, buf, len(buf)) == EINVAL
    assert lib.nttmul_rnsmp_get_info(None, None) == EINVAL
    assert lib.nttmul_rnsmp_limb_info(None, 0, None) == EINVAL
    assert lib.nttmul_rnsmp_last_error(None) == b""
    lib.nttmul_rnsmp_destroy(None)


def test_rnsmp_context_is_its_own_class_on_its_own_library():
    for name in ("multiply_device", "forward_device", "inverse_device", "mac_ntt_device",
                 "multiply", "forward", "inverse", "mac_ntt", "kernel_name", "limb_info"):
        assert callable(getattr(nttmul.RnsMpContext, name))
    assert not issubclass(nttmul.RnsMpContext, (nttmul.Context, nttmul.RnsContext))
    assert not issubclass(nttmul.RnsContext, nttmul.RnsMpContext)
    # separate images: loading one does not rebind the others
    libs = (nttmul.load_library(), nttmul.load_mac_library(), nttmul.load_rns_library(),
            nttmul.load_bconv_library(), nttmul.load_rnsmp_library())
    assert len({id(x) for x in libs}) == 5
    assert [x._name for x in libs] == [nttmul.LIB_PATH, nttmul.MAC_LIB_PATH, nttmul.RNS_LIB_PATH,
                                       nttmul.BCONV_LIB_PATH, nttmul.RNSMP_LIB_PATH]
    assert not hasattr(nttmul.load_bconv_library(), "nttmul_rnsmp_create")
    assert not hasattr(nttmul.load_rns_library(), "nttmul_rnsmp_create")
    assert nttmul.RNSMP_N == R.RNSMP_N


def test_python_refuses_what_the_library_refuses():
    for moduli, status in (((D.Q31, D.Q31), nttmul.NTTMUL_EINVAL), ((), nttmul.NTTMUL_EINVAL),
                           ((D.Q31, D.Q62), nttmul.NTTMUL_EUNSUPPORTED),
                           ((D.Q32,), nttmul.NTTMUL_EUNSUPPORTED)):
        with pytest.raises(nttmul.NttmulError) as ei:
            nttmul.RnsMpContext(8192, moduli)
        assert ei.value.status == status
    for n in (4096, 131072):
        with pytest.raises(nttmul.NttmulError) as ei:
            nttmul.RnsMpContext(n, (D.Q31,))
        assert ei.value.status == nttmul.NTTMUL_EUNSUPPORTED
    with pytest.raises(nttmul.NttmulError) as ei:
        nttmul.RnsMpContext(8192, R.BASIS32, cyclic=True)
    assert ei.value.status == nttmul.NTTMUL_EUNSUPPORTED


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="checks the no-GPU behaviour")
def test_rnsmp_context_without_a_device_fails_loudly():
    with pytest.raises(nttmul.NttmulError) as ei:
        nttmul.RnsMpContext(8192, R.BASIS32)
    assert ei.value.status == nttmul.NTTMUL_ENODEV
