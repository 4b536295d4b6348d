"""lib/libnttmul_galois.so (include/nttmul_galois.h) without a GPU: the library is built, exports
the whole ABI of the six headers unmangled, refuses bad arguments before any device access, and its
host-only entry points (nttmul_galois_element, nttmul_galois_plan) need no device at all."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import dispatch_cases as D
import galois_cases as C
import galois_ref as ref
import nttmul
import rnsmp_cases as R


def _defined(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True,
                         check=True).stdout
    return out, {line.split()[-1] for line in out.splitlines() if " T " in line}


def test_galois_library_is_built():
    assert os.path.exists(nttmul.GALOIS_LIB_PATH), f"{nttmul.GALOIS_LIB_PATH} not built"


def test_galois_library_exports_all_six_headers():
    _, have = _defined(nttmul.GALOIS_LIB_PATH)
    g = nttmul.galois_exported_symbols()
    assert g == sorted([
        "nttmul_galois_create", "nttmul_galois_destroy", "nttmul_galois_last_error",
        "nttmul_galois_get_info", "nttmul_galois_limb_info", "nttmul_galois_element",
        "nttmul_galois_plan", "nttmul_galois_coeff_device", "nttmul_galois_ntt_device",
        "nttmul_galois_ntt_many_device", "nttmul_galois_coeff", "nttmul_galois_ntt",
        "nttmul_galois_kernel_name"])
    want = (set(nttmul.exported_symbols()) | set(nttmul.mac_exported_symbols())
            | set(nttmul.rns_exported_symbols()) | set(nttmul.bconv_exported_symbols())
            | set(nttmul.rnsmp_exported_symbols()) | set(g))
    assert len(want) > 108
    assert sorted(want - have) == []
    assert sorted(s for s in have if s.startswith("nttmul_galois_") and s not in g) == []
    # the other headers' parsers do not pick the new names up
    assert not [s for s in nttmul.rns_exported_symbols() + nttmul.bconv_exported_symbols()
                + nttmul.rnsmp_exported_symbols() + nttmul.exported_symbols() if "galois" in s]
    text = open(nttmul.GALOIS_HEADER_PATH).read()
    assert f"#define NTTMUL_GALOIS_MAX_COUNT {nttmul.GALOIS_MAX_COUNT}\n" in text
    assert nttmul.GALOIS_MAX_COUNT == C.MAX_COUNT == 16


def _params(n, flags=0, q=0, psi=0):
    return nttmul._Params(n, q, psi, 1, 0, flags, 0, 0, 0, 0, 0)


def _create(lib, n, moduli, flags=0, q=0, psi=0, limbs=None):
    h = ctypes.c_void_p()
    prm = _params(n, flags, q, psi)
    qs = (ctypes.c_uint64 * max(1, len(moduli)))(*moduli)
    st = lib.nttmul_galois_create(ctypes.byref(h), ctypes.byref(prm), ctypes.sizeof(prm), qs,
                                  len(moduli) if limbs is None else limbs)
    if st == nttmul.NTTMUL_OK:      # (only where a device is present)
        lib.nttmul_galois_destroy(h)
    else:
        assert not h.value
    return st


def test_create_refusals_come_before_any_device_access():
    lib = nttmul.load_galois_library()
    EINVAL, EUNS = nttmul.NTTMUL_EINVAL, nttmul.NTTMUL_EUNSUPPORTED
    for n in (256, 4096, 8192, 65536):                                       # both ranges alike
        assert _create(lib, n, R.BASIS32, limbs=0) == EINVAL
        assert _create(lib, n, (D.Q31, D.Q31 + 2)) == EINVAL                 # not prime
        assert _create(lib, n, (D.Q31, D.Q31HI, D.Q31)) == EINVAL            # two equal primes
        assert _create(lib, n, R.BASIS32, q=D.Q31) == EINVAL                 # params->q
        assert _create(lib, n, R.BASIS32, psi=3) == EINVAL                   # params->psi
        assert _create(lib, n, (D.Q31, (1 << 62) + 1)) == EINVAL             # q >= 2^62
        assert _create(lib, n, R.BASIS32, flags=nttmul.NTTMUL_FLAG_CYCLIC) == EUNS
        assert _create(lib, n, (D.Q31, D.Q62)) == EUNS                       # mixed classes
        assert _create(lib, n, (D.Q62, D.Q31)) == EUNS
        assert _create(lib, n, (D.Q32,)) == EUNS                             # [2^31, 2^32)
        assert _create(lib, n, (D.Q31, D.Q32)) == EUNS
    many = list(range(3, 3 + nttmul.RNS_MAX_LIMBS + 1))
    assert _create(lib, 8192, many) == EINVAL                                # above the maximum
    assert _create(lib, 8192, (D.Q31, D.Q0)) == EINVAL                       # 2n does not divide q - 1
    assert _create(lib, 65536, (D.Q31, 2305843009213554689)) == EINVAL       # 2^13 | q - 1 only
    assert _create(lib, 10000, R.BASIS32) == EINVAL                          # n not a power of two
    assert _create(lib, 128, R.BASIS32) == EINVAL
    assert _create(lib, 131072, (D.Q31,)) == EUNS                            # a valid n above 65536
    assert _create(lib, 131072, (D.Q62,)) == EUNS
    h = ctypes.c_void_p()
    prm = _params(4096)
    qs = (ctypes.c_uint64 * 1)(D.Q31)
    assert lib.nttmul_galois_create(None, ctypes.byref(prm), ctypes.sizeof(prm), qs, 1) == EINVAL
    assert lib.nttmul_galois_create(ctypes.byref(h), None, ctypes.sizeof(prm), qs, 1) == EINVAL
    assert lib.nttmul_galois_create(ctypes.byref(h), ctypes.byref(prm), 4, qs, 1) == EINVAL
    assert lib.nttmul_galois_create(ctypes.byref(h), ctypes.byref(prm), ctypes.sizeof(prm), None, 1) == EINVAL
    # an invalid modulus is EINVAL even where the context would be unsupported anyway
    assert _create(lib, 131072, (D.Q31, D.Q31HI)) == EINVAL                  # 2^17 | q - 1 only
    # the stacked libraries' answers are unchanged, from this library too
    h = ctypes.c_void_p()
    prm = _params(8192)
    qs = (ctypes.c_uint64 * 3)(*R.BASIS32)
    assert lib.nttmul_rns_create(ctypes.byref(h), ctypes.byref(prm), ctypes.sizeof(prm), qs, 3) == EUNS
    prm = _params(4096)
    assert lib.nttmul_rnsmp_create(ctypes.byref(h), ctypes.byref(prm), ctypes.sizeof(prm), qs, 3) == EUNS


def test_call_refusals_come_before_any_device_access():
    lib = nttmul.load_galois_library()
    EINVAL = nttmul.NTTMUL_EINVAL
    one = (ctypes.c_uint32 * 1)()
    p = ctypes.addressof(one)
    ks = (ctypes.c_uint32 * 1)(3)
    assert lib.nttmul_galois_coeff_device(None, p, p, 3, 1, 0, None) == EINVAL
    assert lib.nttmul_galois_coeff_device(None, None, None, 3, 0, 0, None) == EINVAL
    assert lib.nttmul_galois_ntt_device(None, p, p, 3, 1, 0, None) == EINVAL
    assert lib.nttmul_galois_ntt_many_device(None, p, p, ks, 1, 1, 0, None) == EINVAL
    assert lib.nttmul_galois_ntt_many_device(None, p, p, ks, 0, 1, 0, None) == EINVAL
    assert lib.nttmul_galois_ntt_many_device(None, p, p, None, 1, 1, 0, None) == EINVAL
    assert lib.nttmul_galois_coeff(None, p, p, 3, 1) == EINVAL
    assert lib.nttmul_galois_ntt(None, p, p, 3, 1) == EINVAL
    buf = ctypes.create_string_buffer(64)
    assert lib.nttmul_galois_kernel_name(None, 0, 1, buf, len(buf)) == EINVAL
    assert lib.nttmul_galois_get_info(None, None) == EINVAL
    assert lib.nttmul_galois_limb_info(None, 0, None) == EINVAL
    assert lib.nttmul_galois_last_error(None) == b""
    lib.nttmul_galois_destroy(None)


def test_element_values():
    lib = nttmul.load_galois_library()
    for n in C.ALL_N:
        m = 2 * n
        inv5 = pow(5, -1, m)
        assert nttmul.galois_element(n, 0) == 1
        assert nttmul.galois_element(n, 1) == 5
        assert nttmul.galois_element(n, 7) == pow(5, 7, m)
        assert nttmul.galois_element(n, -1) == inv5
        assert nttmul.galois_element(n, -3) == pow(inv5, 3, m)
        assert nttmul.galois_element(n, 0, True) == m - 1
        assert nttmul.galois_element(n, 2, True) == 25 * (m - 1) % m
        assert nttmul.galois_element(n, -2, True) == pow(inv5, 2, m) * (m - 1) % m
        # 5 has order n / 2: steps wrap, however large
        assert nttmul.galois_element(n, n // 2) == 1
        assert nttmul.galois_element(n, n // 2 + 3) == pow(5, 3, m)
        for step in (-(1 << 62), (1 << 62) + 5, -(1 << 63), (1 << 63) - 1, 12345, -54321):
            for conj in (False, True):
                assert nttmul.galois_element(n, step, conj) == ref.element(n, step, conj)
        k = nttmul.galois_element(n, 3)
        assert k % 2 == 1 and k * nttmul.galois_element(n, -3) % m == 1
    k = ctypes.c_uint32(77)
    for n in (0, 128, 255, 1000, 131072, 1 << 31):
        assert lib.nttmul_galois_element(n, 1, 0, ctypes.byref(k)) == nttmul.NTTMUL_EINVAL
        with pytest.raises(nttmul.NttmulError):
            nttmul.galois_element(n, 1)
    assert lib.nttmul_galois_element(256, 1, 0, None) == nttmul.NTTMUL_EINVAL
    assert k.value == 77


def test_plan_refusals_and_partial_tables():
    lib = nttmul.load_galois_library()
    n = 256
    buf = np.full(n, 0xDEADBEEF, dtype=np.uint32)
    for k in (0, 2, 2 * n, 2 * n + 1, 4 * n + 3, (1 << 32) - 1):
        assert lib.nttmul_galois_plan(n, k, buf.ctypes.data, None, None) == nttmul.NTTMUL_EINVAL
        with pytest.raises(nttmul.NttmulError) as ei:
            nttmul.galois_plan(n, k)
        assert ei.value.status == nttmul.NTTMUL_EINVAL
    for bad in (0, 128, 300, 131072):
        assert lib.nttmul_galois_plan(bad, 3, buf.ctypes.data, None, None) == nttmul.NTTMUL_EINVAL
        with pytest.raises(nttmul.NttmulError):
            nttmul.galois_plan(bad, 3)
    assert (buf == 0xDEADBEEF).all()
    # a NULL table is skipped; the others are written in full and nothing past them
    guard = np.full(n + 8, 0xDEADBEEF, dtype=np.uint32)
    assert lib.nttmul_galois_plan(n, 2 * n - 1, None, None, guard.ctypes.data) == nttmul.NTTMUL_OK
    assert guard[:n].tolist() == ref.tables(n, 2 * n - 1)[2] and (guard[n:] == 0xDEADBEEF).all()
    assert lib.nttmul_galois_plan(n, 3, None, None, None) == nttmul.NTTMUL_OK


def test_galois_context_is_its_own_class_on_its_own_library():
    for name in ("coeff_device", "ntt_device", "ntt_many_device", "coeff", "ntt", "kernel_name",
                 "limb_info"):
        assert callable(getattr(nttmul.GaloisContext, name))
    assert not issubclass(nttmul.GaloisContext,
                          (nttmul.Context, nttmul.RnsContext, nttmul.RnsMpContext))
    libs = (nttmul.load_library(), nttmul.load_mac_library(), nttmul.load_rns_library(),
            nttmul.load_bconv_library(), nttmul.load_rnsmp_library(), nttmul.load_galois_library())
    assert len({id(x) for x in libs}) == 6
    assert [x._name for x in libs] == [nttmul.LIB_PATH, nttmul.MAC_LIB_PATH, nttmul.RNS_LIB_PATH,
                                       nttmul.BCONV_LIB_PATH, nttmul.RNSMP_LIB_PATH,
                                       nttmul.GALOIS_LIB_PATH]
    for older in libs[:5]:
        assert not hasattr(older, "nttmul_galois_create")
        assert not hasattr(older, "nttmul_galois_plan")
    assert nttmul.GALOIS_OPS == C.OPS


def test_python_refuses_what_the_library_refuses():
    for n in (4096, 8192):
        for moduli, status in (((D.Q31, D.Q31), nttmul.NTTMUL_EINVAL), ((), nttmul.NTTMUL_EINVAL),
                               ((D.Q31, D.Q62), nttmul.NTTMUL_EUNSUPPORTED),
                               ((D.Q32,), nttmul.NTTMUL_EUNSUPPORTED)):
            with pytest.raises(nttmul.NttmulError) as ei:
                nttmul.GaloisContext(n, moduli)
            assert ei.value.status == status
        with pytest.raises(nttmul.NttmulError) as ei:
            nttmul.GaloisContext(n, R.BASIS32, cyclic=True)
        assert ei.value.status == nttmul.NTTMUL_EUNSUPPORTED
    with pytest.raises(nttmul.NttmulError) as ei:
        nttmul.GaloisContext(131072, (D.Q31,))
    assert ei.value.status == nttmul.NTTMUL_EUNSUPPORTED
    with pytest.raises(nttmul.NttmulError) as ei:
        nttmul.GaloisContext(128, R.BASIS32)
    assert ei.value.status == nttmul.NTTMUL_EINVAL


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="checks the no-GPU behaviour")
def test_galois_context_without_a_device_fails_loudly():
    for n in (4096, 8192):
        with pytest.raises(nttmul.NttmulError) as ei:
            nttmul.GaloisContext(n, R.BASIS32)
        assert ei.value.status == nttmul.NTTMUL_ENODEV
