"""lib/libnttmul_mdntt.so (include/nttmul_mdntt.h) without a GPU: the library is built, exports the
whole ABI of the ten headers unmangled, and refuses bad arguments before any device access, every
create and call status in the header's order; valid arguments end in NTTMUL_ENODEV on a machine
with no device."""
import ctypes
import os
import subprocess

import pytest

import dispatch_cases as D
import ks_ref as ref
import mdntt_cases as C
import nttmul
import rnsmp_cases as R

OK_OR_NODEV = (nttmul.NTTMUL_OK, nttmul.NTTMUL_ENODEV)


def _defined(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True,
                         check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if " T " in line}


def test_mdntt_library_is_built():
    assert os.path.exists(nttmul.MDNTT_LIB_PATH), f"{nttmul.MDNTT_LIB_PATH} not built"


def test_mdntt_library_exports_all_ten_headers():
    have = _defined(nttmul.MDNTT_LIB_PATH)
    m = nttmul.mdntt_exported_symbols()
    assert m == sorted("nttmul_mdntt_" + s for s in (
        "create", "destroy", "last_error", "get_info", "moddown_device", "moddown", "kernel_name"))
    older = (set(nttmul.exported_symbols()) | set(nttmul.mac_exported_symbols())
             | set(nttmul.rns_exported_symbols()) | set(nttmul.bconv_exported_symbols())
             | set(nttmul.rnsmp_exported_symbols()) | set(nttmul.galois_exported_symbols())
             | set(nttmul.ks_exported_symbols()) | set(nttmul.macn_exported_symbols())
             | set(nttmul.hoist_exported_symbols()))
    assert sorted((older | set(m)) - have) == []
    assert older <= _defined(nttmul.HOIST_LIB_PATH)
    assert sorted(s for s in have if s.startswith("nttmul_mdntt_") and s not in m) == []
    # the library adds the seven entry points to the hoist library's and nothing else
    assert {s for s in have - _defined(nttmul.HOIST_LIB_PATH) if s.startswith("nttmul_")} == set(m)
    # the other headers' parsers do not pick the new names up
    assert not [s for s in older if "_mdntt_" in s]


def _params(n, flags=0, q=0, psi=0):
    return nttmul._Params(n, q, psi, 1, 0, flags, 0, 0, 0, 0, 0)


def _create(lib, n, q, p, flags=0, pq=0, psi=0, L=None, K=None):
    h = ctypes.c_void_p()
    prm = _params(n, flags, pq, psi)
    qa = (ctypes.c_uint64 * max(1, len(q)))(*q)
    pa = (ctypes.c_uint64 * max(1, len(p)))(*p)
    L, K = len(q) if L is None else L, len(p) if K is None else K
    st = lib.nttmul_mdntt_create(ctypes.byref(h), ctypes.byref(prm), ctypes.sizeof(prm), qa, L,
                                 pa, K)
    if st == nttmul.NTTMUL_OK:      # (only where a device is present)
        lib.nttmul_mdntt_destroy(h)
    else:
        assert not h.value
    # nttmul_ks_create's status with any valid digit width is the same decision
    ks = ctypes.c_void_p()
    st_ks = lib.nttmul_ks_create(ctypes.byref(ks), ctypes.byref(prm), ctypes.sizeof(prm), qa, L,
                                 pa, K, 1)
    if st_ks == nttmul.NTTMUL_OK:
        lib.nttmul_ks_destroy(ks)
    assert st_ks == st or {st, st_ks} <= set(OK_OR_NODEV)
    return st


def test_create_refusals_come_before_any_device_access():
    lib = nttmul.load_mdntt_library()
    EINVAL, EUNS = nttmul.NTTMUL_EINVAL, nttmul.NTTMUL_EUNSUPPORTED
    Q32, P32 = R.BASIS32[:2], R.BASIS32[2:]
    Q64, P64 = R.BASIS64[:2], R.BASIS64[2:]
    for n in (256, 4096, 8192, 65536):                                       # every range alike
        for Q, P in ((Q32, P32), (Q64, P64)):
            assert _create(lib, n, Q, P) in OK_OR_NODEV
            assert _create(lib, n, Q, P, L=0) == EINVAL
            assert _create(lib, n, Q, P, K=0) == EINVAL                      # p_limbs = 0
            assert _create(lib, n, Q, Q[:1]) == EINVAL                       # a prime in both bases
            assert _create(lib, n, Q + Q[:1], P) == EINVAL                   # twice within Q
            assert _create(lib, n, Q, P + P) == EINVAL                       # twice within P
            assert _create(lib, n, Q, P, pq=D.Q31) == EINVAL                 # params->q
            assert _create(lib, n, Q, P, psi=3) == EINVAL                    # params->psi
            assert _create(lib, n, Q, P, flags=nttmul.NTTMUL_FLAG_CYCLIC) == EUNS
            # the order: every EINVAL before any EUNSUPPORTED
            assert _create(lib, n, Q, P + P, flags=nttmul.NTTMUL_FLAG_CYCLIC) == EINVAL
        assert _create(lib, n, (D.Q31, D.Q31 + 2), P32) == EINVAL            # not prime
        assert _create(lib, n, Q32, (D.Q31LO + 2,)) == EINVAL
        assert _create(lib, n, Q32, ((1 << 62) + 1,)) == EINVAL              # >= 2^62
        assert _create(lib, n, Q32, P64) == EUNS                             # mixed across Q and P
        assert _create(lib, n, Q64, P32) == EUNS
        assert _create(lib, n, (D.Q31, D.Q62), P32) == EUNS                  # mixed within Q
        assert _create(lib, n, Q64, (R.BASIS64[2], D.Q31)) == EUNS           # mixed within P
        assert _create(lib, n, (D.Q32,), P32) == EUNS                        # [2^31, 2^32)
        assert _create(lib, n, Q32, (D.Q32,)) == EUNS
        assert _create(lib, n, (D.Q32,), (D.Q31LO + 2,)) == EINVAL           # EINVAL of P first
    # q_limbs + p_limbs > NTTMUL_RNS_MAX_LIMBS: the extended basis has to fit one context
    q, p = ref.bases(32, 60, 5)
    assert len(q) + len(p) == nttmul.RNS_MAX_LIMBS + 1
    for n in (256, 65536):
        assert _create(lib, n, q, p) == EINVAL
        assert _create(lib, n, q, p, flags=nttmul.NTTMUL_FLAG_CYCLIC) == EINVAL   # before EUNS
        assert _create(lib, n, q, p[:4]) in OK_OR_NODEV
    q, p = ref.bases(64, 1, 63)
    assert _create(lib, 256, q, p) in OK_OR_NODEV
    many = list(range(3, 3 + nttmul.RNS_MAX_LIMBS + 1))
    assert _create(lib, 8192, many, P32) == EINVAL                           # above the maximum
    assert _create(lib, 8192, Q32, many) == EINVAL
    assert _create(lib, 8192, (D.Q31, D.Q0), P32) == EINVAL                  # 2n does not divide q - 1
    assert _create(lib, 2048, (D.Q31, D.Q0), P32) in OK_OR_NODEV
    assert _create(lib, 10000, Q32, P32) == EINVAL                           # n not a power of two
    assert _create(lib, 128, Q32, P32) == EINVAL
    assert _create(lib, 131072, (D.Q31,), (D.Q31HI,)) == EINVAL              # 2^17 | q - 1 only
    for bits in (32, 64):                                                    # a valid n above 65536
        q18 = ref.B.primes_below(ref.TOP[bits], 1 << 18, 2)
        assert _create(lib, 131072, q18[:1], q18[1:]) == EUNS
    h = ctypes.c_void_p()
    prm = _params(4096)
    qa, pa = (ctypes.c_uint64 * 1)(D.Q31), (ctypes.c_uint64 * 1)(D.Q31HI)
    sz = ctypes.sizeof(prm)
    assert lib.nttmul_mdntt_create(None, ctypes.byref(prm), sz, qa, 1, pa, 1) == EINVAL
    assert lib.nttmul_mdntt_create(ctypes.byref(h), None, sz, qa, 1, pa, 1) == EINVAL
    assert lib.nttmul_mdntt_create(ctypes.byref(h), ctypes.byref(prm), 4, qa, 1, pa, 1) == EINVAL
    assert lib.nttmul_mdntt_create(ctypes.byref(h), ctypes.byref(prm), sz, None, 1, pa, 1) == EINVAL
    assert lib.nttmul_mdntt_create(ctypes.byref(h), ctypes.byref(prm), sz, qa, 1, None, 1) == EINVAL


def test_call_refusals_come_before_any_device_access():
    lib = nttmul.load_mdntt_library()
    EINVAL = nttmul.NTTMUL_EINVAL
    one = (ctypes.c_uint32 * 1)()
    p = ctypes.addressof(one)
    assert lib.nttmul_mdntt_moddown_device(None, p, p, 1, 0, None) == EINVAL
    assert lib.nttmul_mdntt_moddown_device(None, None, None, 0, 0, None) == EINVAL
    assert lib.nttmul_mdntt_moddown(None, p, p, 1) == EINVAL
    assert lib.nttmul_mdntt_moddown(None, None, None, 0) == EINVAL
    buf = ctypes.create_string_buffer(64)
    assert lib.nttmul_mdntt_kernel_name(None, buf, len(buf)) == EINVAL
    assert lib.nttmul_mdntt_get_info(None, None) == EINVAL
    assert lib.nttmul_mdntt_last_error(None) == b""
    lib.nttmul_mdntt_destroy(None)


def test_ntt_moddown_is_its_own_class_on_its_own_library():
    for name in ("moddown_device", "moddown", "kernel_name", "close"):
        assert callable(getattr(nttmul.NttModDown, name))
    new, hoist = nttmul.load_mdntt_library(), nttmul.load_hoist_library()
    assert new is not hoist and new._name == nttmul.MDNTT_LIB_PATH
    for older in (nttmul.load_library(), nttmul.load_ks_library(), hoist):
        assert not hasattr(older, "nttmul_mdntt_create")
    assert ctypes.sizeof(nttmul.MdNttInfo) == 28
    hdr = open(nttmul.MDNTT_HEADER_PATH).read()
    assert "uint32_t n, logn, q_limbs, p_limbs;" in hdr and "uint32_t scratch_mb;" in hdr


def test_python_refuses_what_the_library_refuses():
    Q, P = R.BASIS32[:2], R.BASIS32[2:]
    for n in (4096, 8192):
        for args, status in (((Q, Q[:1]), nttmul.NTTMUL_EINVAL), ((Q, ()), nttmul.NTTMUL_EINVAL),
                             ((Q, R.BASIS64[:1]), nttmul.NTTMUL_EUNSUPPORTED),
                             ((Q, (D.Q32,)), nttmul.NTTMUL_EUNSUPPORTED)):
            with pytest.raises(nttmul.NttmulError) as ei:
                nttmul.NttModDown(n, *args)
            assert ei.value.status == status
        with pytest.raises(nttmul.NttmulError) as ei:
            nttmul.NttModDown(n, Q, P, cyclic=True)
        assert ei.value.status == nttmul.NTTMUL_EUNSUPPORTED


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="checks the no-GPU behaviour")
def test_ntt_moddown_without_a_device_fails_loudly():
    for n in C.ALL_N:
        with pytest.raises(nttmul.NttmulError) as ei:
            nttmul.NttModDown(n, R.BASIS32[:2], R.BASIS32[2:])
        assert ei.value.status == nttmul.NTTMUL_ENODEV
