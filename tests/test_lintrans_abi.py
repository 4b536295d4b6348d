"""lib/libnttmul_lintrans.so (include/nttmul_lintrans.h) without a GPU: the library is built,
exports the whole ABI of the twelve headers unmangled, and refuses bad arguments before any device
access, every create status in nttmul_ksntt_create's order without the digit width's, and every
call status a NULL context allows (the order of apply's other statuses needs a context:
tests/sanitize/lintrans_san.cpp walks it on csrc/lintrans_plan.hpp, which is what the entry points
call); valid arguments end in NTTMUL_ENODEV on a machine with no device."""
import ctypes
import os
import subprocess

import pytest

import dispatch_cases as D
import ks_ref as ref
import nttmul
import rnsmp_cases as R

OK_OR_NODEV = (nttmul.NTTMUL_OK, nttmul.NTTMUL_ENODEV)
ENTRY_POINTS = ("create", "destroy", "last_error", "get_info", "apply_device", "apply",
                "kernel_name")


def _defined(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True,
                         check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if " T " in line}


def test_lintrans_library_is_built():
    assert os.path.exists(nttmul.LINTRANS_LIB_PATH), f"{nttmul.LINTRANS_LIB_PATH} not built"


def test_lintrans_library_exports_all_twelve_headers():
    have = _defined(nttmul.LINTRANS_LIB_PATH)
    k = nttmul.lintrans_exported_symbols()
    assert k == sorted("nttmul_lintrans_" + s for s in ENTRY_POINTS)
    assert set(k) <= have
    # every symbol of libnttmul_ksntt.so is still there
    ksntt = _defined(nttmul.KSNTT_LIB_PATH)
    assert set(nttmul.ksntt_exported_symbols()) <= ksntt
    assert sorted(ksntt - have) == []
    # the library adds the seven entry points to the ksntt library's and nothing else
    assert {s for s in have - ksntt if s.startswith("nttmul_")} == set(k)
    assert not [s for s in ksntt if "_lintrans_" in s]


def _params(n, flags=0, q=0, psi=0):
    return nttmul._Params(n, q, psi, 1, 0, flags, 0, 0, 0, 0, 0)


def _create(lib, n, q, p, flags=0, pq=0, psi=0, L=None, K=None):
    h = ctypes.c_void_p()
    prm = _params(n, flags, pq, psi)
    qa = (ctypes.c_uint64 * max(1, len(q)))(*q)
    pa = (ctypes.c_uint64 * max(1, len(p)))(*p)
    L, K = len(q) if L is None else L, len(p) if K is None else K
    st = lib.nttmul_lintrans_create(ctypes.byref(h), ctypes.byref(prm), ctypes.sizeof(prm), qa, L,
                                    pa, K)
    if st == nttmul.NTTMUL_OK:      # (only where a device is present)
        lib.nttmul_lintrans_destroy(h)
    else:
        assert not h.value
    # nttmul_ksntt_create's status with one digit of one limb is the same decision
    if L >= 1:
        ks = ctypes.c_void_p()
        st_ks = lib.nttmul_ksntt_create(ctypes.byref(ks), ctypes.byref(prm), ctypes.sizeof(prm),
                                        qa, L, pa, K, 1)
        if st_ks == nttmul.NTTMUL_OK:
            lib.nttmul_ksntt_destroy(ks)
        assert st_ks == st or {st, st_ks} <= set(OK_OR_NODEV)
    return st


def test_create_refusals_come_before_any_device_access():
    lib = nttmul.load_lintrans_library()
    EINVAL, EUNS = nttmul.NTTMUL_EINVAL, nttmul.NTTMUL_EUNSUPPORTED
    CYC = nttmul.NTTMUL_FLAG_CYCLIC
    Q32, P32 = R.BASIS32[:2], R.BASIS32[2:]
    Q64, P64 = R.BASIS64[:2], R.BASIS64[2:]
    for n in (256, 4096, 8192, 65536):                                       # every range alike
        for Q, P in ((Q32, P32), (Q64, P64)):
            assert _create(lib, n, Q, P) in OK_OR_NODEV
            assert _create(lib, n, Q, P, L=0) == EINVAL
            assert _create(lib, n, Q, P, K=0) == EINVAL
            assert _create(lib, n, Q, Q[:1]) == EINVAL                       # a prime in both bases
            assert _create(lib, n, Q + Q[:1], P) == EINVAL                   # twice within Q
            assert _create(lib, n, Q, P + P) == EINVAL                       # twice within P
            assert _create(lib, n, Q, P, pq=D.Q31) == EINVAL                 # params->q
            assert _create(lib, n, Q, P, psi=3) == EINVAL                    # params->psi
            assert _create(lib, n, Q, P, flags=CYC) == EUNS
            # the order: every EINVAL before any EUNSUPPORTED
            assert _create(lib, n, Q, P + P, flags=CYC) == EINVAL
        assert _create(lib, n, (D.Q31, D.Q31 + 2), P32) == EINVAL            # not prime
        assert _create(lib, n, Q32, ((1 << 62) + 1,)) == EINVAL              # >= 2^62
        assert _create(lib, n, Q32, P64) == EUNS                             # mixed across Q and P
        assert _create(lib, n, Q64, P32) == EUNS
        assert _create(lib, n, (D.Q31, D.Q62), P32) == EUNS                  # mixed within Q
        assert _create(lib, n, (D.Q32,), P32) == EUNS                        # [2^31, 2^32)
        assert _create(lib, n, (D.Q32,), (D.Q31LO + 2,)) == EINVAL           # EINVAL of P first
    # q_limbs + p_limbs > NTTMUL_RNS_MAX_LIMBS: the extended basis has to fit one context
    q, p = ref.bases(32, 60, 5)
    assert len(q) + len(p) == nttmul.RNS_MAX_LIMBS + 1
    for n in (256, 65536):
        assert _create(lib, n, q, p) == EINVAL
        assert _create(lib, n, q, p, flags=CYC) == EINVAL                    # before EUNS
        assert _create(lib, n, q, p[:4]) in OK_OR_NODEV
    assert _create(lib, 10000, Q32, P32) == EINVAL                           # n not a power of two
    assert _create(lib, 128, Q32, P32) == EINVAL
    for bits in (32, 64):                                                    # a valid n above 65536
        q18 = ref.B.primes_below(ref.TOP[bits], 1 << 18, 2)
        assert _create(lib, 131072, q18[:1], q18[1:]) == EUNS
    h = ctypes.c_void_p()
    prm = _params(4096)
    qa, pa = (ctypes.c_uint64 * 1)(D.Q31), (ctypes.c_uint64 * 1)(D.Q31HI)
    sz = ctypes.sizeof(prm)
    create = lib.nttmul_lintrans_create
    assert create(None, ctypes.byref(prm), sz, qa, 1, pa, 1) == EINVAL
    assert create(ctypes.byref(h), None, sz, qa, 1, pa, 1) == EINVAL
    assert create(ctypes.byref(h), ctypes.byref(prm), 4, qa, 1, pa, 1) == EINVAL
    assert create(ctypes.byref(h), ctypes.byref(prm), sz, None, 1, pa, 1) == EINVAL
    assert create(ctypes.byref(h), ctypes.byref(prm), sz, qa, 1, None, 1) == EINVAL


def test_call_refusals_come_before_any_device_access():
    lib = nttmul.load_lintrans_library()
    EINVAL = nttmul.NTTMUL_EINVAL
    one = (ctypes.c_uint32 * 1)(1)
    p = ctypes.addressof(one)
    dev, host = lib.nttmul_lintrans_apply_device, lib.nttmul_lintrans_apply
    assert dev(None, p, p, p, p, p, one, 1, 1, 1, 1, 0, None) == EINVAL
    assert dev(None, p, p, p, None, None, one, 1, 1, 1, 1, 0, None) == EINVAL
    assert dev(None, None, None, None, None, None, one, 1, 0, 1, 1, 0, None) == EINVAL
    assert host(None, p, p, p, p, p, one, 1, 1, 1, 1) == EINVAL
    assert host(None, None, None, None, None, None, None, 0, 0, 0, 0) == EINVAL
    buf = ctypes.create_string_buffer(64)
    for comps in (0, 1, 2, 3):
        for weighted in (0, 1):
            assert lib.nttmul_lintrans_kernel_name(None, comps, weighted, buf, len(buf)) == EINVAL
    assert lib.nttmul_lintrans_get_info(None, None) == EINVAL
    assert lib.nttmul_lintrans_last_error(None) == b""
    lib.nttmul_lintrans_destroy(None)


def test_ntt_lin_trans_is_its_own_class_on_its_own_library():
    for name in ("apply_device", "apply", "kernel_name", "close", "__enter__", "__exit__"):
        assert callable(getattr(nttmul.NttLinTrans, name))
    new, ksntt = nttmul.load_lintrans_library(), nttmul.load_ksntt_library()
    assert new is not ksntt and new._name == nttmul.LINTRANS_LIB_PATH
    for older in (nttmul.load_library(), nttmul.load_ks_library(), nttmul.load_hoist_library(),
                  nttmul.load_mdntt_library(), ksntt):
        assert not hasattr(older, "nttmul_lintrans_create")
    assert ctypes.sizeof(nttmul.LinTransInfo) == 24
    hdr = open(nttmul.LINTRANS_HEADER_PATH).read()
    assert "uint32_t n, logn, q_limbs, p_limbs;" in hdr and '#include "nttmul_ksntt.h"' in hdr


def test_the_ksntt_header_points_to_the_new_one():
    text = open(nttmul.KSNTT_HEADER_PATH).read()
    scope = text[text.index("Out of scope"):text.index("#ifndef")]
    assert "nttmul_lintrans.h" in scope
    own = open(nttmul.LINTRANS_HEADER_PATH).read()
    scope = own[own.index("Out of scope"):own.index("#ifndef")]
    for word in ("per batch entry", "NTTMUL_MACN_MAX_COMPS", "BSGS", "rounding in ModDown",
                 "NTTMUL_FLAG_CYCLIC", "multi-device", "bench.py"):
        assert word in scope, word
    assert "identity rotation" in own


def test_python_refuses_what_the_library_refuses():
    Q, P = R.BASIS32[:2], R.BASIS32[2:]
    for n in (4096, 8192):
        for args, status in (((Q, Q[:1]), nttmul.NTTMUL_EINVAL),
                             ((Q, R.BASIS64[:1]), nttmul.NTTMUL_EUNSUPPORTED),
                             ((Q, (D.Q32,)), nttmul.NTTMUL_EUNSUPPORTED)):
            with pytest.raises(nttmul.NttmulError) as ei:
                nttmul.NttLinTrans(n, *args)
            assert ei.value.status == status
        with pytest.raises(nttmul.NttmulError) as ei:
            nttmul.NttLinTrans(n, Q, P, cyclic=True)
        assert ei.value.status == nttmul.NTTMUL_EUNSUPPORTED


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="checks the no-GPU behaviour")
def test_ntt_lin_trans_without_a_device_fails_loudly():
    for n in (256, 4096, 8192, 65536):
        with pytest.raises(nttmul.NttmulError) as ei:
            nttmul.NttLinTrans(n, R.BASIS32[:2], R.BASIS32[2:])
        assert ei.value.status == nttmul.NTTMUL_ENODEV
