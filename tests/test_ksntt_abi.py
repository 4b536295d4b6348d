"""lib/libnttmul_ksntt.so (include/nttmul_ksntt.h) without a GPU: the library is built, exports the
whole ABI of the eleven headers unmangled, and refuses bad arguments before any device access,
every create status in nttmul_ks_create's order and every call status a NULL context allows (the
order of the calls' other statuses needs a context: tests/sanitize/ksntt_san.cpp walks it on
csrc/ksntt_plan.hpp, which is what the entry points call); valid arguments end in NTTMUL_ENODEV
on a machine with no device."""
import ctypes
import os
import subprocess

import pytest

import dispatch_cases as D
import ks_ref as ref
import nttmul
import rnsmp_cases as R

OK_OR_NODEV = (nttmul.NTTMUL_OK, nttmul.NTTMUL_ENODEV)
ENTRY_POINTS = ("create", "destroy", "last_error", "get_info", "modup_device", "modup",
                "mac_device", "mac", "kernel_name")


def _defined(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True,
                         check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if " T " in line}


def test_ksntt_library_is_built():
    assert os.path.exists(nttmul.KSNTT_LIB_PATH), f"{nttmul.KSNTT_LIB_PATH} not built"


def test_ksntt_library_exports_all_eleven_headers():
    have = _defined(nttmul.KSNTT_LIB_PATH)
    k = nttmul.ksntt_exported_symbols()
    assert k == sorted("nttmul_ksntt_" + s for s in ENTRY_POINTS)
    older = (set(nttmul.exported_symbols()) | set(nttmul.mac_exported_symbols())
             | set(nttmul.rns_exported_symbols()) | set(nttmul.bconv_exported_symbols())
             | set(nttmul.rnsmp_exported_symbols()) | set(nttmul.galois_exported_symbols())
             | set(nttmul.ks_exported_symbols()) | set(nttmul.macn_exported_symbols())
             | set(nttmul.hoist_exported_symbols()) | set(nttmul.mdntt_exported_symbols()))
    assert sorted((older | set(k)) - have) == []
    assert older <= _defined(nttmul.MDNTT_LIB_PATH)
    # the library adds the nine entry points to the mdntt library's and nothing else
    assert {s for s in have - _defined(nttmul.MDNTT_LIB_PATH) if s.startswith("nttmul_")} == set(k)
    assert not [s for s in older if "_ksntt_" in s]


def _params(n, flags=0, q=0, psi=0):
    return nttmul._Params(n, q, psi, 1, 0, flags, 0, 0, 0, 0, 0)


def _create(lib, n, q, p, alpha=1, flags=0, pq=0, psi=0, L=None, K=None):
    h = ctypes.c_void_p()
    prm = _params(n, flags, pq, psi)
    qa = (ctypes.c_uint64 * max(1, len(q)))(*q)
    pa = (ctypes.c_uint64 * max(1, len(p)))(*p)
    L, K = len(q) if L is None else L, len(p) if K is None else K
    st = lib.nttmul_ksntt_create(ctypes.byref(h), ctypes.byref(prm), ctypes.sizeof(prm), qa, L,
                                 pa, K, alpha)
    if st == nttmul.NTTMUL_OK:      # (only where a device is present)
        lib.nttmul_ksntt_destroy(h)
    else:
        assert not h.value
    # nttmul_ks_create's status is the same decision
    ks = ctypes.c_void_p()
    st_ks = lib.nttmul_ks_create(ctypes.byref(ks), ctypes.byref(prm), ctypes.sizeof(prm), qa, L,
                                 pa, K, alpha)
    if st_ks == nttmul.NTTMUL_OK:
        lib.nttmul_ks_destroy(ks)
    assert st_ks == st or {st, st_ks} <= set(OK_OR_NODEV)
    return st


def test_create_refusals_come_before_any_device_access():
    lib = nttmul.load_ksntt_library()
    EINVAL, EUNS = nttmul.NTTMUL_EINVAL, nttmul.NTTMUL_EUNSUPPORTED
    CYC = nttmul.NTTMUL_FLAG_CYCLIC
    Q32, P32 = R.BASIS32[:2], R.BASIS32[2:]
    Q64, P64 = R.BASIS64[:2], R.BASIS64[2:]
    for n in (256, 4096, 8192, 65536):                                       # every range alike
        for Q, P in ((Q32, P32), (Q64, P64)):
            for alpha in (1, 2):
                assert _create(lib, n, Q, P, alpha) in OK_OR_NODEV
            assert _create(lib, n, Q, P, L=0) == EINVAL
            assert _create(lib, n, Q, P, K=0) == EINVAL
            assert _create(lib, n, Q, Q[:1]) == EINVAL                       # a prime in both bases
            assert _create(lib, n, Q + Q[:1], P) == EINVAL                   # twice within Q
            assert _create(lib, n, Q, P + P) == EINVAL                       # twice within P
            assert _create(lib, n, Q, P, pq=D.Q31) == EINVAL                 # params->q
            assert _create(lib, n, Q, P, psi=3) == EINVAL                    # params->psi
            assert _create(lib, n, Q, P, 0) == EINVAL                        # the digit width
            assert _create(lib, n, Q, P, 3) == EINVAL                        # digit_limbs > q_limbs
            assert _create(lib, n, Q, P, flags=CYC) == EUNS
            # the order: every EINVAL, the digit width's too, before any EUNSUPPORTED
            assert _create(lib, n, Q, P + P, flags=CYC) == EINVAL
            assert _create(lib, n, Q, P, 0, flags=CYC) == EINVAL
            assert _create(lib, n, Q, P, 3, flags=CYC) == EINVAL
        assert _create(lib, n, (D.Q31, D.Q31 + 2), P32) == EINVAL            # not prime
        assert _create(lib, n, Q32, ((1 << 62) + 1,)) == EINVAL              # >= 2^62
        assert _create(lib, n, Q32, P64) == EUNS                             # mixed across Q and P
        assert _create(lib, n, Q64, P32) == EUNS
        assert _create(lib, n, (D.Q31, D.Q62), P32) == EUNS                  # mixed within Q
        assert _create(lib, n, (D.Q32,), P32) == EUNS                        # [2^31, 2^32)
        assert _create(lib, n, (D.Q32,), P32, 2) == EINVAL                   # the width before EUNS
        assert _create(lib, n, (D.Q32,), (D.Q31LO + 2,)) == EINVAL           # EINVAL of P first
    # q_limbs + p_limbs > NTTMUL_RNS_MAX_LIMBS: the extended basis has to fit one context
    q, p = ref.bases(32, 60, 5)
    assert len(q) + len(p) == nttmul.RNS_MAX_LIMBS + 1
    for n in (256, 65536):
        assert _create(lib, n, q, p, 15) == EINVAL
        assert _create(lib, n, q, p, 15, flags=CYC) == EINVAL                # before EUNS
        assert _create(lib, n, q, p[:4], 15) in OK_OR_NODEV
        assert _create(lib, n, q, p[:4], 60) in OK_OR_NODEV                  # one digit of all of Q
        assert _create(lib, n, q, p[:4], 61) == EINVAL
    assert _create(lib, 10000, Q32, P32) == EINVAL                           # n not a power of two
    assert _create(lib, 128, Q32, P32) == EINVAL
    for bits in (32, 64):                                                    # a valid n above 65536
        q18 = ref.B.primes_below(ref.TOP[bits], 1 << 18, 2)
        assert _create(lib, 131072, q18[:1], q18[1:]) == EUNS
        assert _create(lib, 131072, q18[:1], q18[1:], 2) == EINVAL
    h = ctypes.c_void_p()
    prm = _params(4096)
    qa, pa = (ctypes.c_uint64 * 1)(D.Q31), (ctypes.c_uint64 * 1)(D.Q31HI)
    sz = ctypes.sizeof(prm)
    create = lib.nttmul_ksntt_create
    assert create(None, ctypes.byref(prm), sz, qa, 1, pa, 1, 1) == EINVAL
    assert create(ctypes.byref(h), None, sz, qa, 1, pa, 1, 1) == EINVAL
    assert create(ctypes.byref(h), ctypes.byref(prm), 4, qa, 1, pa, 1, 1) == EINVAL
    assert create(ctypes.byref(h), ctypes.byref(prm), sz, None, 1, pa, 1, 1) == EINVAL
    assert create(ctypes.byref(h), ctypes.byref(prm), sz, qa, 1, None, 1, 1) == EINVAL


def test_call_refusals_come_before_any_device_access():
    lib = nttmul.load_ksntt_library()
    EINVAL = nttmul.NTTMUL_EINVAL
    one = (ctypes.c_uint32 * 1)(1)
    p = ctypes.addressof(one)
    assert lib.nttmul_ksntt_modup_device(None, p, p, 1, 0, None) == EINVAL
    assert lib.nttmul_ksntt_modup_device(None, None, None, 0, 0, None) == EINVAL
    assert lib.nttmul_ksntt_modup(None, p, p, 1) == EINVAL
    assert lib.nttmul_ksntt_modup(None, None, None, 0) == EINVAL
    assert lib.nttmul_ksntt_mac_device(None, p, p, p, one, 1, 1, 1, 1, 0, None) == EINVAL
    assert lib.nttmul_ksntt_mac_device(None, None, None, None, one, 1, 0, 1, 1, 0, None) == EINVAL
    assert lib.nttmul_ksntt_mac(None, p, p, p, one, 1, 1, 1, 1) == EINVAL
    assert lib.nttmul_ksntt_mac(None, None, None, None, None, 0, 0, 0, 0) == EINVAL
    buf = ctypes.create_string_buffer(64)
    for op in (0, 1, 2, -1):
        assert lib.nttmul_ksntt_kernel_name(None, op, 1, buf, len(buf)) == EINVAL
    assert lib.nttmul_ksntt_get_info(None, None) == EINVAL
    assert lib.nttmul_ksntt_last_error(None) == b""
    lib.nttmul_ksntt_destroy(None)


def test_ntt_key_switch_is_its_own_class_on_its_own_library():
    for name in ("modup_device", "modup", "mac_device", "mac", "kernel_name", "close"):
        assert callable(getattr(nttmul.NttKeySwitch, name))
    new, mdntt = nttmul.load_ksntt_library(), nttmul.load_mdntt_library()
    assert new is not mdntt and new._name == nttmul.KSNTT_LIB_PATH
    for older in (nttmul.load_library(), nttmul.load_ks_library(), nttmul.load_hoist_library(),
                  mdntt):
        assert not hasattr(older, "nttmul_ksntt_create")
    # nttmul_ks_info's fields plus scratch_mb
    assert [f[0] for f in nttmul.KsNttInfo._fields_] == \
        [f[0] for f in nttmul.KsInfo._fields_] + ["scratch_mb"]
    assert ctypes.sizeof(nttmul.KsNttInfo) == ctypes.sizeof(nttmul.KsInfo) + 4 == 36
    hdr = open(nttmul.KSNTT_HEADER_PATH).read()
    assert "uint32_t n, logn, q_limbs, p_limbs, digit_limbs, digits;" in hdr
    assert "uint32_t scratch_mb;" in hdr and '#include "nttmul_mdntt.h"' in hdr


def test_the_older_headers_point_to_the_new_one():
    inc = os.path.dirname(nttmul.KSNTT_HEADER_PATH)
    for name in ("nttmul_ks.h", "nttmul_hoist.h", "nttmul_mdntt.h"):
        text = open(os.path.join(inc, name)).read()
        scope = text[text.index("Out of scope"):text.index("#ifndef")]
        assert "nttmul_ksntt.h" in scope, name


def test_python_refuses_what_the_library_refuses():
    Q, P = R.BASIS32[:2], R.BASIS32[2:]
    for n in (4096, 8192):
        for args, status in (((Q, Q[:1], 1), nttmul.NTTMUL_EINVAL),
                             ((Q, P, 0), nttmul.NTTMUL_EINVAL), ((Q, P, 3), nttmul.NTTMUL_EINVAL),
                             ((Q, R.BASIS64[:1], 1), nttmul.NTTMUL_EUNSUPPORTED),
                             ((Q, (D.Q32,), 1), nttmul.NTTMUL_EUNSUPPORTED)):
            with pytest.raises(nttmul.NttmulError) as ei:
                nttmul.NttKeySwitch(n, *args)
            assert ei.value.status == status
        with pytest.raises(nttmul.NttmulError) as ei:
            nttmul.NttKeySwitch(n, Q, P, 1, cyclic=True)
        assert ei.value.status == nttmul.NTTMUL_EUNSUPPORTED


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="checks the no-GPU behaviour")
def test_ntt_key_switch_without_a_device_fails_loudly():
    for n in (256, 4096, 8192, 65536):
        with pytest.raises(nttmul.NttmulError) as ei:
            nttmul.NttKeySwitch(n, R.BASIS32[:2], R.BASIS32[2:], 1)
        assert ei.value.status == nttmul.NTTMUL_ENODEV
