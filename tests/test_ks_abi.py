"""lib/libnttmul_ks.so (include/nttmul_ks.h) without a GPU: the library is built, exports the whole
ABI of the seven headers unmangled, refuses bad arguments before any device access, and its
host-only entry point nttmul_ks_plan equals tests/ks_ref.py (and nttmul_bconv_plan for the ModDown
constants) with no device at all."""
import ctypes
import os
import subprocess

import pytest

import bconv_cases as BC
import dispatch_cases as D
import ks_cases as C
import ks_ref as ref
import nttmul
import rnsmp_cases as R


def _defined(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True,
                         check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if " T " in line}


def test_ks_library_is_built():
    assert os.path.exists(nttmul.KS_LIB_PATH), f"{nttmul.KS_LIB_PATH} not built"


def test_ks_library_exports_all_seven_headers():
    have = _defined(nttmul.KS_LIB_PATH)
    k = nttmul.ks_exported_symbols()
    assert k == sorted("nttmul_ks_" + s for s in (
        "create", "destroy", "last_error", "get_info", "plan", "modup_device", "moddown_device",
        "modup", "moddown", "kernel_name"))
    want = (set(nttmul.exported_symbols()) | set(nttmul.mac_exported_symbols())
            | set(nttmul.rns_exported_symbols()) | set(nttmul.bconv_exported_symbols())
            | set(nttmul.rnsmp_exported_symbols()) | set(nttmul.galois_exported_symbols()) | set(k))
    assert len(want) == 120
    assert sorted(want - have) == []
    assert sorted(s for s in have if s.startswith("nttmul_ks_") and s not in k) == []
    # the other headers' parsers do not pick the new names up
    assert not [s for s in nttmul.rns_exported_symbols() + nttmul.bconv_exported_symbols()
                + nttmul.rnsmp_exported_symbols() + nttmul.galois_exported_symbols()
                + nttmul.exported_symbols() if "_ks_" in s]
    # and the older libraries do not hold them
    for path in ("LIB_PATH", "MAC_LIB_PATH", "RNS_LIB_PATH", "BCONV_LIB_PATH", "RNSMP_LIB_PATH",
                 "GALOIS_LIB_PATH"):
        assert not [s for s in _defined(getattr(nttmul, path)) if s.startswith("nttmul_ks_")]
    assert nttmul.KS_OPS == C.OPS


def _params(n, flags=0, q=0, psi=0):
    return nttmul._Params(n, q, psi, 1, 0, flags, 0, 0, 0, 0, 0)


def _create(lib, n, q, p, alpha, flags=0, pq=0, psi=0, L=None, K=None):
    """The status of nttmul_ks_create, and of nttmul_ks_plan with no table: the same decision."""
    h = ctypes.c_void_p()
    prm = _params(n, flags, pq, psi)
    qa = (ctypes.c_uint64 * max(1, len(q)))(*q)
    pa = (ctypes.c_uint64 * max(1, len(p)))(*p)
    L, K = len(q) if L is None else L, len(p) if K is None else K
    st = lib.nttmul_ks_create(ctypes.byref(h), ctypes.byref(prm), ctypes.sizeof(prm), qa, L, pa, K,
                              alpha)
    if st == nttmul.NTTMUL_OK:      # (only where a device is present)
        lib.nttmul_ks_destroy(h)
    else:
        assert not h.value
    plan = lib.nttmul_ks_plan(ctypes.byref(prm), ctypes.sizeof(prm), qa, L, pa, K, alpha,
                              *([None] * 6))
    if st in (nttmul.NTTMUL_EINVAL, nttmul.NTTMUL_EUNSUPPORTED):
        assert plan == st
    else:
        assert plan == nttmul.NTTMUL_OK and st in (nttmul.NTTMUL_OK, nttmul.NTTMUL_ENODEV)
    return st


def test_create_refusals_come_before_any_device_access():
    lib = nttmul.load_ks_library()
    EINVAL, EUNS = nttmul.NTTMUL_EINVAL, nttmul.NTTMUL_EUNSUPPORTED
    Q32, P32 = R.BASIS32[:2], R.BASIS32[2:]
    Q64, P64 = R.BASIS64[:2], R.BASIS64[2:]
    for n in (256, 4096, 8192, 65536):                                       # every range alike
        for Q, P in ((Q32, P32), (Q64, P64)):
            assert _create(lib, n, Q, P, 1) in (nttmul.NTTMUL_OK, nttmul.NTTMUL_ENODEV)
            assert _create(lib, n, Q, P, 1, L=0) == EINVAL
            assert _create(lib, n, Q, P, 1, K=0) == EINVAL                   # p_limbs = 0
            assert _create(lib, n, Q, P, 0) == EINVAL                        # digit_limbs = 0
            assert _create(lib, n, Q, P, 3) == EINVAL                        # digit_limbs > q_limbs
            assert _create(lib, n, Q, P, 2) in (nttmul.NTTMUL_OK, nttmul.NTTMUL_ENODEV)
            assert _create(lib, n, Q, Q[:1], 1) == EINVAL                    # a prime in both bases
            assert _create(lib, n, Q + Q[:1], P, 1) == EINVAL                # twice within Q
            assert _create(lib, n, Q, P + P, 1) == EINVAL                    # twice within P
            assert _create(lib, n, Q, P, 1, pq=D.Q31) == EINVAL              # params->q
            assert _create(lib, n, Q, P, 1, psi=3) == EINVAL                 # params->psi
            assert _create(lib, n, Q, P, 1, flags=nttmul.NTTMUL_FLAG_CYCLIC) == EUNS
        assert _create(lib, n, (D.Q31, D.Q31 + 2), P32, 1) == EINVAL         # not prime
        assert _create(lib, n, Q32, (D.Q31LO + 2,), 1) == EINVAL
        assert _create(lib, n, Q32, ((1 << 62) + 1,), 1) == EINVAL           # >= 2^62
        assert _create(lib, n, Q32, P64, 1) == EUNS                          # mixed across Q and P
        assert _create(lib, n, Q64, P32, 1) == EUNS
        assert _create(lib, n, (D.Q31, D.Q62), P32, 1) == EUNS               # mixed within Q
        assert _create(lib, n, Q64, (R.BASIS64[2], D.Q31), 1) == EUNS        # mixed within P
        assert _create(lib, n, (D.Q32,), P32, 1) == EUNS                     # [2^31, 2^32)
        assert _create(lib, n, Q32, (D.Q32,), 1) == EUNS
    # q_limbs + p_limbs > NTTMUL_RNS_MAX_LIMBS: the extended basis has to fit one mac context
    q, p = ref.bases(32, 60, 5)
    assert len(q) + len(p) == nttmul.RNS_MAX_LIMBS + 1
    for n in (256, 65536):
        assert _create(lib, n, q, p, 15) == EINVAL
        assert _create(lib, n, q, p[:4], 15) in (nttmul.NTTMUL_OK, nttmul.NTTMUL_ENODEV)
    many = list(range(3, 3 + nttmul.RNS_MAX_LIMBS + 1))
    assert _create(lib, 8192, many, P32, 1) == EINVAL                        # above the maximum
    assert _create(lib, 8192, Q32, many, 1) == EINVAL
    assert _create(lib, 8192, (D.Q31, D.Q0), P32, 1) == EINVAL               # 2n does not divide q - 1
    assert _create(lib, 2048, (D.Q31, D.Q0), P32, 1) in (nttmul.NTTMUL_OK, nttmul.NTTMUL_ENODEV)
    assert _create(lib, 10000, Q32, P32, 1) == EINVAL                        # n not a power of two
    assert _create(lib, 128, Q32, P32, 1) == EINVAL
    assert _create(lib, 131072, (D.Q31,), (D.Q31HI,), 1) == EINVAL           # 2^17 | q - 1 only
    for bits in (32, 64):                                                    # a valid n above 65536
        q18 = ref.B.primes_below(ref.TOP[bits], 1 << 18, 2)
        assert _create(lib, 131072, q18[:1], q18[1:], 1) == EUNS
    h = ctypes.c_void_p()
    prm = _params(4096)
    qa, pa = (ctypes.c_uint64 * 1)(D.Q31), (ctypes.c_uint64 * 1)(D.Q31HI)
    sz = ctypes.sizeof(prm)
    assert lib.nttmul_ks_create(None, ctypes.byref(prm), sz, qa, 1, pa, 1, 1) == EINVAL
    assert lib.nttmul_ks_create(ctypes.byref(h), None, sz, qa, 1, pa, 1, 1) == EINVAL
    assert lib.nttmul_ks_create(ctypes.byref(h), ctypes.byref(prm), 4, qa, 1, pa, 1, 1) == EINVAL
    assert lib.nttmul_ks_create(ctypes.byref(h), ctypes.byref(prm), sz, None, 1, pa, 1, 1) == EINVAL
    assert lib.nttmul_ks_create(ctypes.byref(h), ctypes.byref(prm), sz, qa, 1, None, 1, 1) == EINVAL
    # nttmul_bconv_create keeps its own limit, from this library too
    prm = _params(8192)
    assert lib.nttmul_bconv_create(ctypes.byref(h), ctypes.byref(prm), sz, qa, 1, pa, 1) == EUNS


def test_call_refusals_come_before_any_device_access():
    lib = nttmul.load_ks_library()
    EINVAL = nttmul.NTTMUL_EINVAL
    one = (ctypes.c_uint32 * 1)()
    p = ctypes.addressof(one)
    for op in C.OPS:
        assert getattr(lib, f"nttmul_ks_{op}_device")(None, p, p, 1, 0, None) == EINVAL
        assert getattr(lib, f"nttmul_ks_{op}_device")(None, None, None, 0, 0, None) == EINVAL
        assert getattr(lib, f"nttmul_ks_{op}")(None, p, p, 1) == EINVAL
    buf = ctypes.create_string_buffer(64)
    assert lib.nttmul_ks_kernel_name(None, 0, buf, len(buf)) == EINVAL
    assert lib.nttmul_ks_get_info(None, None) == EINVAL
    assert lib.nttmul_ks_last_error(None) == b""
    lib.nttmul_ks_destroy(None)


PLAN_SHAPES = ((1, 1, 1), (4, 2, 2), (5, 2, 2), (5, 3, 5), (5, 3, 1), (7, 2, 3), (60, 4, 15))


@pytest.mark.parametrize("bits", (32, 64))
def test_plan_equals_the_reference(bits):
    """Both classes; a short last digit (5 = 2 + 2 + 1, 7 = 3 + 3 + 1), alpha = 1 and alpha = L."""
    for L, K, alpha in PLAN_SHAPES:
        q, p = ref.bases(bits, L, K)
        for n in (256, 65536):
            got = nttmul.ks_plan(n, q, p, alpha)
            assert got == tuple(ref.constants(q, p, alpha)), (L, K, alpha, n)


def test_plan_with_small_moduli_and_partial_tables():
    lib = nttmul.load_ks_library()
    q, p = C.small_moduli()
    L, K, alpha = C.SMALL_SHAPE
    assert nttmul.ks_plan(256, q, p, alpha) == tuple(ref.constants(q, p, alpha))
    # a NULL table is skipped; the others are written in full and nothing past them
    prm = _params(256)
    qa, pa = (ctypes.c_uint64 * L)(*q), (ctypes.c_uint64 * K)(*p)
    dn = -(-L // alpha)
    guard = (ctypes.c_uint64 * (dn * (L + K) + 4))(*([0xDEADBEEF] * (dn * (L + K) + 4)))
    st = lib.nttmul_ks_plan(ctypes.byref(prm), ctypes.sizeof(prm), qa, L, pa, K, alpha, None, None,
                            ctypes.addressof(guard), None, None, None)
    assert st == nttmul.NTTMUL_OK
    want = [v for row in ref.gadget(q, p, alpha) for v in row]
    assert list(guard[:len(want)]) == want and list(guard[len(want):]) == [0xDEADBEEF] * 4
    with pytest.raises(nttmul.NttmulError) as ei:
        nttmul.ks_plan(256, q, p, L + 1)
    assert ei.value.status == nttmul.NTTMUL_EINVAL
    with pytest.raises(nttmul.NttmulError) as ei:
        nttmul.ks_plan(256, q, q[:1], 1)
    assert ei.value.status == nttmul.NTTMUL_EINVAL


@pytest.mark.parametrize("bits", (32, 64))
def test_moddown_constants_equal_bconv_plan(bits):
    for L in (1, 2, 3):
        for K in (1, 2, 3):
            q, p = BC.bases(bits, L, K)                  # any prime = 1 mod 2 * 4096 serves n = 4096
            _, _, _, pinv, pw, Pinv = nttmul.ks_plan(4096, q, p, 1)
            assert (pinv, pw, Pinv) == nttmul.bconv_plan(4096, p, q)


def test_key_switch_basis_is_its_own_class_on_its_own_library():
    for name in ("modup_device", "moddown_device", "modup", "moddown", "kernel_name", "close"):
        assert callable(getattr(nttmul.KeySwitchBasis, name))
    libs = (nttmul.load_library(), nttmul.load_mac_library(), nttmul.load_rns_library(),
            nttmul.load_bconv_library(), nttmul.load_rnsmp_library(), nttmul.load_galois_library(),
            nttmul.load_ks_library())
    assert len({id(x) for x in libs}) == 7
    assert libs[6]._name == nttmul.KS_LIB_PATH
    for older in libs[:6]:
        assert not hasattr(older, "nttmul_ks_create") and not hasattr(older, "nttmul_ks_plan")
    assert ctypes.sizeof(nttmul.KsInfo) == 32


def test_python_refuses_what_the_library_refuses():
    Q, P = R.BASIS32[:2], R.BASIS32[2:]
    for n in (4096, 8192):
        for args, status in (((Q, Q[:1], 1), nttmul.NTTMUL_EINVAL), ((Q, (), 1), nttmul.NTTMUL_EINVAL),
                             ((Q, P, 0), nttmul.NTTMUL_EINVAL), ((Q, P, 3), nttmul.NTTMUL_EINVAL),
                             ((Q, R.BASIS64[:1], 1), nttmul.NTTMUL_EUNSUPPORTED),
                             ((Q, (D.Q32,), 1), nttmul.NTTMUL_EUNSUPPORTED)):
            with pytest.raises(nttmul.NttmulError) as ei:
                nttmul.KeySwitchBasis(n, *args)
            assert ei.value.status == status
        with pytest.raises(nttmul.NttmulError) as ei:
            nttmul.KeySwitchBasis(n, Q, P, 1, cyclic=True)
        assert ei.value.status == nttmul.NTTMUL_EUNSUPPORTED


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="checks the no-GPU behaviour")
def test_key_switch_basis_without_a_device_fails_loudly():
    for n in (4096, 8192):
        with pytest.raises(nttmul.NttmulError) as ei:
            nttmul.KeySwitchBasis(n, R.BASIS32[:2], R.BASIS32[2:], 1)
        assert ei.value.status == nttmul.NTTMUL_ENODEV
