"""lib/libnttmul_ctmul.so (include/nttmul_ctmul.h) without a GPU: the header compiles as C and as
C++, the library is built, exports the whole ABI of the thirteen headers unmangled, and refuses bad
arguments before any device access: every create status in nttmul_lintrans_create's order, and
every call status a NULL context allows (the order of the calls' other statuses needs a context:
tests/sanitize/ctmul_san.cpp walks it on csrc/ctmul_plan.hpp, which is what the entry points call);
valid arguments end in NTTMUL_ENODEV on a machine with no device."""
import ctypes
import os
import shutil
import subprocess

import pytest

import dispatch_cases as D
import ks_ref as ref
import nttmul
import rnsmp_cases as R

OK_OR_NODEV = (nttmul.NTTMUL_OK, nttmul.NTTMUL_ENODEV)
ENTRY_POINTS = ("create", "destroy", "last_error", "get_info", "high_device", "high",
                "relin_device", "relin", "kernel_name")
INCLUDE = os.path.dirname(nttmul.CTMUL_HEADER_PATH)


def _defined(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True,
                         check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if " T " in line}


@pytest.mark.parametrize("cc,std,ext", (("gcc", "-std=c11", "c"), ("g++", "-std=c++17", "cpp")))
def test_the_header_compiles_as_c_and_as_cxx(cc, std, ext, tmp_path):
    if shutil.which(cc) is None:
        pytest.skip(f"no {cc}")
    src = tmp_path / f"use.{ext}"
    src.write_text('#include "nttmul_ctmul.h"\n'
                   "int use(nttmul_ctmul *h, void *c, const void *a) {\n"
                   "  nttmul_ctmul_info info;\n"
                   "  char name[8];\n"
                   "  if (nttmul_ctmul_get_info(h, &info)) return 1;\n"
                   "  if (nttmul_ctmul_kernel_name(h, NTTMUL_CTMUL_RELIN, name, sizeof name) < 0)\n"
                   "    return 2;\n"
                   "  if (nttmul_ctmul_high(h, c, a, a, 1, 1)) return 3;\n"
                   "  return nttmul_ctmul_relin_device(h, c, a, a, a, a, 1, 1, 1, 0, 0);\n"
                   "}\n")
    subprocess.run([cc, std, "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", INCLUDE, "-c",
                    str(src), "-o", str(tmp_path / "use.o")], check=True)


def test_ctmul_library_is_built():
    assert os.path.exists(nttmul.CTMUL_LIB_PATH), f"{nttmul.CTMUL_LIB_PATH} not built"


def test_ctmul_library_exports_all_thirteen_headers():
    have = _defined(nttmul.CTMUL_LIB_PATH)
    k = nttmul.ctmul_exported_symbols()
    assert k == sorted("nttmul_ctmul_" + s for s in ENTRY_POINTS)
    assert set(k) <= have
    # every symbol of libnttmul_lintrans.so is still there
    lintrans = _defined(nttmul.LINTRANS_LIB_PATH)
    assert set(nttmul.lintrans_exported_symbols()) <= lintrans
    assert sorted(lintrans - have) == []
    # the library adds the nine entry points to the lintrans library's and nothing else
    assert {s for s in have - lintrans if s.startswith("nttmul_")} == set(k)
    assert not [s for s in lintrans if "_ctmul_" in s]


def _params(n, flags=0, q=0, psi=0):
    return nttmul._Params(n, q, psi, 1, 0, flags, 0, 0, 0, 0, 0)


def _create(lib, n, q, p, flags=0, pq=0, psi=0, L=None, K=None):
    h = ctypes.c_void_p()
    prm = _params(n, flags, pq, psi)
    qa = (ctypes.c_uint64 * max(1, len(q)))(*q)
    pa = (ctypes.c_uint64 * max(1, len(p)))(*p)
    L, K = len(q) if L is None else L, len(p) if K is None else K
    st = lib.nttmul_ctmul_create(ctypes.byref(h), ctypes.byref(prm), ctypes.sizeof(prm), qa, L,
                                 pa, K)
    if st == nttmul.NTTMUL_OK:      # (only where a device is present)
        lib.nttmul_ctmul_destroy(h)
    else:
        assert not h.value
    # nttmul_lintrans_create's status is the same decision
    lt = ctypes.c_void_p()
    st_lt = lib.nttmul_lintrans_create(ctypes.byref(lt), ctypes.byref(prm), ctypes.sizeof(prm),
                                       qa, L, pa, K)
    if st_lt == nttmul.NTTMUL_OK:
        lib.nttmul_lintrans_destroy(lt)
    assert st_lt == st or {st, st_lt} <= set(OK_OR_NODEV)
    return st


def test_create_refusals_come_before_any_device_access():
    lib = nttmul.load_ctmul_library()
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
    create = lib.nttmul_ctmul_create
    assert create(None, ctypes.byref(prm), sz, qa, 1, pa, 1) == EINVAL
    assert create(ctypes.byref(h), None, sz, qa, 1, pa, 1) == EINVAL
    assert create(ctypes.byref(h), ctypes.byref(prm), 4, qa, 1, pa, 1) == EINVAL
    assert create(ctypes.byref(h), ctypes.byref(prm), sz, None, 1, pa, 1) == EINVAL
    assert create(ctypes.byref(h), ctypes.byref(prm), sz, qa, 1, None, 1) == EINVAL


def test_call_refusals_come_before_any_device_access():
    lib = nttmul.load_ctmul_library()
    EINVAL = nttmul.NTTMUL_EINVAL
    one = (ctypes.c_uint32 * 1)(1)
    p = ctypes.addressof(one)
    assert lib.nttmul_ctmul_high_device(None, p, p, p, 1, 1, 0, None) == EINVAL
    assert lib.nttmul_ctmul_high_device(None, None, None, None, 0, 1, 0, None) == EINVAL
    assert lib.nttmul_ctmul_high(None, p, p, p, 1, 1) == EINVAL
    assert lib.nttmul_ctmul_high(None, None, None, None, 0, 0) == EINVAL
    assert lib.nttmul_ctmul_relin_device(None, p, p, p, p, p, 1, 1, 1, 0, None) == EINVAL
    assert lib.nttmul_ctmul_relin_device(None, None, None, None, None, None, 0, 1, 1, 0,
                                         None) == EINVAL
    assert lib.nttmul_ctmul_relin(None, p, p, p, p, p, 1, 1, 1) == EINVAL
    assert lib.nttmul_ctmul_relin(None, None, None, None, None, None, 0, 0, 0) == EINVAL
    buf = ctypes.create_string_buffer(64)
    for op in (-1, 0, 1, 2):
        assert lib.nttmul_ctmul_kernel_name(None, op, buf, len(buf)) == EINVAL
    assert lib.nttmul_ctmul_get_info(None, None) == EINVAL
    assert lib.nttmul_ctmul_last_error(None) == b""
    lib.nttmul_ctmul_destroy(None)


def test_ntt_ct_mul_is_its_own_class_on_its_own_library():
    for name in ("high_device", "high", "relin_device", "relin", "kernel_name", "close",
                 "__enter__", "__exit__"):
        assert callable(getattr(nttmul.NttCtMul, name))
    new, lintrans = nttmul.load_ctmul_library(), nttmul.load_lintrans_library()
    assert new is not lintrans and new._name == nttmul.CTMUL_LIB_PATH
    for older in (nttmul.load_library(), nttmul.load_ks_library(), nttmul.load_hoist_library(),
                  nttmul.load_mdntt_library(), nttmul.load_ksntt_library(), lintrans):
        assert not hasattr(older, "nttmul_ctmul_create")
    assert ctypes.sizeof(nttmul.CtMulInfo) == 24
    hdr = open(nttmul.CTMUL_HEADER_PATH).read()
    assert "uint32_t n, logn, q_limbs, p_limbs;" in hdr and '#include "nttmul_lintrans.h"' in hdr
    assert nttmul.CTMUL_OPS == ("high", "relin")
    assert "#define NTTMUL_CTMUL_HIGH 0" in hdr and "#define NTTMUL_CTMUL_RELIN 1" in hdr


def test_the_header_states_its_contract_and_what_it_leaves_out():
    own = open(nttmul.CTMUL_HEADER_PATH).read()
    scope = own[own.index("Out of scope"):own.index("#ifndef")]
    for word in ("nttmul_ksntt_modup's inverse kernels", "per batch entry",
                 "ciphertext x plaintext", "three-component", "rounding in ModDown",
                 "exact conversion", "NTTMUL_FLAG_CYCLIC", "2^31 <= q < 2^32", "multi-device",
                 "bench.py"):
        assert word in scope, word
    memory = own[own.index("Caller memory"):own.index("Out of scope")]
    for word in ("alignment of their word only", "overlap no input", "alias each other",
                 "batch * L * n", "batch * 2 * M * n", "64 bits"):
        assert word in memory, word
    status = own[own.index("Status, all decided"):own.index("Caller memory")]
    order = [status.index(w) for w in ("a NULL context", "pairs = 0", "terms = 0",
                                       "a NULL operand", "batch = 0", "NTTMUL_ENODEV",
                                       "NTTMUL_ERANGE")]
    assert order == sorted(order)
    assert "nttmul_lintrans_apply with" in own            # the form without a tensor term


def test_python_refuses_what_the_library_refuses():
    Q, P = R.BASIS32[:2], R.BASIS32[2:]
    for n in (4096, 8192):
        for args, status in (((Q, Q[:1]), nttmul.NTTMUL_EINVAL),
                             ((Q, R.BASIS64[:1]), nttmul.NTTMUL_EUNSUPPORTED),
                             ((Q, (D.Q32,)), nttmul.NTTMUL_EUNSUPPORTED)):
            with pytest.raises(nttmul.NttmulError) as ei:
                nttmul.NttCtMul(n, *args)
            assert ei.value.status == status
        with pytest.raises(nttmul.NttmulError) as ei:
            nttmul.NttCtMul(n, Q, P, cyclic=True)
        assert ei.value.status == nttmul.NTTMUL_EUNSUPPORTED


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="checks the no-GPU behaviour")
def test_ntt_ct_mul_without_a_device_fails_loudly():
    for n in (256, 4096, 8192, 65536):
        with pytest.raises(nttmul.NttmulError) as ei:
            nttmul.NttCtMul(n, R.BASIS32[:2], R.BASIS32[2:])
        assert ei.value.status == nttmul.NTTMUL_ENODEV
