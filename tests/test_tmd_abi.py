"""lib/libnttmul_tmd.so (include/nttmul_tmd.h) without a GPU: the header compiles as C and as
C++, the library is built, exports the whole ABI of the seventeen headers unmangled, and refuses
bad arguments before any device access: every create status in nttmul_mdntt_create's order and
then the plaintext modulus' in the order the header states, every call status a NULL context
allows, batch = 0; the plan constants and msg_factor against Python integers; the ctypes mirror
against the header; valid arguments end in NTTMUL_ENODEV on a machine with no device."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

import dispatch_cases as D
import ks_ref
import nttmul
import rnsmp_cases as R
import tmd_cases as C
import tmd_ref as ref

OK_OR_NODEV = (nttmul.NTTMUL_OK, nttmul.NTTMUL_ENODEV)
ENTRY_POINTS = ("create", "destroy", "last_error", "get_info", "moddown_device", "moddown", "plan",
                "kernel_name")
INCLUDE = os.path.dirname(nttmul.TMD_HEADER_PATH)


def _defined(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True,
                         check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if " T " in line}


@pytest.mark.parametrize("cc,std,ext", (("gcc", "-std=c11", "c"), ("g++", "-std=c++17", "cpp")))
def test_the_header_compiles_as_c_and_as_cxx(cc, std, ext, tmp_path):
    if shutil.which(cc) is None:
        pytest.skip(f"no {cc}")
    src = tmp_path / f"use.{ext}"
    src.write_text('#include "nttmul_tmd.h"\n'
                   "int use(nttmul_tmd *h, void *c, const void *a) {\n"
                   "  nttmul_tmd_info info;\n"
                   "  char name[8];\n"
                   "  if (nttmul_tmd_get_info(h, &info)) return 1;\n"
                   "  if (nttmul_tmd_kernel_name(h, name, sizeof name) < 0) return 2;\n"
                   "  if (nttmul_tmd_moddown(h, c, a, 1)) return 3;\n"
                   "  return nttmul_tmd_moddown_device(h, c, a, 1, 0, 0) + (int)info.msg_factor;\n"
                   "}\n")
    subprocess.run([cc, std, "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", INCLUDE, "-c",
                    str(src), "-o", str(tmp_path / "use.o")], check=True)


def test_tmd_library_is_built():
    assert os.path.exists(nttmul.TMD_LIB_PATH), f"{nttmul.TMD_LIB_PATH} not built"


def test_tmd_library_exports_all_seventeen_headers():
    have = _defined(nttmul.TMD_LIB_PATH)
    k = nttmul.tmd_exported_symbols()
    assert k == sorted("nttmul_tmd_" + s for s in ENTRY_POINTS)
    assert set(k) <= have
    # every symbol of libnttmul_ctlin.so is still there
    ctlin = _defined(nttmul.CTLIN_LIB_PATH)
    assert set(nttmul.ctlin_exported_symbols()) <= ctlin
    assert sorted(ctlin - have) == []
    # the library adds the eight entry points to the ctlin library's and nothing else
    assert {s for s in have - ctlin if s.startswith("nttmul_")} == set(k)
    assert not [s for s in ctlin if "_tmd_" in s]


def _params(n, flags=0, q=0, psi=0):
    return nttmul._Params(n, q, psi, 1, 0, flags, 0, 0, 0, 0, 0)


def _create(lib, n, q, p, t=65537, flags=0, pq=0, psi=0, L=None, K=None):
    h = ctypes.c_void_p()
    prm = _params(n, flags, pq, psi)
    qa = (ctypes.c_uint64 * max(1, len(q)))(*q)
    pa = (ctypes.c_uint64 * max(1, len(p)))(*p)
    L, K = len(q) if L is None else L, len(p) if K is None else K
    st = lib.nttmul_tmd_create(ctypes.byref(h), ctypes.byref(prm), ctypes.sizeof(prm), qa, L, pa,
                               K, t)
    if st == nttmul.NTTMUL_OK:      # (only where a device is present)
        lib.nttmul_tmd_destroy(h)
    else:
        assert not h.value
    # the host-only plan entry point makes the same decision, without the device
    st_plan = lib.nttmul_tmd_plan(ctypes.byref(prm), ctypes.sizeof(prm), qa, L, pa, K, t,
                                  None, None, None, None, None)
    assert st_plan == (nttmul.NTTMUL_OK if st in OK_OR_NODEV else st)
    return st


def _md_status(lib, n, q, p, flags=0):
    """nttmul_mdntt_create's status for the same bases."""
    h = ctypes.c_void_p()
    prm = _params(n, flags)
    qa = (ctypes.c_uint64 * max(1, len(q)))(*q)
    pa = (ctypes.c_uint64 * max(1, len(p)))(*p)
    st = lib.nttmul_mdntt_create(ctypes.byref(h), ctypes.byref(prm), ctypes.sizeof(prm), qa,
                                 len(q), pa, len(p))
    if st == nttmul.NTTMUL_OK:
        lib.nttmul_mdntt_destroy(h)
    return st


def test_create_refusals_come_before_any_device_access():
    lib = nttmul.load_tmd_library()
    EINVAL, EUNS = nttmul.NTTMUL_EINVAL, nttmul.NTTMUL_EUNSUPPORTED
    CYC = nttmul.NTTMUL_FLAG_CYCLIC
    Q32, P32 = R.BASIS32[:2], R.BASIS32[2:]
    Q64, P64 = R.BASIS64[:2], R.BASIS64[2:]
    for n in (256, 4096, 8192, 65536):                                       # every range alike
        for (Q, P), bits in (((Q32, P32), 32), ((Q64, P64), 64)):
            top = C.T_BOUND[bits]
            for t in C.plain_moduli(bits):
                assert _create(lib, n, Q, P, t) in OK_OR_NODEV
            # 1. nttmul_mdntt_create's statuses, in its order
            assert _create(lib, n, Q, P, L=0) == EINVAL
            assert _create(lib, n, Q, P, K=0) == EINVAL
            assert _create(lib, n, Q, Q[:1]) == EINVAL                       # a prime in both bases
            assert _create(lib, n, Q + Q[:1], P) == EINVAL                   # twice within Q
            assert _create(lib, n, Q, P, pq=D.Q31) == EINVAL                 # params->q
            assert _create(lib, n, Q, P, psi=3) == EINVAL                    # params->psi
            assert _create(lib, n, Q, P, flags=CYC) == EUNS
            assert _create(lib, n, Q, P + P, flags=CYC) == EINVAL
            for bad_t in (0, 2, 4, top, Q[0]):                               # ... before any of t's
                assert _create(lib, n, Q, P, bad_t, flags=CYC) == EUNS == _md_status(lib, n, Q, P, CYC)
                assert _create(lib, n, Q, P + P, bad_t) == EINVAL == _md_status(lib, n, Q, P + P)
            # 2. t < 3: EINVAL, also for the even ones among them
            for t in (0, 1, 2):
                assert _create(lib, n, Q, P, t) == EINVAL
            # 3. an even t: EUNSUPPORTED, also at or above the class bound
            for t in (4, 65536, top - 2, top, top + 2, (1 << 64) - 2):
                assert _create(lib, n, Q, P, t) == EUNS
            # 4. an odd t at or above the class bound: EINVAL, also a multiple of a modulus
            for t in (top + 1, top + 3, (1 << 64) - 1):
                assert _create(lib, n, Q, P, t) == EINVAL
            assert _create(lib, n, Q, P, top - 1) in OK_OR_NODEV             # the largest
            # 5. t = 0 modulo some p_j or q_l
            for m in Q + P:
                for f in (1, 3):
                    if f * m < top:
                        assert _create(lib, n, Q, P, f * m) == EINVAL
        assert _create(lib, n, (D.Q31, D.Q31 + 2), P32) == EINVAL            # not prime
        assert _create(lib, n, Q32, P64) == EUNS                             # mixed across Q and P
        assert _create(lib, n, Q32, P64, 2) == EUNS                          # before t < 3
        assert _create(lib, n, (D.Q32,), P32) == EUNS                        # [2^31, 2^32)
        # 32-bit words: an odd t in [2^31, 2^62) is valid on 64-bit words only
        assert _create(lib, n, Q32, P32, (1 << 31) + 1) == EINVAL
        assert _create(lib, n, Q64, P64, (1 << 31) + 1) in OK_OR_NODEV
    q, p = ks_ref.bases(32, 60, 5)
    assert len(q) + len(p) == nttmul.RNS_MAX_LIMBS + 1
    assert _create(lib, 256, q, p) == EINVAL
    assert _create(lib, 256, q, p[:4]) in OK_OR_NODEV
    assert _create(lib, 10000, Q32, P32) == EINVAL                           # n not a power of two
    for bits in (32, 64):                                                    # a valid n above 65536
        q18 = ks_ref.B.primes_below(ks_ref.TOP[bits], 1 << 18, 2)
        assert _create(lib, 131072, q18[:1], q18[1:]) == EUNS
    h = ctypes.c_void_p()
    prm = _params(4096)
    qa, pa = (ctypes.c_uint64 * 1)(D.Q31), (ctypes.c_uint64 * 1)(D.Q31HI)
    sz = ctypes.sizeof(prm)
    create = lib.nttmul_tmd_create
    assert create(None, ctypes.byref(prm), sz, qa, 1, pa, 1, 3) == EINVAL
    assert create(ctypes.byref(h), None, sz, qa, 1, pa, 1, 3) == EINVAL
    assert create(ctypes.byref(h), ctypes.byref(prm), 4, qa, 1, pa, 1, 3) == EINVAL
    assert create(ctypes.byref(h), ctypes.byref(prm), sz, None, 1, pa, 1, 3) == EINVAL
    assert create(ctypes.byref(h), ctypes.byref(prm), sz, qa, 1, None, 1, 3) == EINVAL


def test_call_refusals_come_before_any_device_access():
    lib = nttmul.load_tmd_library()
    EINVAL = nttmul.NTTMUL_EINVAL
    one = (ctypes.c_uint32 * 1)(1)
    p = ctypes.addressof(one)
    dev, host = lib.nttmul_tmd_moddown_device, lib.nttmul_tmd_moddown
    assert dev(None, p, p, 1, 0, None) == EINVAL
    assert dev(None, None, None, 0, 0, None) == EINVAL                       # batch = 0, no context
    assert host(None, p, p, 1) == EINVAL
    assert host(None, None, None, 0) == EINVAL
    buf = ctypes.create_string_buffer(64)
    assert lib.nttmul_tmd_kernel_name(None, buf, len(buf)) == EINVAL
    assert lib.nttmul_tmd_get_info(None, None) == EINVAL
    assert lib.nttmul_tmd_last_error(None) == b""
    lib.nttmul_tmd_destroy(None)


@pytest.mark.parametrize("which", range(3))
@pytest.mark.parametrize("bits", (32, 64))
@pytest.mark.parametrize("L,K", ((1, 1), (3, 2), (2, 5), (1, 63)))
def test_the_plan_constants_against_python_integers(L, K, bits, which):
    q, p = ks_ref.bases(bits, L, K)
    t = C.plain_moduli(bits)[which]
    got = nttmul.tmd_plan(q, p, t)
    assert tuple(got) == tuple(ref.plan(q, p, t))
    yscale, g, w, v, mf = got
    assert len(yscale) == len(g) == K and len(w) == K + 2 and len(v) == L
    P = 1
    for m in p:
        P *= m
    assert mf * P % t == 1 and all((gj * m + 1) % t == 0 for gj, m in zip(g, p))
    with pytest.raises(nttmul.NttmulError) as ei:
        nttmul.tmd_plan(q, p, 4)
    assert ei.value.status == nttmul.NTTMUL_EUNSUPPORTED


def test_a_composite_plaintext_modulus():
    """t need not be prime: the inverses modulo t come from Euclid's algorithm."""
    q, p = ks_ref.bases(64, 2, 3)
    for t in (9, 3 * 5 * 7 * 11, 65537 * 3, (1 << 62) - 1):
        assert tuple(nttmul.tmd_plan(q, p, t)) == tuple(ref.plan(q, p, t))


def test_the_ctypes_mirror_matches_the_header():
    for name in ("moddown_device", "moddown", "kernel_name", "close", "__enter__", "__exit__"):
        assert hasattr(nttmul.NttPlainModDown, name)
    new, ctlin = nttmul.load_tmd_library(), nttmul.load_ctlin_library()
    assert new is not ctlin and new._name == nttmul.TMD_LIB_PATH
    for older in (nttmul.load_library(), nttmul.load_mdntt_library(), nttmul.load_xconv_library(),
                  nttmul.load_level_library(), ctlin):
        assert not hasattr(older, "nttmul_tmd_create")
    hdr = open(nttmul.TMD_HEADER_PATH).read()
    body = re.search(r"typedef struct \{(.*?)\} nttmul_tmd_info;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [(t, nm.strip()) for t, names in re.findall(r"(uint32_t|uint64_t|int) ([\w, ]+);", body)
              for nm in names.split(",")]
    ctype = {"uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64, "int": ctypes.c_int}
    assert [(nm, ctype[t]) for t, nm in fields] == list(nttmul.TmdInfo._fields_)
    # nttmul_mdntt_info's fields, then t and msg_factor
    assert list(nttmul.TmdInfo._fields_[:len(nttmul.MdNttInfo._fields_)]) == \
        list(nttmul.MdNttInfo._fields_)
    assert [nm for nm, _ in nttmul.TmdInfo._fields_[-2:]] == ["t", "msg_factor"]
    assert ctypes.sizeof(nttmul.TmdInfo) == 48
    assert '#include "nttmul_ctlin.h"' in hdr
    plan = open(os.path.join(nttmul.PKG_DIR, "csrc", "tmd_plan.hpp")).read()
    assert "word_bits == 32 ? (uint64_t)1 << 31 : (uint64_t)1 << 62" in plan
    assert C.T_BOUND == ref.T_BOUND == {32: 1 << 31, 64: 1 << 62}


def test_the_header_states_its_contract_and_what_it_leaves_out():
    own = open(nttmul.TMD_HEADER_PATH).read()
    scope = own[own.index("Out of scope"):own.index("#ifndef")]
    for word in ("even t", "centred variant", "coefficient-order", "once per coefficient",
                 "NTTMUL_FLAG_CYCLIC", "2^31 <= q < 2^32", "multi-device", "bench.py"):
        assert word in scope, word
    memory = own[own.index("Caller memory"):own.index("Scratch, as")]
    for word in ("alignment of their word only", "must not overlap", "batch * L * n", "64 bits"):
        assert word in memory, word
    for word in ("msg_factor", "P out = X (mod t)", "K = 1", "BGV rescale", "section 2k",
                 "K + (t + 1) / 2"):
        assert word in own, word
    # the headers that listed this as out of scope, or called the floor form BGV's, point here
    for name in ("nttmul_xconv.h", "nttmul_mdntt.h"):
        assert "nttmul_tmd.h" in open(os.path.join(INCLUDE, name)).read(), name
    assert "CKKS / BGV rescale" not in open(os.path.join(INCLUDE, "nttmul_mdntt.h")).read()


def test_python_refuses_what_the_library_refuses():
    Q, P = R.BASIS32[:2], R.BASIS32[2:]
    for n in (4096, 8192):
        for args, status in (((Q, Q[:1], 3), nttmul.NTTMUL_EINVAL),
                             ((Q, P, 1), nttmul.NTTMUL_EINVAL),
                             ((Q, P, 4), nttmul.NTTMUL_EUNSUPPORTED),
                             ((Q, P, Q[0]), nttmul.NTTMUL_EINVAL),
                             ((Q, P, (1 << 31) + 1), nttmul.NTTMUL_EINVAL),
                             ((Q, P, 1 << 64), nttmul.NTTMUL_EINVAL),
                             ((Q, R.BASIS64[:1], 3), nttmul.NTTMUL_EUNSUPPORTED)):
            with pytest.raises(nttmul.NttmulError) as ei:
                nttmul.NttPlainModDown(n, *args)
            assert ei.value.status == status
        with pytest.raises(nttmul.NttmulError) as ei:
            nttmul.NttPlainModDown(n, Q, P, 3, cyclic=True)
        assert ei.value.status == nttmul.NTTMUL_EUNSUPPORTED


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="checks the no-GPU behaviour")
def test_ntt_plain_moddown_without_a_device_fails_loudly():
    for n in (256, 4096, 8192, 65536):
        with pytest.raises(nttmul.NttmulError) as ei:
            nttmul.NttPlainModDown(n, R.BASIS32[:2], R.BASIS32[2:], 65537)
        assert ei.value.status == nttmul.NTTMUL_ENODEV
