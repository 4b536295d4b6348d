"""lib/libnttmul_xconv.so (include/nttmul_xconv.h) without a GPU: the header compiles as C and as
C++, the library is built, exports the whole ABI of the fourteen headers unmangled, and refuses bad
arguments before any device access: every create status in nttmul_mdntt_create's order and then
the scale's, every call status a NULL context allows; the plan constants against Python integers;
the ctypes mirror against the header; valid arguments end in NTTMUL_ENODEV on a machine with no
device."""
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
import xconv_cases as C
import xconv_ref as ref

OK_OR_NODEV = (nttmul.NTTMUL_OK, nttmul.NTTMUL_ENODEV)
ENTRY_POINTS = ("create", "destroy", "last_error", "get_info", "extend_device", "moddown_device",
                "extend", "moddown", "plan", "kernel_name")
INCLUDE = os.path.dirname(nttmul.XCONV_HEADER_PATH)


def _defined(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True,
                         check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if " T " in line}


@pytest.mark.parametrize("cc,std,ext", (("gcc", "-std=c11", "c"), ("g++", "-std=c++17", "cpp")))
def test_the_header_compiles_as_c_and_as_cxx(cc, std, ext, tmp_path):
    if shutil.which(cc) is None:
        pytest.skip(f"no {cc}")
    src = tmp_path / f"use.{ext}"
    src.write_text('#include "nttmul_xconv.h"\n'
                   "int use(nttmul_xconv *h, void *c, const void *a) {\n"
                   "  nttmul_xconv_info info;\n"
                   "  char name[8];\n"
                   "  if (nttmul_xconv_get_info(h, &info)) return 1;\n"
                   "  if (nttmul_xconv_kernel_name(h, NTTMUL_XCONV_MODDOWN, name, sizeof name) < 0)\n"
                   "    return 2;\n"
                   "  if (nttmul_xconv_extend(h, c, a, 1)) return 3;\n"
                   "  return nttmul_xconv_moddown_device(h, c, a, 1, 0, 0) + (int)info.band_log2;\n"
                   "}\n")
    subprocess.run([cc, std, "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", INCLUDE, "-c",
                    str(src), "-o", str(tmp_path / "use.o")], check=True)


def test_xconv_library_is_built():
    assert os.path.exists(nttmul.XCONV_LIB_PATH), f"{nttmul.XCONV_LIB_PATH} not built"


def test_xconv_library_exports_all_fourteen_headers():
    have = _defined(nttmul.XCONV_LIB_PATH)
    k = nttmul.xconv_exported_symbols()
    assert k == sorted("nttmul_xconv_" + s for s in ENTRY_POINTS)
    assert set(k) <= have
    # every symbol of libnttmul_ctmul.so is still there
    ctmul = _defined(nttmul.CTMUL_LIB_PATH)
    assert set(nttmul.ctmul_exported_symbols()) <= ctmul
    assert sorted(ctmul - have) == []
    # the library adds the ten entry points to the ctmul library's and nothing else
    assert {s for s in have - ctmul if s.startswith("nttmul_")} == set(k)
    assert not [s for s in ctmul if "_xconv_" in s]


def _params(n, flags=0, q=0, psi=0):
    return nttmul._Params(n, q, psi, 1, 0, flags, 0, 0, 0, 0, 0)


def _create(lib, n, q, p, scale=1, flags=0, pq=0, psi=0, L=None, K=None):
    h = ctypes.c_void_p()
    prm = _params(n, flags, pq, psi)
    qa = (ctypes.c_uint64 * max(1, len(q)))(*q)
    pa = (ctypes.c_uint64 * max(1, len(p)))(*p)
    L, K = len(q) if L is None else L, len(p) if K is None else K
    st = lib.nttmul_xconv_create(ctypes.byref(h), ctypes.byref(prm), ctypes.sizeof(prm), qa, L,
                                 pa, K, scale)
    if st == nttmul.NTTMUL_OK:      # (only where a device is present)
        lib.nttmul_xconv_destroy(h)
    else:
        assert not h.value
    # the host-only plan entry point makes the same decision, without the device
    st_plan = lib.nttmul_xconv_plan(ctypes.byref(prm), ctypes.sizeof(prm), qa, L, pa, K, scale,
                                    None, None, None, None)
    assert st_plan == (nttmul.NTTMUL_OK if st in OK_OR_NODEV else st)
    if scale == 1:
        # with t = 1 nttmul_mdntt_create's status is the same decision
        md = ctypes.c_void_p()
        st_md = lib.nttmul_mdntt_create(ctypes.byref(md), ctypes.byref(prm), ctypes.sizeof(prm),
                                        qa, L, pa, K)
        if st_md == nttmul.NTTMUL_OK:
            lib.nttmul_mdntt_destroy(md)
        assert st_md == st or {st, st_md} <= set(OK_OR_NODEV)
    return st


def test_create_refusals_come_before_any_device_access():
    lib = nttmul.load_xconv_library()
    EINVAL, EUNS = nttmul.NTTMUL_EINVAL, nttmul.NTTMUL_EUNSUPPORTED
    CYC = nttmul.NTTMUL_FLAG_CYCLIC
    Q32, P32 = R.BASIS32[:2], R.BASIS32[2:]
    Q64, P64 = R.BASIS64[:2], R.BASIS64[2:]
    for n in (256, 4096, 8192, 65536):                                       # every range alike
        for Q, P in ((Q32, P32), (Q64, P64)):
            assert _create(lib, n, Q, P) in OK_OR_NODEV
            assert _create(lib, n, Q, P, 65537) in OK_OR_NODEV
            assert _create(lib, n, Q, P, (1 << 62) - 1) in OK_OR_NODEV
            assert _create(lib, n, Q, P, L=0) == EINVAL
            assert _create(lib, n, Q, P, K=0) == EINVAL
            assert _create(lib, n, Q, Q[:1]) == EINVAL                       # a prime in both bases
            assert _create(lib, n, Q + Q[:1], P) == EINVAL                   # twice within Q
            assert _create(lib, n, Q, P + P) == EINVAL                       # twice within P
            assert _create(lib, n, Q, P, pq=D.Q31) == EINVAL                 # params->q
            assert _create(lib, n, Q, P, psi=3) == EINVAL                    # params->psi
            assert _create(lib, n, Q, P, flags=CYC) == EUNS
            # the order: every EINVAL of the bases before any EUNSUPPORTED
            assert _create(lib, n, Q, P + P, flags=CYC) == EINVAL
            # the scale: 0, 2^62 and above, a multiple of some q_l (a multiple of a p_j is fine)
            assert _create(lib, n, Q, P, 0) == EINVAL
            assert _create(lib, n, Q, P, 1 << 62) == EINVAL
            assert _create(lib, n, Q, P, (1 << 64) - 1) == EINVAL
            assert _create(lib, n, Q, P, Q[1]) == EINVAL
            if 3 * Q[0] < 1 << 62:
                assert _create(lib, n, Q, P, 3 * Q[0]) == EINVAL
            assert _create(lib, n, Q, P, P[0]) in OK_OR_NODEV
            # ... after nttmul_mdntt_create's statuses, in their order
            assert _create(lib, n, Q, P, 0, flags=CYC) == EUNS
            assert _create(lib, n, Q, P + P, 0) == EINVAL
        assert _create(lib, n, (D.Q31, D.Q31 + 2), P32) == EINVAL            # not prime
        assert _create(lib, n, Q32, ((1 << 62) + 1,)) == EINVAL              # >= 2^62
        assert _create(lib, n, Q32, P64) == EUNS                             # mixed across Q and P
        assert _create(lib, n, Q32, P64, 0) == EUNS
        assert _create(lib, n, Q64, P32) == EUNS
        assert _create(lib, n, (D.Q31, D.Q62), P32) == EUNS                  # mixed within Q
        assert _create(lib, n, (D.Q32,), P32) == EUNS                        # [2^31, 2^32)
        assert _create(lib, n, (D.Q32,), (D.Q31LO + 2,)) == EINVAL           # EINVAL of P first
    q, p = ks_ref.bases(32, 60, 5)
    assert len(q) + len(p) == nttmul.RNS_MAX_LIMBS + 1
    for n in (256, 65536):
        assert _create(lib, n, q, p) == EINVAL
        assert _create(lib, n, q, p, flags=CYC) == EINVAL                    # before EUNS
        assert _create(lib, n, q, p[:4]) in OK_OR_NODEV
    assert _create(lib, 10000, Q32, P32) == EINVAL                           # n not a power of two
    assert _create(lib, 128, Q32, P32) == EINVAL
    for bits in (32, 64):                                                    # a valid n above 65536
        q18 = ks_ref.B.primes_below(ks_ref.TOP[bits], 1 << 18, 2)
        assert _create(lib, 131072, q18[:1], q18[1:]) == EUNS
    h = ctypes.c_void_p()
    prm = _params(4096)
    qa, pa = (ctypes.c_uint64 * 1)(D.Q31), (ctypes.c_uint64 * 1)(D.Q31HI)
    sz = ctypes.sizeof(prm)
    create = lib.nttmul_xconv_create
    assert create(None, ctypes.byref(prm), sz, qa, 1, pa, 1, 1) == EINVAL
    assert create(ctypes.byref(h), None, sz, qa, 1, pa, 1, 1) == EINVAL
    assert create(ctypes.byref(h), ctypes.byref(prm), 4, qa, 1, pa, 1, 1) == EINVAL
    assert create(ctypes.byref(h), ctypes.byref(prm), sz, None, 1, pa, 1, 1) == EINVAL
    assert create(ctypes.byref(h), ctypes.byref(prm), sz, qa, 1, None, 1, 1) == EINVAL


def test_call_refusals_come_before_any_device_access():
    lib = nttmul.load_xconv_library()
    EINVAL = nttmul.NTTMUL_EINVAL
    one = (ctypes.c_uint32 * 1)(1)
    p = ctypes.addressof(one)
    for op in C.OPS:
        dev = getattr(lib, f"nttmul_xconv_{op}_device")
        host = getattr(lib, f"nttmul_xconv_{op}")
        assert dev(None, p, p, 1, 0, None) == EINVAL
        assert dev(None, None, None, 0, 0, None) == EINVAL
        assert host(None, p, p, 1) == EINVAL
        assert host(None, None, None, 0) == EINVAL
    buf = ctypes.create_string_buffer(64)
    for op in (-1, 0, 1, 2):
        assert lib.nttmul_xconv_kernel_name(None, op, buf, len(buf)) == EINVAL
    assert lib.nttmul_xconv_get_info(None, None) == EINVAL
    assert lib.nttmul_xconv_last_error(None) == b""
    lib.nttmul_xconv_destroy(None)


@pytest.mark.parametrize("t", (1, 65537, 1032193, (1 << 62) - 57))
@pytest.mark.parametrize("bits", (32, 64))
@pytest.mark.parametrize("L,K", ((1, 1), (3, 2), (2, 5), (1, 63)))
def test_the_plan_constants_against_python_integers(L, K, bits, t):
    q, p = ks_ref.bases(bits, L, K)
    got = nttmul.xconv_plan(256, q, p, t)
    assert tuple(got) == tuple(ref.plan(q, p, t))
    yscale, w_ext, w_md, v = got
    assert len(yscale) == K and len(w_ext) == len(w_md) == K + 1 and len(v) == L
    with pytest.raises(nttmul.NttmulError) as ei:
        nttmul.xconv_plan(256, q, p, q[0])
    assert ei.value.status == nttmul.NTTMUL_EINVAL


def test_the_ctypes_mirror_matches_the_header():
    for name in ("extend_device", "extend", "moddown_device", "moddown", "kernel_name", "close",
                 "__enter__", "__exit__", "eps"):
        assert hasattr(nttmul.NttExactConv, name)
    new, ctmul = nttmul.load_xconv_library(), nttmul.load_ctmul_library()
    assert new is not ctmul and new._name == nttmul.XCONV_LIB_PATH
    for older in (nttmul.load_library(), nttmul.load_ks_library(), nttmul.load_hoist_library(),
                  nttmul.load_mdntt_library(), nttmul.load_ksntt_library(),
                  nttmul.load_lintrans_library(), ctmul):
        assert not hasattr(older, "nttmul_xconv_create")
    hdr = open(nttmul.XCONV_HEADER_PATH).read()
    body = re.search(r"typedef struct \{(.*?)\} nttmul_xconv_info;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [(t, nm.strip()) for t, names in re.findall(r"(uint32_t|uint64_t|int) ([\w, ]+);", body)
              for nm in names.split(",")]
    ctype = {"uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64, "int": ctypes.c_int}
    assert [(nm, ctype[t]) for t, nm in fields] == list(nttmul.XConvInfo._fields_)
    # nttmul_mdntt_info's fields, then band_log2 and scale
    assert list(nttmul.XConvInfo._fields_[:len(nttmul.MdNttInfo._fields_)]) == \
        list(nttmul.MdNttInfo._fields_)
    assert [nm for nm, _ in nttmul.XConvInfo._fields_[-2:]] == ["band_log2", "scale"]
    assert ctypes.sizeof(nttmul.XConvInfo) == 40
    assert '#include "nttmul_ctmul.h"' in hdr
    assert nttmul.XCONV_OPS == C.OPS == ("extend", "moddown")
    assert "#define NTTMUL_XCONV_EXTEND 0" in hdr and "#define NTTMUL_XCONV_MODDOWN 1" in hdr
    assert f"eps = K 2^-band_log2" in hdr and f"{C.BAND_LOG2} in this library" in hdr
    assert C.BAND_LOG2 >= C.MIN_BAND_LOG2
    plan = open(os.path.join(os.path.dirname(nttmul.PKG_DIR), os.path.basename(nttmul.PKG_DIR),
                             "csrc", "xconv_plan.hpp")).read()
    assert f"constexpr uint32_t kXcBandLog2 = {C.BAND_LOG2};" in plan


def test_the_header_states_its_contract_and_what_it_leaves_out():
    own = open(nttmul.XCONV_HEADER_PATH).read()
    scope = own[own.index("Out of scope"):own.index("#ifndef")]
    for word in ("BGV's t-correcting ModDown", "once per coefficient", "coefficient-order",
                 "NTTMUL_FLAG_CYCLIC", "2^31 <= q < 2^32", "multi-device", "bench.py"):
        assert word in scope, word
    memory = own[own.index("Caller memory"):own.index("Scratch, as")]
    for word in ("alignment of their word only", "must not overlap", "batch * L * n", "64 bits"):
        assert word in memory, word
    # the five headers that listed this as out of scope point here
    for name in ("nttmul_bconv.h", "nttmul_mdntt.h", "nttmul_ksntt.h", "nttmul_lintrans.h",
                 "nttmul_ctmul.h"):
        text = open(os.path.join(INCLUDE, name)).read()
        assert "nttmul_xconv.h" in text[text.index("Out of scope"):], name


def test_python_refuses_what_the_library_refuses():
    Q, P = R.BASIS32[:2], R.BASIS32[2:]
    for n in (4096, 8192):
        for args, status in (((Q, Q[:1]), nttmul.NTTMUL_EINVAL),
                             ((Q, P, 0), nttmul.NTTMUL_EINVAL),
                             ((Q, P, Q[0]), nttmul.NTTMUL_EINVAL),
                             ((Q, P, 1 << 62), nttmul.NTTMUL_EINVAL),
                             ((Q, P, 1 << 64), nttmul.NTTMUL_EINVAL),
                             ((Q, R.BASIS64[:1]), nttmul.NTTMUL_EUNSUPPORTED),
                             ((Q, (D.Q32,)), nttmul.NTTMUL_EUNSUPPORTED)):
            with pytest.raises(nttmul.NttmulError) as ei:
                nttmul.NttExactConv(n, *args)
            assert ei.value.status == status
        with pytest.raises(nttmul.NttmulError) as ei:
            nttmul.NttExactConv(n, Q, P, cyclic=True)
        assert ei.value.status == nttmul.NTTMUL_EUNSUPPORTED


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="checks the no-GPU behaviour")
def test_ntt_exact_conv_without_a_device_fails_loudly():
    for n in (256, 4096, 8192, 65536):
        with pytest.raises(nttmul.NttmulError) as ei:
            nttmul.NttExactConv(n, R.BASIS32[:2], R.BASIS32[2:], 65537)
        assert ei.value.status == nttmul.NTTMUL_ENODEV
