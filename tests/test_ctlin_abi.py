"""lib/libnttmul_ctlin.so (include/nttmul_ctlin.h) without a GPU: the header compiles as C and as
C++, the library is built, exports the whole ABI of the sixteen headers unmangled and its own
symbols in no older library, and refuses bad arguments before any device access.  The order of
combine's statuses on a live context is walked term by term by tests/sanitize/ctlin_san.cpp on
csrc/ctlin_plan.hpp, which is what the entry points call, and by tests/test_gpu_ctlin.py on a
context."""
import ctypes
import os
import shutil
import subprocess

import pytest

import nttmul
import rnsmp_cases as R

ENTRY_POINTS = ("nttmul_ctlin_create", "nttmul_ctlin_destroy", "nttmul_ctlin_last_error",
                "nttmul_ctlin_get_info", "nttmul_ctlin_combine_device", "nttmul_ctlin_combine",
                "nttmul_ctlin_tensor_device", "nttmul_ctlin_tensor", "nttmul_ctlin_kernel_name")
INCLUDE = os.path.dirname(nttmul.CTLIN_HEADER_PATH)
OLDER = ("LIB_PATH", "MAC_LIB_PATH", "RNS_LIB_PATH", "BCONV_LIB_PATH", "RNSMP_LIB_PATH",
         "GALOIS_LIB_PATH", "KS_LIB_PATH", "MACN_LIB_PATH", "HOIST_LIB_PATH", "MDNTT_LIB_PATH",
         "KSNTT_LIB_PATH", "LINTRANS_LIB_PATH", "CTMUL_LIB_PATH", "XCONV_LIB_PATH",
         "LEVEL_LIB_PATH")
EXPORTS = ("exported_symbols", "mac_exported_symbols", "rns_exported_symbols",
           "bconv_exported_symbols", "rnsmp_exported_symbols", "galois_exported_symbols",
           "ks_exported_symbols", "macn_exported_symbols", "hoist_exported_symbols",
           "mdntt_exported_symbols", "ksntt_exported_symbols", "lintrans_exported_symbols",
           "ctmul_exported_symbols", "xconv_exported_symbols", "level_exported_symbols",
           "ctlin_exported_symbols")


def _defined(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True,
                         check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if " T " in line}


@pytest.mark.parametrize("cc,std,ext", (("gcc", "-std=c11", "c"), ("g++", "-std=c++17", "cpp")))
def test_the_header_compiles_as_c_and_as_cxx(cc, std, ext, tmp_path):
    if shutil.which(cc) is None:
        pytest.skip(f"no {cc}")
    src = tmp_path / f"use.{ext}"
    src.write_text('#include "nttmul_ctlin.h"\n'
                   "int use(nttmul_ctlin *cl, void *out, const void *x, const void *w) {\n"
                   "  nttmul_ctlin_term t[NTTMUL_CTLIN_MAX_TERMS];\n"
                   "  nttmul_ctlin_info info;\n"
                   "  char name[8];\n"
                   "  t[0].x = x;\n"
                   "  t[0].w = w;\n"
                   "  t[0].kind = NTTMUL_CTLIN_PLAIN;\n"
                   "  t[0].reserved = 0;\n"
                   "  t[1].x = out;\n"
                   "  t[1].w = 0;\n"
                   "  t[1].kind = NTTMUL_CTLIN_ONE;\n"
                   "  t[1].reserved = 0;\n"
                   "  if (nttmul_ctlin_get_info(cl, &info)) return 1;\n"
                   "  if (nttmul_ctlin_kernel_name(cl, NTTMUL_CTLIN_COMBINE, NTTMUL_CTLIN_MAX_COMPS,\n"
                   "                               name, sizeof name) < 0)\n"
                   "    return 2;\n"
                   "  if (nttmul_ctlin_combine_device(cl, out, t, 2, 1, 2, 0, 0)) return 3;\n"
                   "  if (nttmul_ctlin_combine(cl, out, t, 2, 1, 2)) return 4;\n"
                   "  if (nttmul_ctlin_tensor(cl, out, x, x, 1, 1)) return 5;\n"
                   "  return nttmul_ctlin_tensor_device(cl, out, x, w, 1, 1, 0, 0) +\n"
                   "         NTTMUL_CTLIN_SCALAR + NTTMUL_CTLIN_TENSOR;\n"
                   "}\n")
    subprocess.run([cc, std, "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", INCLUDE, "-c",
                    str(src), "-o", str(tmp_path / "use.o")], check=True)


def test_ctlin_library_is_built():
    assert os.path.exists(nttmul.CTLIN_LIB_PATH), f"{nttmul.CTLIN_LIB_PATH} not built"


def test_ctlin_library_exports_all_sixteen_headers():
    have = _defined(nttmul.CTLIN_LIB_PATH)
    k = nttmul.ctlin_exported_symbols()
    assert k == sorted(ENTRY_POINTS)
    assert set(k) <= have
    assert len(EXPORTS) == 16
    for name in EXPORTS:
        syms = getattr(nttmul, name)()
        assert syms and set(syms) <= have, name
    assert not [s for s in have if s.startswith("_Z") and "nttmul_ctlin" in s]   # unmangled
    # every symbol of libnttmul_level.so is still there
    level = _defined(nttmul.LEVEL_LIB_PATH)
    assert set(nttmul.level_exported_symbols()) <= level
    assert sorted(level - have) == []
    # the library adds its nine entry points to the level library's and nothing else
    assert {s for s in have - level if s.startswith("nttmul_")} == set(k)


def test_no_older_library_exports_a_ctlin_symbol():
    for name in OLDER:
        older = _defined(getattr(nttmul, name))
        assert not older & set(ENTRY_POINTS), name
        assert not [s for s in older if "_ctlin_" in s], name


def _term(x, w, kind, reserved=0):
    return nttmul.CtLinTerm(x, w, kind, reserved)


def test_bad_arguments_are_refused_before_any_device_access():
    """A NULL context is the first status of every call, whatever else is wrong; create refuses in
    nttmul_galois_create's order."""
    lib = nttmul.load_ctlin_library()
    EINVAL = nttmul.NTTMUL_EINVAL
    one = (ctypes.c_uint64 * 1)(1)
    p = ctypes.addressof(one)
    good = (nttmul.CtLinTerm * 1)(_term(p, None, nttmul.CTLIN_ONE))
    bad = (nttmul.CtLinTerm * 1)(_term(None, p, 3, 1))
    for terms, count, comps in ((good, 1, 1), (bad, 1, 1), (None, 0, 0), (good, 17, 4)):
        assert lib.nttmul_ctlin_combine_device(None, p, terms, count, 1, comps, 0, None) == EINVAL
        assert lib.nttmul_ctlin_combine(None, p, terms, count, 1, comps) == EINVAL
        assert lib.nttmul_ctlin_combine(None, None, terms, count, 0, comps) == EINVAL
    assert lib.nttmul_ctlin_tensor_device(None, p, p, p, 1, 1, 0, None) == EINVAL
    assert lib.nttmul_ctlin_tensor(None, p, p, p, 1, 1) == EINVAL
    assert lib.nttmul_ctlin_tensor(None, None, None, None, 0, 0) == EINVAL
    assert lib.nttmul_ctlin_kernel_name(None, 0, 1, None, 0) == EINVAL
    assert lib.nttmul_ctlin_get_info(None, None) == EINVAL
    assert lib.nttmul_ctlin_last_error(None) == b""
    lib.nttmul_ctlin_destroy(None)
    # create: the handle, the params size, the basis, the degree, the moduli, then EUNSUPPORTED
    h = ctypes.c_void_p()
    q32 = (ctypes.c_uint64 * 3)(*R.BASIS32[:3])
    prm = nttmul._Params(4096, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0)
    size = ctypes.sizeof(prm)
    create = lib.nttmul_ctlin_create
    assert create(None, ctypes.byref(prm), size, q32, 3) == EINVAL
    assert create(ctypes.byref(h), None, size, q32, 3) == EINVAL
    assert create(ctypes.byref(h), ctypes.byref(prm), 4, q32, 3) == EINVAL
    assert create(ctypes.byref(h), ctypes.byref(prm), size, None, 3) == EINVAL
    assert create(ctypes.byref(h), ctypes.byref(prm), size, q32, 0) == EINVAL
    assert create(ctypes.byref(h), ctypes.byref(prm), size, q32, nttmul.RNS_MAX_LIMBS + 1) == EINVAL
    twice = (ctypes.c_uint64 * 2)(R.BASIS32[0], R.BASIS32[0])
    assert create(ctypes.byref(h), ctypes.byref(prm), size, twice, 2) == EINVAL
    odd = nttmul._Params(3000, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0)
    assert create(ctypes.byref(h), ctypes.byref(odd), size, q32, 3) == EINVAL
    cyc = nttmul._Params(4096, 0, 0, 1, 0, nttmul.NTTMUL_FLAG_CYCLIC, 0, 0, 0, 0, 0)
    assert create(ctypes.byref(h), ctypes.byref(cyc), size, q32, 3) == nttmul.NTTMUL_EUNSUPPORTED
    assert create(ctypes.byref(h), ctypes.byref(cyc), size, twice, 2) == EINVAL      # EINVAL first
    mixed = (ctypes.c_uint64 * 2)(R.BASIS32[0], R.BASIS64[0])
    assert create(ctypes.byref(h), ctypes.byref(prm), size, mixed, 2) == nttmul.NTTMUL_EUNSUPPORTED
    assert not h.value


def test_the_python_mirror_is_the_headers():
    hdr = open(nttmul.CTLIN_HEADER_PATH).read()
    assert '#include "nttmul_level.h"' in hdr
    assert f"#define NTTMUL_CTLIN_MAX_TERMS {nttmul.CTLIN_MAX_TERMS}" in hdr
    assert f"#define NTTMUL_CTLIN_MAX_COMPS {nttmul.CTLIN_MAX_COMPS}" in hdr
    for name, v in (("ONE", nttmul.CTLIN_ONE), ("SCALAR", nttmul.CTLIN_SCALAR),
                    ("PLAIN", nttmul.CTLIN_PLAIN)):
        assert f"#define NTTMUL_CTLIN_{name} {v}" in hdr
    assert nttmul.CTLIN_OPS == ("combine", "tensor")
    for i, op in enumerate(("COMBINE", "TENSOR")):
        assert f"#define NTTMUL_CTLIN_{op} {i}" in hdr
    assert ctypes.sizeof(nttmul.CtLinTerm) == 24 and ctypes.sizeof(nttmul.CtLinInfo) == 20
    assert "const void *x;" in hdr and "const void *w;" in hdr and "uint32_t reserved;" in hdr
    x, w = object(), object()
    assert nttmul.ctlin_one(x) == (x, None, 0) and nttmul.ctlin_scalar(x, w) == (x, w, 1)
    assert nttmul.ctlin_plain(x, w) == (x, w, 2)
    assert nttmul.ctlin_const_scalar(w) == (None, w, 1)
    assert nttmul.ctlin_const_plain(w) == (None, w, 2)
    new, level = nttmul.load_ctlin_library(), nttmul.load_level_library()
    assert new is not level and new._name == nttmul.CTLIN_LIB_PATH
    for older in (nttmul.load_library(), nttmul.load_ctmul_library(), level):
        assert not hasattr(older, "nttmul_ctlin_combine")
    for name in ("combine_device", "combine", "tensor_device", "tensor", "kernel_name"):
        assert callable(getattr(nttmul.NttCtLin, name))


def test_the_header_states_its_contract_and_what_it_leaves_out():
    own = open(nttmul.CTLIN_HEADER_PATH).read()
    scope = own[own.index("Out of scope"):own.index("#ifndef")]
    for word in ("per batch entry", "weight per component", "NTTMUL_CTLIN_MAX_TERMS",
                 "rotations", "key", "coefficient-order", "NTTMUL_FLAG_CYCLIC", "2^31 <= q < 2^32",
                 "multi-device", "bench.py"):
        assert word in scope, word
    status = own[own.index("Status, all decided"):own.index("Caller memory")]
    order = [status.index(w) for w in ("nttmul_galois_create's", "a NULL context", "nterms 0",
                                       "comps 0", "NULL terms", "a kind above 2",
                                       "a non-zero reserved", "ONE with a non-NULL w",
                                       "SCALAR or PLAIN with a\n * NULL w", "ONE with a NULL x",
                                       "a NULL out", "batch = 0", "NTTMUL_ENODEV",
                                       "NTTMUL_ERANGE")]
    assert order == sorted(order)
    memory = own[own.index("Caller memory"):own.index("Out of scope")]
    for word in ("alignment of their word only", "the same pointer", "overlap\n *     no input",
                 "batch * comps * L * n", "batch * 3 * L * n", "64 bits"):
        assert word in memory, word
    older = open(nttmul.CTMUL_HEADER_PATH).read()
    scope = older[older.index("Out of scope"):older.index("#ifndef")]
    assert scope.count("nttmul_ctlin.h") >= 2


def test_python_refuses_what_the_library_refuses():
    with pytest.raises(nttmul.NttmulError) as ei:
        nttmul.NttCtLin(4096, R.BASIS32[:2], cyclic=True)
    assert ei.value.status == nttmul.NTTMUL_EUNSUPPORTED
    with pytest.raises(nttmul.NttmulError) as ei:
        nttmul.NttCtLin(4096, ())
    assert ei.value.status == nttmul.NTTMUL_EINVAL


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="checks the no-GPU behaviour")
def test_the_context_without_a_device_fails_loudly():
    for n in (256, 8192):
        with pytest.raises(nttmul.NttmulError) as ei:
            nttmul.NttCtLin(n, R.BASIS32[:2])
        assert ei.value.status == nttmul.NTTMUL_ENODEV
