"""lib/libnttmul_level.so (include/nttmul_level.h) without a GPU: the header compiles as C and as
C++, the library is built, exports the whole ABI of the fifteen headers unmangled and its own
symbols in no older library, and refuses bad arguments before any device access.  A NULL context
is the dense call's first status and comes before every status of the view; the order of the
view's own statuses needs a context's L and K: tests/sanitize/level_san.cpp walks it on
csrc/level_plan.hpp, which is what the entry points call, and tests/test_gpu_level.py on a
context."""
import ctypes
import os
import shutil
import subprocess

import pytest

import nttmul
import rnsmp_cases as R

ENTRY_POINTS = ("nttmul_ksntt_mac_view_device", "nttmul_ksntt_mac_view",
                "nttmul_lintrans_apply_view_device", "nttmul_lintrans_apply_view",
                "nttmul_ctmul_relin_view_device", "nttmul_ctmul_relin_view",
                "nttmul_level_kernel_name")
INCLUDE = os.path.dirname(nttmul.LEVEL_HEADER_PATH)
OLDER = ("LIB_PATH", "MAC_LIB_PATH", "RNS_LIB_PATH", "BCONV_LIB_PATH", "RNSMP_LIB_PATH",
         "GALOIS_LIB_PATH", "KS_LIB_PATH", "MACN_LIB_PATH", "HOIST_LIB_PATH", "MDNTT_LIB_PATH",
         "KSNTT_LIB_PATH", "LINTRANS_LIB_PATH", "CTMUL_LIB_PATH", "XCONV_LIB_PATH")


def _defined(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True,
                         check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if " T " in line}


@pytest.mark.parametrize("cc,std,ext", (("gcc", "-std=c11", "c"), ("g++", "-std=c++17", "cpp")))
def test_the_header_compiles_as_c_and_as_cxx(cc, std, ext, tmp_path):
    if shutil.which(cc) is None:
        pytest.skip(f"no {cc}")
    src = tmp_path / f"use.{ext}"
    src.write_text('#include "nttmul_level.h"\n'
                   "int use(nttmul_ksntt *ks, nttmul_lintrans *lt, nttmul_ctmul *ct, void *c,\n"
                   "        const void *a, const uint32_t *k) {\n"
                   "  nttmul_level_view v;\n"
                   "  char name[8];\n"
                   "  v.top_q_limbs = 5;\n"
                   "  v.top_terms = 3;\n"
                   "  if (nttmul_level_kernel_name(NTTMUL_LEVEL_RELIN, 12, 64, 1, 0, name,\n"
                   "                               sizeof name) < 0)\n"
                   "    return 1;\n"
                   "  if (nttmul_ksntt_mac_view(ks, c, a, a, k, 1, 1, 1, 1, &v)) return 2;\n"
                   "  if (nttmul_lintrans_apply_view_device(lt, c, a, a, a, a, k, 1, 1, 1, 1, &v,\n"
                   "                                        0, 0))\n"
                   "    return 3;\n"
                   "  return nttmul_ctmul_relin_view_device(ct, c, a, a, a, a, 1, 1, 1, &v, 0, 0);\n"
                   "}\n")
    subprocess.run([cc, std, "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", INCLUDE, "-c",
                    str(src), "-o", str(tmp_path / "use.o")], check=True)


def test_level_library_is_built():
    assert os.path.exists(nttmul.LEVEL_LIB_PATH), f"{nttmul.LEVEL_LIB_PATH} not built"


def test_level_library_exports_all_fifteen_headers():
    have = _defined(nttmul.LEVEL_LIB_PATH)
    k = nttmul.level_exported_symbols()
    assert k == sorted(ENTRY_POINTS)
    assert set(k) <= have
    # every symbol of libnttmul_xconv.so is still there
    xconv = _defined(nttmul.XCONV_LIB_PATH)
    assert set(nttmul.xconv_exported_symbols()) <= xconv
    assert sorted(xconv - have) == []
    # the library adds the seven entry points to the xconv library's and nothing else
    assert {s for s in have - xconv if s.startswith("nttmul_")} == set(k)


def test_no_older_library_exports_a_level_symbol():
    for name in OLDER:
        older = _defined(getattr(nttmul, name))
        assert not older & set(ENTRY_POINTS), name
        assert not [s for s in older if "_level_" in s or s.endswith("_view")], name


def test_a_null_context_is_refused_before_the_view_is_looked_at():
    lib = nttmul.load_level_library()
    EINVAL = nttmul.NTTMUL_EINVAL
    one = (ctypes.c_uint32 * 1)(1)
    p = ctypes.addressof(one)
    for view in (None, ctypes.byref(nttmul.LevelView(5, 3)), ctypes.byref(nttmul.LevelView(0, 0))):
        assert lib.nttmul_ksntt_mac_view_device(None, p, p, p, one, 1, 1, 1, 1, view, 0,
                                                None) == EINVAL
        assert lib.nttmul_ksntt_mac_view(None, p, p, p, one, 1, 1, 1, 1, view) == EINVAL
        assert lib.nttmul_ksntt_mac_view(None, None, None, None, None, 0, 0, 0, 0, view) == EINVAL
        assert lib.nttmul_lintrans_apply_view_device(None, p, p, p, p, p, one, 1, 1, 1, 1, view,
                                                     0, None) == EINVAL
        assert lib.nttmul_lintrans_apply_view(None, p, p, p, None, None, one, 1, 1, 1, 1,
                                              view) == EINVAL
        assert lib.nttmul_ctmul_relin_view_device(None, p, p, p, p, p, 1, 1, 1, view, 0,
                                                  None) == EINVAL
        assert lib.nttmul_ctmul_relin_view(None, p, p, p, p, p, 1, 1, 1, view) == EINVAL
        assert lib.nttmul_ctmul_relin_view(None, None, None, None, None, None, 0, 0, 0,
                                           view) == EINVAL


def test_kernel_name_needs_no_context_and_names_every_instantiation():
    lib = nttmul.load_level_library()
    EINVAL = nttmul.NTTMUL_EINVAL
    buf = ctypes.create_string_buffer(64)
    name = lib.nttmul_level_kernel_name
    for op in (-1, 3):
        assert name(op, 12, 32, 1, 0, buf, len(buf)) == EINVAL
    for logn in (7, 17):
        assert name(0, logn, 32, 1, 0, buf, len(buf)) == EINVAL
    for bits in (0, 16, 48):
        assert name(0, 12, bits, 1, 0, buf, len(buf)) == EINVAL
    for comps in (0, 3):
        assert name(0, 12, 32, comps, 0, buf, len(buf)) == EINVAL
        assert name(1, 12, 32, comps, 0, buf, len(buf)) == EINVAL
        assert name(2, 12, 32, comps, 0, buf, len(buf)) > 0        # relin has no comps
    assert name(0, 12, 32, 1, 0, None, 8) == EINVAL
    for bits, cls in ((32, "Arith32P,u32"), (64, "Arith64,u64")):
        for logn in (8, 12, 13, 16):
            for comps in (1, 2):
                assert nttmul.level_kernel_name("mac", logn, bits, comps) == \
                    f"k_level_mac<{cls},{comps}>"
                for w in (0, 1):
                    assert nttmul.level_kernel_name("lintrans", logn, bits, comps, bool(w)) == \
                        f"k_level_lintrans<{cls},{comps},{w}>"
            assert nttmul.level_kernel_name("relin", logn, bits) == f"k_level_relin<{cls}>"
    # the untruncated length with no buffer, and truncation
    full = name(2, 12, 64, 1, 0, None, 0)
    assert full == len("k_level_relin<Arith64,u64>")
    small = ctypes.create_string_buffer(8)
    assert name(2, 12, 64, 1, 0, small, len(small)) == full and small.value == b"k_level"


def test_the_level_classes_are_their_parents_on_the_level_library():
    for cls, parent, names in ((nttmul.NttLevelKeySwitch, nttmul.NttKeySwitch, ("mac", "mac_device")),
                               (nttmul.NttLevelLinTrans, nttmul.NttLinTrans,
                                ("apply", "apply_device")),
                               (nttmul.NttLevelCtMul, nttmul.NttCtMul, ("relin", "relin_device"))):
        assert issubclass(cls, parent)
        assert cls._library() is nttmul.load_level_library()
        assert parent._library() is not nttmul.load_level_library()
        import inspect
        for name in names:
            assert "view" in inspect.signature(getattr(cls, name)).parameters
            assert "view" not in inspect.signature(getattr(parent, name)).parameters
    new, xconv = nttmul.load_level_library(), nttmul.load_xconv_library()
    assert new is not xconv and new._name == nttmul.LEVEL_LIB_PATH
    for older in (nttmul.load_library(), nttmul.load_ksntt_library(),
                  nttmul.load_lintrans_library(), nttmul.load_ctmul_library(), xconv):
        assert not hasattr(older, "nttmul_level_kernel_name")
        assert not hasattr(older, "nttmul_ksntt_mac_view")
    assert ctypes.sizeof(nttmul.LevelView) == 8
    hdr = open(nttmul.LEVEL_HEADER_PATH).read()
    assert "uint32_t top_q_limbs;" in hdr and "uint32_t top_terms;" in hdr
    assert '#include "nttmul_xconv.h"' in hdr
    assert nttmul.LEVEL_OPS == ("mac", "lintrans", "relin")
    for i, op in enumerate(("MAC", "LINTRANS", "RELIN")):
        assert f"#define NTTMUL_LEVEL_{op} {i}" in hdr


def test_the_header_states_its_contract_and_what_it_leaves_out():
    own = open(nttmul.LEVEL_HEADER_PATH).read()
    scope = own[own.index("Out of scope"):own.index("#ifndef")]
    for word in ("coefficient-output chains", "nttmul_rns_macn_ntt", "nttmul_rns_hoist_ntt",
                 "sharing twiddles", "bench.py"):
        assert word in scope, word
    promise = own[own.index("The caller guarantees"):own.index("nttmul_ksntt_mac_view  ")]
    for word in ("cannot check", "first L primes", "chain's P"):
        assert word in promise, word
    status = own[own.index("Status, all decided"):own.index("Caller memory")]
    order = [status.index(w) for w in ("the dense call's", "a NULL view", "top_q_limbs below",
                                       "top_q_limbs + K above", "top_terms below", "batch = 0",
                                       "NTTMUL_ENODEV", "NTTMUL_ERANGE")]
    assert order == sorted(order)
    memory = own[own.index("Caller memory"):own.index("Out of scope")]
    for word in ("alignment of their word only", "overlap no input", "viewed operands are never",
                 "64 bits"):
        assert word in memory, word


def test_python_refuses_what_the_library_refuses():
    Q, P = R.BASIS32[:2], R.BASIS32[2:]
    for make in (lambda **kw: nttmul.NttLevelKeySwitch(4096, Q, P, 1, **kw),
                 lambda **kw: nttmul.NttLevelLinTrans(4096, Q, P, **kw),
                 lambda **kw: nttmul.NttLevelCtMul(4096, Q, P, **kw)):
        with pytest.raises(nttmul.NttmulError) as ei:
            make(cyclic=True)
        assert ei.value.status == nttmul.NTTMUL_EUNSUPPORTED


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="checks the no-GPU behaviour")
def test_the_level_classes_without_a_device_fail_loudly():
    Q, P = R.BASIS32[:2], R.BASIS32[2:]
    for n in (256, 8192):
        for make in (lambda: nttmul.NttLevelKeySwitch(n, Q, P, 1),
                     lambda: nttmul.NttLevelLinTrans(n, Q, P),
                     lambda: nttmul.NttLevelCtMul(n, Q, P)):
            with pytest.raises(nttmul.NttmulError) as ei:
                make()
            assert ei.value.status == nttmul.NTTMUL_ENODEV
