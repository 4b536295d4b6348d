"""lib/libnttmul_hoist.so (include/nttmul_hoist.h) without a GPU: the library is built, exports the
whole ABI of the nine headers unmangled, and its six entry points refuse bad arguments before any
device access, in the order the header states."""
import ctypes
import os
import subprocess

import pytest

import hoist_cases as C
import nttmul
import rnsmp_cases as R


def _defined(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True,
                         check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if " T " in line}


def test_hoist_library_is_built():
    assert os.path.exists(nttmul.HOIST_LIB_PATH), f"{nttmul.HOIST_LIB_PATH} not built"


def test_hoist_library_exports_all_nine_headers():
    have = _defined(nttmul.HOIST_LIB_PATH)
    h = nttmul.hoist_exported_symbols()
    assert h == sorted(f"nttmul_{ctx}_hoist_{s}" for ctx in ("rns", "rnsmp")
                       for s in ("ntt_device", "ntt", "kernel_name"))
    want = (set(nttmul.exported_symbols()) | set(nttmul.mac_exported_symbols())
            | set(nttmul.rns_exported_symbols()) | set(nttmul.bconv_exported_symbols())
            | set(nttmul.rnsmp_exported_symbols()) | set(nttmul.galois_exported_symbols())
            | set(nttmul.ks_exported_symbols()) | set(nttmul.macn_exported_symbols()) | set(h))
    assert len(want) == 132
    assert sorted(want - have) == []
    assert sorted(s for s in have if "_hoist_" in s and s not in h) == []
    # the other headers' parsers do not pick the new names up
    assert not [s for s in nttmul.rns_exported_symbols() + nttmul.bconv_exported_symbols()
                + nttmul.rnsmp_exported_symbols() + nttmul.galois_exported_symbols()
                + nttmul.ks_exported_symbols() + nttmul.macn_exported_symbols()
                + nttmul.exported_symbols() if "_hoist_" in s]
    # and the older libraries hold none of them, and exactly the nttmul_* names they held
    for path in ("LIB_PATH", "MAC_LIB_PATH", "RNS_LIB_PATH", "BCONV_LIB_PATH", "RNSMP_LIB_PATH",
                 "GALOIS_LIB_PATH", "KS_LIB_PATH", "MACN_LIB_PATH"):
        assert not [s for s in _defined(getattr(nttmul, path)) if "_hoist" in s]
    assert {s for s in _defined(nttmul.MACN_LIB_PATH) if s.startswith("nttmul_")} == \
        {s for s in have if s.startswith("nttmul_")} - set(h)
    assert nttmul.HOIST_MAX_ROTS == C.MAX_ROTS == nttmul.GALOIS_MAX_COUNT


def test_call_refusals_come_before_any_device_access():
    """A NULL context is NTTMUL_EINVAL whatever else is passed, from all six entry points."""
    lib = nttmul.load_hoist_library()
    EINVAL = nttmul.NTTMUL_EINVAL
    one = (ctypes.c_uint32 * 1)()
    p = ctypes.addressof(one)
    ks = (ctypes.c_uint32 * 16)(*([1] * 16))
    buf = ctypes.create_string_buffer(64)
    for ctx in ("nttmul_rns", "nttmul_rnsmp"):
        dev = getattr(lib, f"{ctx}_hoist_ntt_device")
        host = getattr(lib, f"{ctx}_hoist_ntt")
        for comps in (0, 1, 2, 3):
            for rots in (0, 1, 16, 17):
                assert dev(None, p, p, p, ks, rots, 1, 1, comps, 0, None) == EINVAL
                assert dev(None, None, None, None, None, rots, 0, 1, comps, 0, None) == EINVAL
                assert host(None, p, p, p, ks, rots, 1, 1, comps) == EINVAL
            assert getattr(lib, f"{ctx}_hoist_kernel_name")(None, comps, buf, len(buf)) == EINVAL


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="checks the no-GPU behaviour")
def test_hoist_contexts_without_a_device_fail_loudly():
    for cls, n in ((nttmul.RnsHoistContext, 4096), (nttmul.RnsMpHoistContext, 8192)):
        with pytest.raises(nttmul.NttmulError) as ei:
            cls(n, R.BASIS32)
        assert ei.value.status == nttmul.NTTMUL_ENODEV


def test_the_contexts_are_their_own_classes_on_their_own_library():
    assert issubclass(nttmul.RnsHoistContext, nttmul.RnsMacnContext)
    assert issubclass(nttmul.RnsMpHoistContext, nttmul.RnsMpMacnContext)
    for cls in (nttmul.RnsHoistContext, nttmul.RnsMpHoistContext):
        for name in ("hoist_ntt", "hoist_ntt_device", "hoist_kernel_name", "macn_ntt", "mac_ntt",
                     "forward", "kernel_name", "close"):
            assert callable(getattr(cls, name))
    for cls in (nttmul.RnsContext, nttmul.RnsMpContext, nttmul.RnsMacnContext,
                nttmul.RnsMpMacnContext):
        assert not hasattr(cls, "hoist_ntt")
    libs = (nttmul.load_library(), nttmul.load_mac_library(), nttmul.load_rns_library(),
            nttmul.load_bconv_library(), nttmul.load_rnsmp_library(), nttmul.load_galois_library(),
            nttmul.load_ks_library(), nttmul.load_macn_library(), nttmul.load_hoist_library())
    assert len({id(x) for x in libs}) == 9
    assert libs[8]._name == nttmul.HOIST_LIB_PATH
    for older in libs[:8]:
        assert not hasattr(older, "nttmul_rns_hoist_ntt_device")
        assert not hasattr(older, "nttmul_rnsmp_hoist_kernel_name")
    # the prototypes through ctypes: k and rots sit between b_hat and batch, comps after terms
    vp, sz, u32, i32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_int
    u32p = ctypes.POINTER(u32)
    for ctx in ("nttmul_rns", "nttmul_rnsmp"):
        assert getattr(libs[8], f"{ctx}_hoist_ntt_device").argtypes == \
            [vp, vp, vp, vp, u32p, u32, sz, u32, u32, i32, vp]
        assert getattr(libs[8], f"{ctx}_hoist_ntt").argtypes == \
            [vp, vp, vp, vp, u32p, u32, sz, u32, u32]
        assert getattr(libs[8], f"{ctx}_hoist_kernel_name").argtypes == \
            [vp, u32, ctypes.c_char_p, sz]
        assert getattr(libs[8], f"{ctx}_macn_ntt_device").argtypes == \
            [vp, vp, vp, vp, sz, u32, u32, i32, i32, vp]
