"""lib/libnttmul_mac.so (include/nttmul_mac.h) without a GPU: the library is built, exports the
whole ABI of nttmul.h and nttmul_mac.h unmangled, and refuses bad arguments before any device
access."""
import ctypes
import os
import subprocess

import pytest

import nttmul


def test_mac_library_is_built():
    assert os.path.exists(nttmul.MAC_LIB_PATH), f"{nttmul.MAC_LIB_PATH} not built"


def test_mac_library_exports_both_headers():
    out = subprocess.run(["nm", "-D", "--defined-only", nttmul.MAC_LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    have = {line.split()[-1] for line in out.splitlines() if " T " in line}
    mac = nttmul.mac_exported_symbols()
    assert mac == ["nttmul_mac_kernel_name", "nttmul_mac_ntt_device", "nttmul_mac_ntt_u32",
                   "nttmul_mac_ntt_u64"]
    want = set(nttmul.exported_symbols()) | set(mac)
    assert len(want) > 40
    assert sorted(want - have) == []


def test_the_product_library_does_not_grow():
    """libnttmul.so keeps its ABI: the new entry points are in the second library only."""
    out = subprocess.run(["nm", "-D", "--defined-only", nttmul.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    assert "nttmul_mac_" not in out and "k_mac" not in out


def test_bad_arguments_are_refused_before_any_device_access():
    lib = nttmul.load_mac_library()
    one = (ctypes.c_uint32 * 1)()
    p = ctypes.addressof(one)
    assert lib.nttmul_mac_ntt_device(None, p, p, p, 1, 1, 0, 32, 0, None) == nttmul.NTTMUL_EINVAL
    assert lib.nttmul_mac_ntt_device(None, p, p, p, 1, 0, 0, 32, 0, None) == nttmul.NTTMUL_EINVAL
    assert lib.nttmul_mac_ntt_device(None, None, None, None, 0, 1, 0, 32, 0, None) == nttmul.NTTMUL_EINVAL
    assert lib.nttmul_mac_ntt_u32(None, p, p, p, 1, 1, 0) == nttmul.NTTMUL_EINVAL
    assert lib.nttmul_mac_ntt_u64(None, p, p, p, 1, 0, 1) == nttmul.NTTMUL_EINVAL
    buf = ctypes.create_string_buffer(64)
    assert lib.nttmul_mac_kernel_name(None, 32, buf, len(buf)) == nttmul.NTTMUL_EINVAL


def test_mac_context_is_a_context_with_more():
    assert issubclass(nttmul.MacContext, nttmul.Context)
    for name in ("mac_ntt_device", "mac_ntt", "mac_kernel_name"):
        assert callable(getattr(nttmul.MacContext, name)) and not hasattr(nttmul.Context, name)
    # the two libraries are separate images: loading one does not rebind the other
    assert nttmul.load_mac_library() is not nttmul.load_library()
    assert nttmul.load_library()._name == nttmul.LIB_PATH


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="checks the no-GPU behaviour")
def test_mac_context_without_a_device_fails_loudly():
    with pytest.raises(nttmul.NttmulError) as ei:
        nttmul.MacContext(4096, 2013265921)
    assert ei.value.status == nttmul.NTTMUL_ENODEV
