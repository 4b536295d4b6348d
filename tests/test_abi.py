"""CPU tests of the C ABI boundary: the library loads, exports every entry point include/nttmul.h
declares, and reports errors (never falls back to a CPU path) when no GPU is present."""
import ctypes
import os
import subprocess
import sys

import pytest

import nttmul


def test_library_exports_every_declared_symbol():
    lib = nttmul.load_library()
    syms = nttmul.exported_symbols()
    expected = {"nttmul_create", "nttmul_create_ex", "nttmul_create_sized", "nttmul_destroy",
                "nttmul_strerror",
                "nttmul_last_error", "nttmul_get_info", "nttmul_multiply_u32",
                "nttmul_multiply_u64", "nttmul_multiply_batch_u32", "nttmul_multiply_batch_u64",
                "nttmul_multiply_batch_device", "nttmul_fill_random_device", "ntt256_product1",
                "ntt256_product4", "ntt_red256_product1", "ntt_red256_product4",
                "nttmul_host_alloc", "nttmul_host_free"}
    assert expected <= set(syms), set(expected) - set(syms)
    for s in syms:
        assert hasattr(lib, s), s


def test_diag_library_exports_both_headers():
    """lib/libnttmul_diag.so (include/nttmul_diag.h) is the same ABI plus the diagnostic entry
    points: every symbol of both headers, unmangled."""
    import re
    path = os.path.join(os.path.dirname(nttmul.LIB_PATH), "libnttmul_diag.so")
    if not os.path.exists(path):
        pytest.skip("diagnostic build not present")
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True,
                         check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if " T " in line}
    diag_h = os.path.join(os.path.dirname(nttmul.HEADER_PATH), "nttmul_diag.h")
    diag = set(re.findall(r"^int (nttmul_diag_\w+)\(", open(diag_h).read(), re.M))
    assert diag == {"nttmul_diag_clock_stamps", "nttmul_diag_server_stamps",
                    "nttmul_diag_server_failpoint", "nttmul_diag_server_state"}, diag
    missing = (set(nttmul.exported_symbols()) | diag) - names
    assert not missing, missing
    assert {n for n in names if n.startswith("nttmul_diag_")} == diag


def test_only_the_diag_library_holds_the_diagnostic_entry_points():
    """The failure points of the device server (include/nttmul_diag.h) exist in the diagnostic
    build alone: no other library under lib/ defines a nttmul_diag_* symbol, and the Python
    bindings of the two new entry points match the header's site list and state structure."""
    import glob
    import re
    libs = sorted(glob.glob(os.path.join(os.path.dirname(nttmul.LIB_PATH), "*.so")))
    assert nttmul.LIB_PATH in libs
    for path in libs:
        if os.path.basename(path) == "libnttmul_diag.so":
            continue
        out = subprocess.run(["nm", "-D", path], capture_output=True, text=True, check=True).stdout
        assert "nttmul_diag_" not in out, path
    hdr = open(os.path.join(os.path.dirname(nttmul.HEADER_PATH), "nttmul_diag.h")).read()
    sites = re.findall(r"NTTMUL_DIAG_SITE_(\w+) = (\d+)", hdr)
    assert [(nm, int(v)) for nm, v in sites] == \
        [(nm, i) for i, nm in enumerate(nttmul.DIAG_SITES + ("COUNT",))]
    body = re.search(r"typedef struct nttmul_diag_server_state_t \{(.*?)\} nttmul_diag_server_state_t;",
                     hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [(t, nm.strip()) for t, names_ in re.findall(r"(u?int32_t) ([\w, ]+);", body)
              for nm in names_.split(",")]
    ctype = {"uint32_t": ctypes.c_uint32, "int32_t": ctypes.c_int32}
    assert [(nm, ctype[t]) for t, nm in fields] == list(nttmul.DiagServerState._fields_)


def test_exports_are_plain_c_abi():
    out = subprocess.run(["nm", "-D", "--defined-only", nttmul.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for s in nttmul.exported_symbols():
        assert s in names, f"{s} missing or C++-mangled"


def test_strerror_and_invalid_params():
    assert nttmul.strerror(0) == "ok"
    assert "range" in nttmul.strerror(nttmul.NTTMUL_ERANGE)
    lib = nttmul.load_library()
    h = ctypes.c_void_p()
    # parameter validation happens before any device access
    assert lib.nttmul_create(ctypes.byref(h), 1000, 2013265921, 1) == nttmul.NTTMUL_EINVAL
    assert lib.nttmul_create(ctypes.byref(h), 4096, 12289, 1) == nttmul.NTTMUL_EINVAL  # no 8192th root
    assert lib.nttmul_create(ctypes.byref(h), 4096, 2013265923, 1) == nttmul.NTTMUL_EINVAL  # composite
    assert lib.nttmul_create(ctypes.byref(h), 4096, (1 << 62) + 1, 1) == nttmul.NTTMUL_EINVAL
    assert lib.nttmul_create(ctypes.byref(h), 128, 12289, 1) == nttmul.NTTMUL_EINVAL  # n < 256


@pytest.mark.parametrize("field,value", [("issue_prio", 2), ("issue_prio", -2),
                                         ("zero_copy_kb", -5), ("copy_threads", -1)])
def test_invalid_dispatch_knobs(field, value):
    """The nttmul_params dispatch knobs (read once by nttmul_create_sized, include/nttmul.h) are
    range-checked before any device access: an out-of-range value is NTTMUL_EINVAL.
    nttmul_create_ex reads only the round 1-3 fields (NTTMUL_PARAMS_BASE_SIZE bytes, advisor r4),
    so the same struct through it never sees the knob: no EINVAL (ENODEV on a host without a
    GPU)."""
    lib = nttmul.load_library()
    h = ctypes.c_void_p()
    p = nttmul._Params(4096, 2013265921, 0, 1, 0, 0)
    setattr(p, field, value)
    assert lib.nttmul_create_sized(ctypes.byref(h), ctypes.byref(p), ctypes.sizeof(p)) == \
        nttmul.NTTMUL_EINVAL
    if not os.path.exists("/dev/kfd"):
        assert lib.nttmul_create_ex(ctypes.byref(h), ctypes.byref(p)) == nttmul.NTTMUL_ENODEV


def test_params_size_checked():
    """nttmul_create_sized takes the caller's struct size: below the round 1-3 layout (n .. flags,
    36 bytes) or above the struct this library knows is NTTMUL_EINVAL, before any device access."""
    lib = nttmul.load_library()
    h = ctypes.c_void_p()
    p = nttmul._Params(4096, 2013265921, 0, 1, 0, 0)
    base = nttmul._Params.issue_prio.offset
    assert base == 36
    for size in (0, base - 4, ctypes.sizeof(p) + 4):
        assert lib.nttmul_create_sized(ctypes.byref(h), ctypes.byref(p), size) == nttmul.NTTMUL_EINVAL
    if not os.path.exists("/dev/kfd"):
        for size in (base, ctypes.sizeof(p)):
            assert lib.nttmul_create_sized(ctypes.byref(h), ctypes.byref(p), size) == \
                nttmul.NTTMUL_ENODEV


def test_no_environment_reads_on_the_product_path():
    """Kernel choice comes from nttmul_params, never from the process environment: the library's
    sources call getenv nowhere."""
    src = os.path.join(os.path.dirname(nttmul.LIB_PATH), "..", "csrc")
    for name in os.listdir(src):
        if name.endswith((".cpp", ".hip", ".hpp")):
            text = open(os.path.join(src, name)).read()
            assert "getenv(" not in text, name


@pytest.mark.skipif(os.environ.get("HIP_VISIBLE_DEVICES") is None and os.path.exists("/dev/kfd"),
                    reason="a GPU may be present")
def test_no_gpu_fails_loudly():
    """Without a HIP device there is no silent CPU fallback: create returns NTTMUL_ENODEV."""
    with pytest.raises(nttmul.NttmulError) as ei:
        nttmul.Context(4096, 2013265921)
    assert ei.value.status == nttmul.NTTMUL_ENODEV


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="checks the no-GPU behaviour")
def test_no_device_host_alloc():
    """nttmul_host_alloc without a device: NTTMUL_ENODEV and a NULL pointer, no fallback."""
    with pytest.raises(nttmul.NttmulError) as ei:
        nttmul.host_empty((4, 16), "uint32")
    assert ei.value.status == nttmul.NTTMUL_ENODEV


@pytest.mark.parametrize("hook", ["NTTMUL_HOOK_ROWS_LD(b,u,N,b0)=0", "NTTMUL_HOOK_ROWS_ST(b,u,N,b0)=0",
                                  "NTTMUL_HOOK_ROWS_INPUT(x,y,u,j)=", "NTTMUL_HOOK_ROWS_OUTPUT(x,c,b,l)=",
                                  "NTTMUL_HOOK_XCHG()=", "NTTMUL_HOOK_COLS_LD(b,p,s,c,d)=0",
                                  "NTTMUL_HOOK_COLS_ST(b,p,s,c)=0", "NTTMUL_HOOK_TW(t,i,d)=0",
                                  "NTTMUL_HOOK_PRIO0(u)="])
def test_instrumentation_hooks_refuse_library_build(hook):
    """The wrong-result pricing variants live in tools/kbench (kb_kernels.hip defines the
    NTTMUL_HOOK_* points of csrc/kernels_dev.hpp); the library's translation unit kernels.hip
    stops with #error if any hook arrives defined, so none can reach libnttmul.so."""
    src = os.path.join(nttmul.PKG_DIR, "csrc", "kernels.hip")
    inc = ["-I" + os.path.join(nttmul.PKG_DIR, "csrc"),
           "-I" + os.path.join(os.path.dirname(nttmul.PKG_DIR), "include")]
    cmd = ["/opt/rocm/bin/hipcc", "-E", "--offload-arch=gfx950", "-std=c++17", *inc, src,
           "-o", os.devnull]
    if not os.path.exists(cmd[0]):
        pytest.skip("hipcc not present")
    bad = subprocess.run(cmd + [f"-D{hook}"], capture_output=True, text=True)
    assert bad.returncode != 0 and "instrumentation points" in bad.stderr
    ok = subprocess.run(cmd, capture_output=True, text=True)
    assert ok.returncode == 0, ok.stderr[-2000:]


def test_product_sources_hold_no_kbench_code():
    """Verdict r4 item 4: the rejected kernels (k_mp_persist, k_rows_w4 / _pipe / _ab) and the
    ablation switches moved to tools/kbench; the product sources name none of them."""
    csrc = os.path.join(nttmul.PKG_DIR, "csrc")
    for name in os.listdir(csrc):
        text = open(os.path.join(csrc, name), encoding="utf-8").read()
        for banned in ("NTTMUL_KBENCH", "NTTMUL_ABL_", "k_mp_persist", "k_rows_w4", "k_rows_pipe",
                       "k_rows_ab", "mp_lag", "pipe_per_wave", "rows_lds_extra"):
            assert banned not in text, (name, banned)


def test_product_sources_hold_no_settled_switches():
    """A compile-time switch lives in csrc/ only while a tracked tool builds both of its values
    (DESIGN.md "Where the experiments live"): the sources hold no `#ifndef NTTMUL_<NAME>` default
    but the kbench instrumentation points and the square-split switch that
    test_kbench_sources_compile builds both ways.  (NTTMUL_CLOCK_STAMPS, the diagnostic library's
    flag, is tested with #ifdef and has no default to declare.)  NTTMUL_SPLIT16 is the one settled
    switch left: the instantiations of its dead branch change the machine code of the n = 2048
    kernels (arith_select.hpp), so it goes in a change of its own."""
    import re
    allowed = re.compile(r"NTTMUL_(HOOK_[A-Z0-9_]+|C5_SQ|SPLIT16)")
    csrc = os.path.join(nttmul.PKG_DIR, "csrc")
    found = []
    for name in sorted(os.listdir(csrc)):
        if not name.endswith((".hpp", ".hip", ".cpp")):
            continue
        text = open(os.path.join(csrc, name), encoding="utf-8").read()
        found += [(name, m) for m in re.findall(r"^[ \t]*#[ \t]*ifndef[ \t]+(NTTMUL_\w+)", text, re.M)
                  if not allowed.fullmatch(m)]
    assert not found, found


@pytest.mark.parametrize("flags", [
    ["-DKB_SET=1"],
    ["-DKB_SET=1", "-DKB_ABL_NOLOAD=1", "-DKB_ABL_NOSTORE=1", "-DKB_ABL_NOXCHG=1"],
    ["-DKB_SET=1", "-DKB_ABL_L2LOAD=64"],
    ["-DKB_SET=2"],
    ["-DKB_SET=2", "-DNTTMUL_C5_SQ=0", "-DKB_ABL_STROWS=16", "-DKB_ABL_STCF=1"],
    ["-DKB_SET=2", "-DKB_ABL_STROWS=256", "-DKB_ABL_STCF=1", "-DKB_ABL_L2LOAD=256",
     "-DKB_ABL_L2CI=1", "-DKB_ABL_L2CF=1"],
    ["-DKB_SET=2", "-DKB_ABL_L2CI=1"],
    ["-DKB_SET=1", "-DKB_ABL_NOTW=1"], ["-DKB_SET=1", "-DKB_TW_LDS=1"],
    ["-DKB_SET=1", "-DKB_PRIO_GEN=1024"],
    ["-DKB_SET=1", "-DKB_ABL_X4LOAD=1", "-DKB_ABL_X4STORE=1"],
    ["-DKB_SET=1", "-DKB_PL=1"]])
def test_kbench_sources_compile(flags, tmp_path):
    """tools/kbench compiles the library's device code (csrc/kernels_dev.hpp) with its own
    launchers and pricing hooks: every kernel set and hook combination it is built with stays a
    valid translation unit (semantic check of every instantiated template, no code generation)."""
    root = os.path.dirname(nttmul.PKG_DIR)
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-std=c++17", "-fsyntax-only",
           "-I" + os.path.join(root, "include"), "-I" + os.path.join(nttmul.PKG_DIR, "csrc"),
           "-I" + os.path.join(root, "tools", "kbench"), "-I" + str(tmp_path), *flags,
           os.path.join(root, "tools", "kbench", "kb_kernels.hip")]
    if not os.path.exists(cmd[0]):
        pytest.skip("hipcc not present")
    # (KB_PL: the reordered-argument k_rows, generated from the product source)
    subprocess.run([sys.executable, os.path.join(root, "tools", "kbench", "gen_rows_pl.py"),
                    str(tmp_path)], check=True)
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
