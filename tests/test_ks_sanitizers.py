"""An ASan/UBSan CPU build of the host-only entry point of include/nttmul_ks.h (nttmul_ks_plan:
csrc/ks_plan.cpp as it stands, with the create-time checks of csrc/basis.cpp that every limb-aware
library shares and the planner's modular arithmetic of csrc/planner.cpp, the part of the host code
that needs no device), driven by the stand-alone program
tests/sanitize/ks_san.cpp, which also checks the results.  Any sanitizer report fails the run
(-fno-sanitize-recover=all).  Nothing is loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ntt-based-polynomial-multiplier-fpga_amd", "csrc")


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_asan_ubsan_ks_host_code(tmp_path):
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           "-g", "-O1"]
    exe = tmp_path / "ks_san"
    subprocess.run(["g++", "-std=c++17", *san, "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    "-o", str(exe),
                    os.path.join(ROOT, "tests", "sanitize", "ks_san.cpp"),
                    os.path.join(CSRC, "ks_plan.cpp"), os.path.join(CSRC, "basis.cpp"),
                    os.path.join(CSRC, "planner.cpp")],
                   check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    env.pop("LD_PRELOAD", None)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "ks sanitizer run ok: 40 plans" in out.stdout
