"""An ASan/UBSan CPU build of the host-only part of include/nttmul_tmd.h (csrc/tmd_plan.hpp:
create's statuses in nttmul_mdntt_create's order over csrc/basis.cpp and then the plaintext
modulus' four, the bounds of t at both ends of each class, the constant tables against naive
recomputation, the calls' statuses, and the sub-batch arithmetic with offsets past 2^32 words), the
sources as they stand, driven by the stand-alone program tests/sanitize/tmd_san.cpp, which also
checks the results.  Any sanitizer report fails the run (-fno-sanitize-recover=all).  The program
runs as a plain child process; nothing is loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ntt-based-polynomial-multiplier-fpga_amd", "csrc")


def test_the_plan_header_has_no_device_header():
    text = open(os.path.join(CSRC, "tmd_plan.hpp")).read()
    assert "#include <hip" not in text and "_dev.hpp" not in text
    for name in ("mdntt_plan.hpp", "planner.hpp", "basis.hpp", "subbatch.hpp"):  # nor what it includes
        inner = open(os.path.join(CSRC, name)).read()
        assert "#include <hip" not in inner and "_dev.hpp" not in inner


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_asan_ubsan_tmd_host_arithmetic(tmp_path):
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           "-g", "-O1"]
    exe = tmp_path / "tmd_san"
    subprocess.run(["g++", "-std=c++17", *san, "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    "-o", str(exe), os.path.join(ROOT, "tests", "sanitize", "tmd_san.cpp"),
                    os.path.join(CSRC, "basis.cpp"), os.path.join(CSRC, "planner.cpp")],
                   check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "tmd sanitizer run ok: 20 tables, 290 walks" in out.stdout
