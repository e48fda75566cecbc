"""CPU: the host-only code of the pixel formats (csrc/pixfmt.cpp: validation and the model the kernel is pinned to) under
AddressSanitizer + UBSan, from a stand-alone program of its own.  The file calls nothing outside itself."""
import os
import shutil
import subprocess

import pytest

import gpu_lib as gl

CSRC = os.path.join(gl.ROOT, "bnn-pynq_amd", "csrc")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_pixfmt_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "pixfmt_sanitize")
    srcs = [os.path.join(gl.ROOT, "tests", "host_sanitize", "pixfmt_main.cpp"), os.path.join(CSRC, "pixfmt.cpp")]
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, "-o", exe] + srcs,
                   check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "pixfmt sanitize run ok" in out.stdout
