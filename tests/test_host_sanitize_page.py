"""CPU: the host-only code of read_page (csrc/page.cpp: validation, order_lines -- the line model -- and the masked
route's plan) under AddressSanitizer + UBSan, from a stand-alone program of its own, compiled together with what it calls
(components.cpp, glyphs.cpp, resample.cpp)."""
import os
import shutil
import subprocess

import pytest

import gpu_lib as gl

CSRC = os.path.join(gl.ROOT, "bnn-pynq_amd", "csrc")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_page_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "page_sanitize")
    srcs = [os.path.join(gl.ROOT, "tests", "host_sanitize_page", "main.cpp")] + [os.path.join(CSRC, f) for f in
                                                                                 ("page.cpp", "components.cpp", "glyphs.cpp", "resample.cpp")]
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    "-o", exe] + srcs, check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "page sanitize run ok" in out.stdout
