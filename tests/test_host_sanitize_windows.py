"""CPU: the host-only planning code of windows_to_cifar / classify_windows (csrc/windows.cpp: tile_boxes, the validation of
the caller's boxes, the grouping by size with its permutation, the route decision, the coefficient tables' layout) under
AddressSanitizer + UBSan, from a stand-alone program of its own."""
import os
import shutil
import subprocess

import pytest

import gpu_lib as gl

CSRC = os.path.join(gl.ROOT, "bnn-pynq_amd", "csrc")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_windows_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "windows_sanitize")
    srcs = [os.path.join(gl.ROOT, "tests", "host_sanitize_windows", "main.cpp")] + [os.path.join(CSRC, f) for f in ("windows.cpp", "resample.cpp")]
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    "-o", exe] + srcs, check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "windows sanitize run ok" in out.stdout
