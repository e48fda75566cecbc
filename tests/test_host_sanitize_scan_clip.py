"""CPU: the host-only code of the clip scan (csrc/scan_clip.cpp on top of csrc/scan.cpp: the order of the maps, the
layout, the launch tables, the limits, the capacity) under AddressSanitizer + UBSan, from a stand-alone program of its
own.  The two files call nothing outside themselves."""
import os
import shutil
import subprocess

import pytest

import gpu_lib as gl

CSRC = os.path.join(gl.ROOT, "bnn-pynq_amd", "csrc")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_scan_clip_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "scan_clip_sanitize")
    srcs = [os.path.join(gl.ROOT, "tests", "host_sanitize_scan_clip", "main.cpp"), os.path.join(CSRC, "scan_clip.cpp"), os.path.join(CSRC, "scan.cpp")]
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, "-o", exe] + srcs,
                   check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "scan clip sanitize run ok" in out.stdout
