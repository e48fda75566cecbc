"""CPU: the host-only code of enhance_picture / glyphs_to_mnist / classify_glyphs (csrc/glyphs.cpp: validation, the fit
rule, the plan with its shared coefficient tables and the global temporary's layout; csrc/resample.cpp: both filters'
tables) under AddressSanitizer + UBSan, from a stand-alone program of its own."""
import os
import shutil
import subprocess

import pytest

import gpu_lib as gl

CSRC = os.path.join(gl.ROOT, "bnn-pynq_amd", "csrc")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_glyphs_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "glyphs_sanitize")
    srcs = [os.path.join(gl.ROOT, "tests", "host_sanitize_glyphs", "main.cpp")] + [os.path.join(CSRC, f) for f in ("glyphs.cpp", "resample.cpp")]
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    "-o", exe] + srcs, check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "glyphs sanitize run ok" in out.stdout
