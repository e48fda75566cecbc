"""CPU: the column-interleaved coded weight memories' host code (csrc/mem_org.cpp: wecc_depth, iwecc_site, phys_load,
phys_logical, phys_repair and phys_replay with weight_interleave 1, the route of bnn_mi355x_pack_params_iwecc) and the
kernels' bit exchange (csrc/iwecc.h, stepped with an array of lanes) under AddressSanitizer + UBSan, from a stand-alone
program of its own."""
import os
import shutil
import subprocess

import pytest

import gpu_lib as gl

CSRC = os.path.join(gl.ROOT, "bnn-pynq_amd", "csrc")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_iwecc_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "iwecc_sanitize")
    srcs = [os.path.join(gl.ROOT, "tests", "host_sanitize_iwecc", "main.cpp")] + \
           [os.path.join(CSRC, f) for f in ("topology.cpp", "packed_params.cpp", "faults.cpp", "mem_org.cpp")]
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, "-o", exe] + srcs,
                   check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([exe, os.path.join(gl.ROOT, "bnn-pynq_amd", "bnn", "params")], capture_output=True, text=True, env=env)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "iwecc sanitize run ok" in out.stdout
