"""CPU build check of the LFC nets' matrix form (csrc/lfc_mfma_kernels.hip): the file compiles for gfx950, and the
compiler's own resource remarks show six instantiations of k_lfc_mfma without scratch, at two waves a SIMD.  (The library's
exports are tests/test_abi_symbols.py's: this form adds none.)"""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_lfc_matrix_kernels_compile_for_gfx950_without_scratch(tmp_path):
    src = os.path.join(ROOT, "bnn-pynq_amd", "csrc", "lfc_mfma_kernels.hip")
    out = subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "-Wall", "--offload-arch=gfx950", "-mllvm", "-amdgpu-mfma-vgpr-form=1",
                          "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", str(tmp_path / "lfc_mfma_kernels.o")],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    assert "warning:" not in out.stderr, out.stderr[-3000:]
    kernels = re.findall(r"Function Name: (\S*k_lfc_mfma\S*)", out.stderr)
    assert len(kernels) == 6 and len(set(kernels)) == 6, kernels
    assert [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", out.stderr)] == [0] * 6
    assert all(int(x) <= 256 for x in re.findall(r" VGPRs: (\d+)", out.stderr))
    assert [int(x) for x in re.findall(r"Occupancy \[waves/SIMD\]: (\d+)", out.stderr)] == [2] * 6
