"""CPU build check of the single-fault sweeps' matrix form (csrc/list_mfma_kernels.hip, DESIGN.md 9 "Sweeps on the matrix
cores") in the BUILT gfx950 code object: every list kernel present, no scratch and no spills, registers and LDS within the
occupancy its launch bounds claim.  Method and shapes are those of test_campaign_matrix_build.py."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from test_campaign_matrix_build import CONV, TAIL
from test_conv_matrix_build import LDS_PER_CU, LLVM, ROOT

OBJ = os.path.join(ROOT, "bnn-pynq_amd", "build", "list_mfma_kernels.o")
# kernel -> waves per block (a CU holds 8 waves of these kernels: two 4-wave blocks or one 8-wave block)
KERNELS = {"k_list_conv_mfma<%s>" % a: 4 for a in CONV}
KERNELS.update({"k_list_conv_mfma_a2<%s>" % a: 4 for a in CONV})
KERNELS.update({"k_list_tail_mfma<%s, %s>" % (a2, a): int(a.split(", ")[3]) for a2 in ("false", "true") for a in TAIL})


@pytest.fixture(scope="module")
def notes():
    if not os.path.exists(OBJ):  # a tree that arrived with prebuilt libraries only: rebuild the object (hipcc cross-compiles)
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "bnn-pynq_amd"), "build/list_mfma_kernels.o"], check=True)
    with tempfile.TemporaryDirectory() as d:
        shutil.copy(OBJ, os.path.join(d, "k.o"))  # (the code object is written next to the name given)
        subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", "k.o"], cwd=d, check=True, capture_output=True)
        co = os.path.join(d, next(f for f in os.listdir(d) if "gfx950" in f))
        raw = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
    return subprocess.run(["c++filt"], input=raw, check=True, capture_output=True, text=True).stdout


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_list_kernels_in_the_code_object(notes, kernel):
    m = re.search(r"\.name:\s+void bnn::\(anonymous namespace\)::%s\(" % re.escape(kernel), notes)
    assert m, kernel + " not in the code object"
    end = notes.find(".agpr_count", m.end())
    blk = notes[notes.rfind(".agpr_count", 0, m.start()): end if end > 0 else len(notes)]
    md = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*$", blk, re.M)}
    waves = KERNELS[kernel]
    assert md["private_segment_fixed_size"] == 0 and md["vgpr_spill_count"] == 0 and md["sgpr_spill_count"] == 0
    assert md["vgpr_count"] + md.get("agpr_count", 0) <= 256          # 8 waves per CU: two per SIMD share its 512 registers
    assert (8 // waves) * md["group_segment_fixed_size"] <= LDS_PER_CU
    assert md["max_flat_workgroup_size"] == 64 * waves
