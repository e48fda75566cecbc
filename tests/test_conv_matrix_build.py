"""CPU build check of the matrix forms of cnvW1A1 layers 1-3 (k_conv_mfma, DESIGN.md 5 "The matrix pipe") in the BUILT
gfx950 code object: no scratch and no spills, the expected number of v_mfma_scale_f32_32x32x64_f8f6f4 and
ds_read_b128 per tile, and LDS / VGPRs that leave two blocks per CU; and a batch-size policy that gives both lanes of a
forked 131 072-image pass (65 536 images each) the matrix forms."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJ = os.path.join(ROOT, "bnn-pynq_amd", "build", "kernels.o")
LLVM = "/opt/rocm/lib/llvm/bin"
# template arguments -> (MFMAs, LDS reads of B per tile and wave: 9 taps x 2 rows x Cin/64; 3 columns x 4 rows x Cin/64)
KERNELS = {"30, 2, 2, true, 2": (18, 12), "14, 2, 4, false, 8": (18, 12), "12, 4, 4, true, 8": (36, 24)}
LDS_PER_CU = 160 * 1024


@pytest.fixture(scope="module")
def code_object():
    if not os.path.exists(OBJ):  # a tree that arrived with prebuilt libraries only: rebuild the object (hipcc cross-compiles)
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "bnn-pynq_amd"), "build/kernels.o"], check=True)
    d = tempfile.mkdtemp()
    try:
        shutil.copy(OBJ, os.path.join(d, "k.o"))
        subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", "k.o"], cwd=d, check=True, capture_output=True)
        co = os.path.join(d, next(f for f in os.listdir(d) if "gfx950" in f))
        dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", co], check=True, capture_output=True,
                             text=True).stdout
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
        dem = subprocess.run(["c++filt"], input=dis + "\n@@@\n" + notes, check=True, capture_output=True, text=True).stdout
        dis, notes = dem.split("\n@@@\n")
        yield dis, notes
    finally:
        shutil.rmtree(d)


def kernel_body(dis, args):
    m = re.search(r"<void bnn::\(anonymous namespace\)::k_conv_mfma<%s>\(.*?>:\n(.*?)(?=\n[0-9a-f]+ <[^L]|\Z)" % re.escape(args), dis, re.S)
    assert m, "k_conv_mfma<%s> not in the code object" % args
    return m.group(1)


def metadata(notes, args):
    m = re.search(r"\.name:\s+void bnn::\(anonymous namespace\)::k_conv_mfma<%s>" % re.escape(args), notes)
    assert m, args
    start = notes.rfind(".agpr_count", 0, m.start())
    blk = notes[start:m.end()]
    blk += notes[m.end():notes.find(".agpr_count", m.end()) if notes.find(".agpr_count", m.end()) > 0 else len(notes)]
    return {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*$", blk, re.M)}


@pytest.mark.parametrize("args", sorted(KERNELS))
def test_matrix_forms_in_the_code_object(code_object, args):
    dis, notes = code_object
    body = kernel_body(dis, args)
    mfma, reads = KERNELS[args]
    assert len(re.findall(r"\bv_mfma_scale_f32_32x32x64_f8f6f4\b", body)) == mfma
    assert len(re.findall(r"\bds_read_b128\b", body)) == reads
    assert not re.search(r"\bscratch_|\bbuffer_store", body), "scratch traffic"
    md = metadata(notes, args)
    assert md["private_segment_fixed_size"] == 0 and md["vgpr_spill_count"] == 0 and md["sgpr_spill_count"] == 0
    assert md["vgpr_count"] + md.get("agpr_count", 0) <= 256                 # two waves per SIMD: two blocks of 4 waves per CU
    assert 2 * md["group_segment_fixed_size"] <= LDS_PER_CU                  # two blocks per CU


def test_policy_sends_both_forked_lanes_to_the_matrix_forms():
    with open(os.path.join(ROOT, "bnn-pynq_amd", "csrc", "kernels.hip")) as f:
        src = f.read()
    m = re.search(r'inline long long conv_mfma_min\(\) \{.*?getenv\("BNN_MI355X_CONV_MFMA_MIN"\);\s*return e \? std::atoll\(e\) : (\d+)LL;', src,
                  re.S)
    assert m and 1 < int(m.group(1)) <= 65536
