"""CPU build check of the dense scan's kernels (csrc/scan_kernels.hip) in the BUILT gfx950 code object: the
six stage kernels and the four resize kernels are there, use no scratch, spill nothing, use no LDS and are built for the
256 threads they are launched with; the stage kernels read their rows through scalar loads and count with v_bcnt (layer
0: v_dot4).  Nothing else about the instruction stream is checked."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJ = os.path.join(ROOT, "bnn-pynq_amd", "build", "scan_kernels.o")
LLVM = "/opt/rocm/llvm/bin"
STAGES = ["k_scan_conv0", "k_scan_quad<1, true>", "k_scan_quad<1, false>", "k_scan_quad<2, true>", "k_scan_vec<2>", "k_scan_vec<4>"]
RESIZE = ["k_scan_resize_h<1>", "k_scan_resize_h<3>", "k_scan_resize_v<1>", "k_scan_resize_v<3>"]


@pytest.fixture(scope="module")
def code_object():
    if not os.path.exists(OBJ):  # a tree that arrived with prebuilt libraries only: rebuild the object (hipcc cross-compiles)
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "bnn-pynq_amd"), "build/scan_kernels.o"], check=True)
    d = tempfile.mkdtemp()
    try:
        shutil.copy(OBJ, os.path.join(d, "k.o"))
        subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", "k.o"], cwd=d, check=True, capture_output=True)
        co = os.path.join(d, next(f for f in os.listdir(d) if "gfx950" in f))
        dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", co], check=True, capture_output=True,
                             text=True).stdout
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
        dem = subprocess.run(["c++filt"], input=dis + "\n@@@\n" + notes, check=True, capture_output=True, text=True).stdout
        yield dem.split("\n@@@\n")
    finally:
        shutil.rmtree(d)


def body_and_metadata(code_object, kernel):
    dis, notes = code_object
    name = r"(?:void )?bnn::\(anonymous namespace\)::%s\(" % re.escape(kernel)
    m = re.search(r"<%s.*?>:\n(.*?)(?=\n[0-9a-f]+ <[^L]|\Z)" % name, dis, re.S)
    assert m, "%s not in the code object" % kernel
    n = re.search(r"\.name:\s+%s" % name, notes)
    assert n
    start = notes.rfind(".agpr_count", 0, n.start())
    nxt = notes.find(".agpr_count", n.end())
    md = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*$", notes[start:nxt if nxt > 0 else len(notes)], re.M)}
    return m.group(1), md


@pytest.mark.parametrize("kernel", STAGES + RESIZE)
def test_kernels_in_the_code_object(code_object, kernel):
    body, md = body_and_metadata(code_object, kernel)
    print({k: md[k] for k in ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size", "kernarg_segment_size")})
    assert not re.search(r"\bscratch_", body), "scratch traffic"
    assert md["private_segment_fixed_size"] == 0 and md["vgpr_spill_count"] == 0 and md["sgpr_spill_count"] == 0
    assert md["max_flat_workgroup_size"] == 256
    assert md["group_segment_fixed_size"] == 0 and not re.search(r"\bds_", body), "LDS"
    if kernel in STAGES:
        assert re.search(r"\bs_load_dword", body), "the rows come through scalar loads"
        assert re.search(r"\bv_dot4", body) if kernel == "k_scan_conv0" else re.search(r"\bv_bcnt_u32_b32", body)


def test_the_stated_lds_bound():
    with open(os.path.join(ROOT, "bnn-pynq_amd", "csrc", "scan_kernels.h")) as f:
        assert re.search(r"constexpr int kScanLdsBytes = 0;", f.read())


def test_the_lane_bodies_are_stated_once():
    """the neuron loops, the popcount helpers and clip8 stand in csrc/scan_bodies.h and in no other scan file; the dense
    scan's and the clip scan's kernel files both include it"""
    import glob
    csrc = os.path.join(ROOT, "bnn-pynq_amd", "csrc")
    files = sorted(f for ext in ("h", "hip", "cpp") for f in glob.glob(os.path.join(csrc, "scan*." + ext)))
    text = {}
    for f in files:
        with open(f) as fh:
            text[os.path.basename(f)] = fh.read()
    assert "scan_bodies.h" in text and "scan_kernels.hip" in text and "scan_clip_kernels.hip" in text
    for needle in ("__builtin_amdgcn_sdot4", "v_bcnt_u32_b32"):
        assert [f for f in text if needle in text[f]] == ["scan_bodies.h"], needle
    assert [f for f in text if re.search(r"^[^/\n]*\bclip8\(uint32_t \w+\) \{", text[f], re.M)] == ["scan_bodies.h"]
    for f in ("scan_kernels.hip", "scan_clip_kernels.hip"):
        assert '#include "scan_bodies.h"' in text[f], f


def test_kernel_objects_are_separate_translation_units():
    """the Makefile and tools/build_variant.sh link the scan kernels' object, and the host-only model's, next to the older
    ones, whose rules do not depend on the new files (kernels.o is what it was but for run_cnv's first_stage)"""
    with open(os.path.join(ROOT, "bnn-pynq_amd", "Makefile")) as f:
        mk = f.read()
    assert re.search(r"^\$\(OBJ\)/scan_kernels\.o: csrc/scan_kernels\.hip.*\n\t.*--offload-arch", mk, re.M)
    assert re.search(r"^\$\(OBJ\)/scan\.o: csrc/scan\.cpp.*\n\t.*-x c\+\+", mk, re.M)
    assert re.search(r"^\$\(LIBDIR\)/python_sw-%.*\$\(OBJ\)/scan_kernels\.o \$\(OBJ\)/scan\.o", mk, re.M)
    for older in ("kernels", "ecc_kernels", "repair_kernels", "wecc_kernels", "iwecc_kernels", "window_kernels", "windows", "glyph_kernels",
                  "glyphs", "component_kernels", "components", "page_kernels", "page", "preprocess", "resample"):
        assert "scan" not in re.search(r"^\$\(OBJ\)/%s\.o: (.*)$" % older, mk, re.M).group(1), older
    with open(os.path.join(ROOT, "tools", "build_variant.sh")) as f:
        sh = f.read()
    assert "build/scan_kernels.o" in sh and "build/scan.o" in sh
    for f in ("scan.h", "scan.cpp"):  # the model's statement is host-only: no HIP in it
        with open(os.path.join(ROOT, "bnn-pynq_amd", "csrc", f)) as fh:
            text = fh.read()
            assert "#include <hip" not in text and "__global__" not in text and "__device__" not in text, f
