"""CPU build check of the detections' kernels (csrc/detect_kernels.hip) in the BUILT gfx950 code object: the
two kernels are there, use no scratch, spill nothing, are built for the threads they are launched with and stay inside
the resource record DESIGN.md states; the frame kernel's LDS is what detect_kernels.h says, the key kernel uses none.
Nothing else about the instruction stream is checked -- the same properties as test_scan_clip_build.py's."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJ = os.path.join(ROOT, "bnn-pynq_amd", "build", "detect_kernels.o")
LLVM = "/opt/rocm/llvm/bin"
# kernel -> (threads, LDS bytes, VGPR bound, SGPR bound): DESIGN.md 9, "Detections"
KERNELS = {"k_detect_keys": (256, 0, 16, 32), "k_detect_frame": (1024, 67352, 64, 96)}


@pytest.fixture(scope="module")
def code_object():
    if not os.path.exists(OBJ):  # a tree that arrived with prebuilt libraries only: rebuild the object (hipcc cross-compiles)
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "bnn-pynq_amd"), "build/detect_kernels.o"], check=True)
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


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_kernels_in_the_code_object(code_object, kernel):
    threads, lds, vgprs, sgprs = KERNELS[kernel]
    body, md = body_and_metadata(code_object, kernel)
    print({k: md[k] for k in ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size", "kernarg_segment_size")})
    assert not re.search(r"\bscratch_", body), "scratch traffic"
    assert md["private_segment_fixed_size"] == 0 and md["vgpr_spill_count"] == 0 and md["sgpr_spill_count"] == 0
    assert md["max_flat_workgroup_size"] == threads
    assert md["group_segment_fixed_size"] == lds
    assert md["vgpr_count"] <= vgprs and md["sgpr_count"] <= sgprs and md["agpr_count"] == 0
    if lds:
        assert re.search(r"\bds_", body) and re.search(r"\bs_barrier", body)
    else:
        assert not re.search(r"\bds_", body), "LDS"


def test_the_stated_lds_bound():
    """detect_kernels.h states the frame kernel's static LDS; it is the figure above, below the 160 KiB of a CU"""
    with open(os.path.join(ROOT, "bnn-pynq_amd", "csrc", "detect_kernels.h")) as f:
        m = re.search(r"constexpr int kDetectLdsBytes = kDetectMaxCandidates \* 16 \+ 256 \* 4 \+ \(kDetectMaxCandidates / 32\) \* 4 \+ 4 \* 16 \* 4 \+ 6 \* 4;",
                      f.read())
    assert m
    assert 4096 * 16 + 256 * 4 + (4096 // 32) * 4 + 4 * 16 * 4 + 6 * 4 == KERNELS["k_detect_frame"][1] <= 160 * 1024


def test_kernel_objects_are_separate_translation_units():
    """the Makefile and tools/build_variant.sh link the detection kernels' object, and the host-only model's, behind the clip
    scan's; the rules of the older objects do not name the new files"""
    with open(os.path.join(ROOT, "bnn-pynq_amd", "Makefile")) as f:
        mk = f.read()
    assert re.search(r"^\$\(OBJ\)/detect_kernels\.o: csrc/detect_kernels\.hip.*\n\t.*--offload-arch", mk, re.M)
    assert re.search(r"^\$\(OBJ\)/detect\.o: csrc/detect\.cpp.*\n\t.*-x c\+\+", mk, re.M)
    assert re.search(r"^\$\(LIBDIR\)/python_sw-%.*\$\(OBJ\)/scan_clip_kernels\.o \$\(OBJ\)/scan_clip\.o \$\(OBJ\)/detect_kernels\.o \$\(OBJ\)/detect\.o", mk, re.M)
    for older in ("kernels", "ecc_kernels", "repair_kernels", "wecc_kernels", "iwecc_kernels", "window_kernels", "windows", "glyph_kernels",
                  "glyphs", "component_kernels", "components", "page_kernels", "page", "scan_kernels", "scan", "scan_clip_kernels", "scan_clip",
                  "preprocess", "resample"):
        assert "detect" not in re.search(r"^\$\(OBJ\)/%s\.o: (.*)$" % older, mk, re.M).group(1), older
    for f in ("scan_kernels.hip", "scan_clip_kernels.hip", "kernels.hip"):
        with open(os.path.join(ROOT, "bnn-pynq_amd", "csrc", f)) as fh:
            assert "detect" not in fh.read(), f
    with open(os.path.join(ROOT, "tools", "build_variant.sh")) as f:
        assert "build/scan_clip_kernels.o build/scan_clip.o build/detect_kernels.o build/detect.o" in f.read()
    for f in ("detect.h", "detect.cpp"):  # the model's statement is host-only: no HIP in it
        with open(os.path.join(ROOT, "bnn-pynq_amd", "csrc", f)) as fh:
            text = fh.read()
            assert "#include <hip" not in text and "__global__" not in text and "__device__" not in text, f
