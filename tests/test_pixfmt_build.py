"""CPU build check of the pixel formats' kernel (csrc/pixfmt_kernels.hip, DESIGN.md 9 "Camera frames") in the BUILT gfx950
code object: every k_unpack_frames instance is there, uses no scratch and no LDS, spills nothing, is built for the threads
it is launched with and stays inside the register record DESIGN.md states.  Resource metadata only -- the same properties
as test_detect_build.py's."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJ = os.path.join(ROOT, "bnn-pynq_amd", "build", "pixfmt_kernels.o")
LLVM = "/opt/rocm/llvm/bin"
# format -> (VGPR bound, SGPR bound): DESIGN.md 9, "Camera frames" (RGB, L, BGR, NV12, I420, YUYV)
INSTANCES = {0: (16, 32), 1: (24, 32), 2: (24, 32), 3: (56, 40), 4: (56, 40), 5: (32, 32)}


@pytest.fixture(scope="module")
def notes():
    if not os.path.exists(OBJ):  # a tree that arrived with prebuilt libraries only: rebuild the object (hipcc cross-compiles)
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "bnn-pynq_amd"), "build/pixfmt_kernels.o"], check=True)
    d = tempfile.mkdtemp()
    try:
        shutil.copy(OBJ, os.path.join(d, "k.o"))
        subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", "k.o"], cwd=d, check=True, capture_output=True)
        co = os.path.join(d, next(f for f in os.listdir(d) if "gfx950" in f))
        out = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
        yield subprocess.run(["c++filt"], input=out, check=True, capture_output=True, text=True).stdout
    finally:
        shutil.rmtree(d)


def metadata(notes, fmt):
    name = r"(?:void )?bnn::\(anonymous namespace\)::k_unpack_frames<%d>\(" % fmt
    n = re.search(r"\.name:\s+%s" % name, notes)
    assert n, "k_unpack_frames<%d> not in the code object" % fmt
    start = notes.rfind(".agpr_count", 0, n.start())
    nxt = notes.find(".agpr_count", n.end())
    return {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*$", notes[start:nxt if nxt > 0 else len(notes)], re.M)}


@pytest.mark.parametrize("fmt", sorted(INSTANCES))
def test_instances_in_the_code_object(notes, fmt):
    vgprs, sgprs = INSTANCES[fmt]
    md = metadata(notes, fmt)
    print(fmt, {k: md[k] for k in ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size", "kernarg_segment_size")})
    assert md["private_segment_fixed_size"] == 0 and md["vgpr_spill_count"] == 0 and md["sgpr_spill_count"] == 0
    assert md["group_segment_fixed_size"] == 0
    assert md["max_flat_workgroup_size"] == 256
    assert md["vgpr_count"] <= vgprs and md["sgpr_count"] <= sgprs and md["agpr_count"] == 0


def test_there_are_exactly_six_instances(notes):
    assert len(re.findall(r"\.name:\s+(?:void )?bnn::\(anonymous namespace\)::k_unpack_frames<", notes)) == len(INSTANCES)


def test_kernel_objects_are_separate_translation_units():
    """the Makefile and tools/build_variant.sh link the kernel's object, and the host-only model's, behind the detections';
    the rules of the older objects do not name the new files"""
    with open(os.path.join(ROOT, "bnn-pynq_amd", "Makefile")) as f:
        mk = f.read()
    assert re.search(r"^\$\(OBJ\)/pixfmt_kernels\.o: csrc/pixfmt_kernels\.hip.*\n\t.*--offload-arch", mk, re.M)
    assert re.search(r"^\$\(OBJ\)/pixfmt\.o: csrc/pixfmt\.cpp.*\n\t.*-x c\+\+", mk, re.M)
    assert re.search(r"^\$\(LIBDIR\)/python_sw-%.*\$\(OBJ\)/detect_kernels\.o \$\(OBJ\)/detect\.o \$\(OBJ\)/pixfmt_kernels\.o \$\(OBJ\)/pixfmt\.o", mk, re.M)
    for older in ("kernels", "ecc_kernels", "repair_kernels", "wecc_kernels", "iwecc_kernels", "window_kernels", "windows", "glyph_kernels",
                  "glyphs", "component_kernels", "components", "page_kernels", "page", "scan_kernels", "scan", "scan_clip_kernels", "scan_clip",
                  "detect_kernels", "detect", "preprocess", "resample"):
        assert "pixfmt" not in re.search(r"^\$\(OBJ\)/%s\.o: (.*)$" % older, mk, re.M).group(1), older
    with open(os.path.join(ROOT, "tools", "build_variant.sh")) as f:
        assert "build/detect_kernels.o build/detect.o build/pixfmt_kernels.o build/pixfmt.o" in f.read()
    for f in ("pixfmt.h", "pixfmt.cpp"):  # the model's statement is host-only: no HIP in it
        with open(os.path.join(ROOT, "bnn-pynq_amd", "csrc", f)) as fh:
            text = fh.read()
            assert "#include <hip" not in text and "__global__" not in text and "__device__" not in text, f
