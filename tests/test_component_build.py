"""CPU build check of the component kernels (csrc/component_kernels.hip) in the BUILT gfx950 code object: the
seven kernels are there, use no scratch and spill nothing, are built for the 256 threads they are launched with, and stay
within the LDS bound the header states (none); the merge kernel joins with an atomic min, the stats kernel reduces with
atomic min and max.  Nothing else about the instruction stream is checked."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJ = os.path.join(ROOT, "bnn-pynq_amd", "build", "component_kernels.o")
LLVM = "/opt/rocm/llvm/bin"
KERNELS = ["k_cc_bits", "k_cc_merge", "k_cc_flatten", "k_cc_roots", "k_cc_stats", "k_cc_compact", "k_cc_relabel"]


def stated(path, pattern):
    with open(os.path.join(ROOT, path)) as f:
        m = re.search(pattern, f.read())
    assert m, "%s does not state %s" % (path, pattern)
    return int(m.group(1))


@pytest.fixture(scope="module")
def code_object():
    if not os.path.exists(OBJ):  # a tree that arrived with prebuilt libraries only: rebuild the object (hipcc cross-compiles)
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "bnn-pynq_amd"), "build/component_kernels.o"], check=True)
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


def test_the_stated_limits_agree():
    assert stated("bnn-pynq_amd/csrc/components.h", r"constexpr long kMaxComponentPixels = 1L << (\d+);") == 24
    assert stated("include/bnn_mi355x.h", r"#define BNN_MI355X_FIND_MAX_PIXELS (\d+)") == 1 << 24
    assert stated("bnn-pynq_amd/csrc/components.h", r"constexpr int kMaxReach = (\d+);") == stated("include/bnn_mi355x.h",
                                                                                                  r"#define BNN_MI355X_FIND_MAX_REACH (\d+)")


@pytest.mark.parametrize("kernel", KERNELS)
def test_kernels_in_the_code_object(code_object, kernel):
    body, md = body_and_metadata(code_object, kernel)
    print({k: md[k] for k in ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size", "kernarg_segment_size")})
    assert not re.search(r"\bscratch_", body), "scratch traffic"
    assert md["private_segment_fixed_size"] == 0 and md["vgpr_spill_count"] == 0 and md["sgpr_spill_count"] == 0
    assert md["max_flat_workgroup_size"] == 256
    assert md["group_segment_fixed_size"] <= stated("bnn-pynq_amd/csrc/component_kernels.h", r"constexpr int kComponentLdsBytes = (\d+);")
    if kernel == "k_cc_merge":
        assert re.search(r"global_atomic_[su]?min", body)
    if kernel == "k_cc_stats":
        assert re.search(r"global_atomic_[su]?min", body) and re.search(r"global_atomic_[su]?max", body)


def test_kernel_objects_are_separate_translation_units():
    """the Makefile and tools/build_variant.sh link the component kernels' object, and the host-only model's, next to the
    older ones, whose rules do not depend on the new files"""
    with open(os.path.join(ROOT, "bnn-pynq_amd", "Makefile")) as f:
        mk = f.read()
    assert re.search(r"^\$\(OBJ\)/component_kernels\.o: csrc/component_kernels\.hip.*\n\t.*--offload-arch", mk, re.M)
    assert re.search(r"^\$\(OBJ\)/components\.o: csrc/components\.cpp.*\n\t.*-x c\+\+", mk, re.M)
    assert re.search(r"^\$\(LIBDIR\)/python_sw-%.*\$\(OBJ\)/component_kernels\.o \$\(OBJ\)/components\.o", mk, re.M)
    for older in ("kernels", "ecc_kernels", "repair_kernels", "wecc_kernels", "iwecc_kernels", "window_kernels", "windows", "glyph_kernels",
                  "glyphs", "preprocess", "resample"):
        assert "component" not in re.search(r"^\$\(OBJ\)/%s\.o: (.*)$" % older, mk, re.M).group(1), older
    with open(os.path.join(ROOT, "tools", "build_variant.sh")) as f:
        sh = f.read()
    assert "build/component_kernels.o" in sh and "build/components.o" in sh
    for f in ("components.h", "components.cpp"):  # the model's statement is host-only: no HIP in it
        with open(os.path.join(ROOT, "bnn-pynq_amd", "csrc", f)) as fh:
            text = fh.read()
            assert "#include <hip" not in text and "__global__" not in text and "__device__" not in text, f
