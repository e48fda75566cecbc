"""CPU build check of the page kernel (csrc/page_kernels.hip) in the BUILT gfx950 code object: k_page_record is
there, uses no scratch and spills nothing, keeps the glyph record kernel's LDS bound (csrc/glyphs.h: kGlyphMidBytes + a
record), writes the record in 16-byte stores -- and DESIGN.md's paragraph states the figures the code object holds.  The
new objects are translation units of their own, next to the older ones, whose rules do not depend on the new files."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJ = os.path.join(ROOT, "bnn-pynq_amd", "build", "page_kernels.o")
LLVM = "/opt/rocm/llvm/bin"
NAME = r"(?:void )?bnn::\(anonymous namespace\)::k_page_record\("


@pytest.fixture(scope="module")
def code_object():
    if not os.path.exists(OBJ):  # a tree that arrived with prebuilt libraries only: rebuild the object (hipcc cross-compiles)
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "bnn-pynq_amd"), "build/page_kernels.o"], check=True)
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


def body_and_metadata(code_object):
    dis, notes = code_object
    m = re.search(r"<%s.*?>:\n(.*?)(?=\n[0-9a-f]+ <[^L]|\Z)" % NAME, dis, re.S)
    assert m, "k_page_record not in the code object"
    n = re.search(r"\.name:\s+%s" % NAME, notes)
    assert n
    start = notes.rfind(".agpr_count", 0, n.start())
    nxt = notes.find(".agpr_count", n.end())
    md = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*$", notes[start:nxt if nxt > 0 else len(notes)], re.M)}
    return m.group(1), md


def test_the_kernel_in_the_code_object(code_object):
    body, md = body_and_metadata(code_object)
    print({k: md[k] for k in ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size", "kernarg_segment_size")})
    assert not re.search(r"\bscratch_", body), "scratch traffic"
    assert md["private_segment_fixed_size"] == 0 and md["vgpr_spill_count"] == 0 and md["sgpr_spill_count"] == 0
    assert md["max_flat_workgroup_size"] == 256 and md["agpr_count"] == 0
    with open(os.path.join(ROOT, "bnn-pynq_amd", "csrc", "glyphs.h")) as f:
        bound = int(re.search(r"constexpr int kGlyphMidBytes = (\d+);", f.read()).group(1)) + 784
    assert 0 < md["group_segment_fixed_size"] <= bound <= 64 * 1024
    assert re.search(r"\bds_(read|write|load|store)", body) and "s_barrier" in body  # the intermediate goes through LDS
    assert re.search(r"global_store_dwordx4", body)  # the record leaves in 16-byte stores
    assert re.search(r"global_load_dword\b", body) and re.search(r"global_load_ubyte", body)  # a tap: the label, then the pixel


def test_design_states_the_code_objects_figures(code_object):
    _, md = body_and_metadata(code_object)
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        m = re.search(r"`k_page_record` in the built code object: (\d+) VGPRs, (\d+) SGPRs, (\d+) bytes of LDS, (\d+) bytes of scratch", f.read())
    assert m, "DESIGN.md 9 does not state the figures of k_page_record"
    assert [int(v) for v in m.groups()] == [md["vgpr_count"], md["sgpr_count"], md["group_segment_fixed_size"], md["private_segment_fixed_size"]]


def test_kernel_objects_are_separate_translation_units():
    with open(os.path.join(ROOT, "bnn-pynq_amd", "Makefile")) as f:
        mk = f.read()
    assert re.search(r"^\$\(OBJ\)/page_kernels\.o: csrc/page_kernels\.hip.*\n\t.*--offload-arch=\$\(ARCH\)", mk, re.M)
    assert re.search(r"^\$\(OBJ\)/page\.o: csrc/page\.cpp.*\n\t.*-x c\+\+", mk, re.M)
    assert re.search(r"^\$\(LIBDIR\)/python_sw-%.*\$\(OBJ\)/page_kernels\.o \$\(OBJ\)/page\.o", mk, re.M)
    for older in ("kernels", "ecc_kernels", "repair_kernels", "wecc_kernels", "iwecc_kernels", "window_kernels", "windows", "preprocess",
                  "glyph_kernels", "glyphs", "component_kernels", "components"):
        assert "page" not in re.search(r"^\$\(OBJ\)/%s\.o: (.*)$" % older, mk, re.M).group(1), older
    with open(os.path.join(ROOT, "tools", "build_variant.sh")) as f:
        sh = f.read()
    assert "build/page_kernels.o" in sh and "build/page.o" in sh
    for f in ("page.h", "page.cpp"):  # the model and the plan are host-only: no HIP in them
        with open(os.path.join(ROOT, "bnn-pynq_amd", "csrc", f)) as fh:
            text = fh.read()
            assert "#include <hip" not in text and "__global__" not in text and "__device__" not in text, f
    for f in ("glyphs.h", "components.h", "glyph_kernels.h", "component_kernels.h", "glyph_kernels.hip", "component_kernels.hip"):
        with open(os.path.join(ROOT, "bnn-pynq_amd", "csrc", f)) as fh:
            assert "page" not in fh.read(), f  # GlyphDesc and the older kernels know nothing of the new route
