"""CPU build check of the glyph kernels (csrc/glyph_kernels.hip) in the BUILT gfx950 code object: the six
kernels are there, use no scratch and spill nothing; the record kernel's LDS is the bound the headers state
(csrc/glyphs.h: kGlyphMidBytes + a record; include/bnn_mi355x.h: BNN_MI355X_GLYPH_LDS_BYTES); and the enhancement holds
no fused multiply-add: Pillow's blend rounds the multiply and the add separately, and an FMA gives other bytes."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJ = os.path.join(ROOT, "bnn-pynq_amd", "build", "glyph_kernels.o")
LLVM = "/opt/rocm/llvm/bin"
KERNELS = ["k_glyph_luma<1>", "k_glyph_luma<3>", "k_glyph_luma<4>", "k_glyph_enhance", "k_glyph_bbox", "k_glyph_record"]


def stated(path, pattern):
    with open(os.path.join(ROOT, path)) as f:
        m = re.search(pattern, f.read())
    assert m, "%s does not state %s" % (path, pattern)
    return int(m.group(1))


@pytest.fixture(scope="module")
def code_object():
    if not os.path.exists(OBJ):  # a tree that arrived with prebuilt libraries only: rebuild the object (hipcc cross-compiles)
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "bnn-pynq_amd"), "build/glyph_kernels.o"], check=True)
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


def test_the_stated_bounds_agree():
    mid = stated("bnn-pynq_amd/csrc/glyphs.h", r"constexpr int kGlyphMidBytes = (\d+);")
    assert stated("include/bnn_mi355x.h", r"#define BNN_MI355X_GLYPH_LDS_BYTES (\d+)") == mid
    assert mid == stated("bnn-pynq_amd/csrc/windows.h", r"constexpr int kWindowMidBytes = (\d+);")  # the window kernel's budget
    assert mid + 784 <= 64 * 1024


@pytest.mark.parametrize("kernel", KERNELS)
def test_kernels_in_the_code_object(code_object, kernel):
    body, md = body_and_metadata(code_object, kernel)
    print({k: md[k] for k in ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size", "kernarg_segment_size")})
    assert not re.search(r"\bscratch_", body), "scratch traffic"
    assert md["private_segment_fixed_size"] == 0 and md["vgpr_spill_count"] == 0 and md["sgpr_spill_count"] == 0
    assert md["max_flat_workgroup_size"] == 256
    if kernel == "k_glyph_record":
        bound = stated("bnn-pynq_amd/csrc/glyphs.h", r"constexpr int kGlyphMidBytes = (\d+);") + 784
        assert 0 < md["group_segment_fixed_size"] <= bound <= 64 * 1024
        assert re.search(r"\bds_(read|write|load|store)", body) and "s_barrier" in body  # the intermediate goes through LDS
        assert re.search(r"global_store_dwordx4", body)  # the record leaves in 16-byte stores
    if kernel.startswith("k_glyph_luma"):
        assert re.search(r"global_load_dwordx4", body) and re.search(r"global_store_dwordx4", body)  # 16-byte lanes in and out
        assert re.search(r"global_atomic_add_x2", body)  # the block's pixel sum: one 64-bit atomic
    if kernel == "k_glyph_bbox":
        assert re.search(r"global_atomic_[su]?min", body) and re.search(r"global_atomic_[su]?max", body)


def test_the_blend_is_not_fused(code_object):
    """float(a) + alpha * float(b - a) with two roundings: v_mul_f32 and v_add_f32, never v_fma / v_fmac / v_mad on the
    samples.  (The 64-bit division of the mean converts through floats and may use v_fmamk / v_fmaak with a literal: those
    are not the blend.)"""
    body, _ = body_and_metadata(code_object, "k_glyph_enhance")
    assert re.search(r"\bv_(pk_)?mul_f32", body) and re.search(r"\bv_(pk_)?add_f32", body)
    fused = re.findall(r"\bv_(?:pk_)?(?:fma|fmac|mad|mac)_(?:legacy_)?f32\w*", body)
    assert not fused, sorted(set(fused))


def test_kernel_objects_are_separate_translation_units():
    """the Makefile and tools/build_variant.sh link the glyph kernels' object, and the host-only planning code's, next to
    the older ones, whose rules do not depend on the new files; both new objects are built without contraction"""
    with open(os.path.join(ROOT, "bnn-pynq_amd", "Makefile")) as f:
        mk = f.read()
    assert re.search(r"^\$\(OBJ\)/glyph_kernels\.o: csrc/glyph_kernels\.hip.*\n\t.*-ffp-contract=off", mk, re.M)
    assert re.search(r"^\$\(OBJ\)/glyphs\.o: csrc/glyphs\.cpp.*\n\t.*-ffp-contract=off", mk, re.M)
    assert re.search(r"^\$\(LIBDIR\)/python_sw-%.*\$\(OBJ\)/glyph_kernels\.o \$\(OBJ\)/glyphs\.o", mk, re.M)
    for older in ("kernels", "ecc_kernels", "repair_kernels", "wecc_kernels", "iwecc_kernels", "window_kernels", "windows", "preprocess"):
        assert "glyph" not in re.search(r"^\$\(OBJ\)/%s\.o: (.*)$" % older, mk, re.M).group(1), older
    with open(os.path.join(ROOT, "tools", "build_variant.sh")) as f:
        sh = f.read()
    assert "build/glyph_kernels.o" in sh and "build/glyphs.o" in sh
    for f in ("glyphs.h", "glyphs.cpp"):  # the planning code is host-only: no HIP in it
        with open(os.path.join(ROOT, "bnn-pynq_amd", "csrc", f)) as fh:
            text = fh.read()
            assert "#include <hip" not in text and "__global__" not in text and "__device__" not in text, f
