"""CPU build check of the window kernel (csrc/window_kernels.hip) in the BUILT gfx950 code object: the three
band forms of k_windows_to_cifar are there, use no scratch, spill nothing, and their LDS is the bound the headers state
(csrc/windows.h: kWindowMidBytes + kWindowOutBytes; include/bnn_mi355x.h: BNN_MI355X_WINDOW_LDS_BYTES, at most 64 KB)."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJ = os.path.join(ROOT, "bnn-pynq_amd", "build", "window_kernels.o")
LLVM = "/opt/rocm/llvm/bin"
BANDS = [1, 3, 4]


def stated(path, pattern):
    with open(os.path.join(ROOT, path)) as f:
        m = re.search(pattern, f.read())
    assert m, "%s does not state %s" % (path, pattern)
    return int(m.group(1))


@pytest.fixture(scope="module")
def code_object():
    if not os.path.exists(OBJ):  # a tree that arrived with prebuilt libraries only: rebuild the object (hipcc cross-compiles)
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "bnn-pynq_amd"), "build/window_kernels.o"], check=True)
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


def test_the_stated_bounds_agree():
    mid = stated("bnn-pynq_amd/csrc/windows.h", r"constexpr int kWindowMidBytes = (\d+);")
    out = stated("bnn-pynq_amd/csrc/windows.h", r"constexpr int kWindowOutBytes = (\d+);")
    assert stated("include/bnn_mi355x.h", r"#define BNN_MI355X_WINDOW_LDS_BYTES (\d+)") == mid
    assert out >= 32 * 32 * 4  # the resampled window at its largest, RGBA
    assert mid + out <= 64 * 1024


@pytest.mark.parametrize("bands", BANDS)
def test_kernels_in_the_code_object(code_object, bands):
    dis, notes = code_object
    name = r"void bnn::\(anonymous namespace\)::k_windows_to_cifar<%d>\(" % bands
    m = re.search(r"<%s.*?>:\n(.*?)(?=\n[0-9a-f]+ <[^L]|\Z)" % name, dis, re.S)
    assert m, "k_windows_to_cifar<%d> not in the code object" % bands
    body = m.group(1)
    assert not re.search(r"\bscratch_", body), "scratch traffic"
    assert re.search(r"\bds_(read|write|load|store)", body) and "s_barrier" in body  # the intermediate goes through LDS
    n = re.search(r"\.name:\s+%s" % name, notes)
    assert n
    start = notes.rfind(".agpr_count", 0, n.start())
    nxt = notes.find(".agpr_count", n.end())
    md = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*$", notes[start:nxt if nxt > 0 else len(notes)], re.M)}
    print({k: md[k] for k in ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size", "kernarg_segment_size")})
    assert md["private_segment_fixed_size"] == 0 and md["vgpr_spill_count"] == 0 and md["sgpr_spill_count"] == 0
    bound = stated("bnn-pynq_amd/csrc/windows.h", r"constexpr int kWindowMidBytes = (\d+);") + \
        stated("bnn-pynq_amd/csrc/windows.h", r"constexpr int kWindowOutBytes = (\d+);")
    assert 0 < md["group_segment_fixed_size"] <= bound <= 64 * 1024
    assert md["max_flat_workgroup_size"] == 256


def test_kernel_objects_are_separate_translation_units():
    """the Makefile and tools/build_variant.sh link the window kernel's object, and the host-only planning code's, next to
    the older ones (whose byte-identity with the parent's build is recorded in CHANGELOG.md: a test cannot build the
    parent commit from a tree without its history)"""
    with open(os.path.join(ROOT, "bnn-pynq_amd", "Makefile")) as f:
        mk = f.read()
    assert re.search(r"^\$\(OBJ\)/window_kernels\.o: csrc/window_kernels\.hip", mk, re.M)
    assert re.search(r"^\$\(OBJ\)/windows\.o: csrc/windows\.cpp", mk, re.M)
    assert re.search(r"^\$\(LIBDIR\)/python_sw-%.*\$\(OBJ\)/window_kernels\.o \$\(OBJ\)/windows\.o", mk, re.M)
    for older in ("kernels", "ecc_kernels", "repair_kernels", "wecc_kernels", "iwecc_kernels", "preprocess", "resample"):
        assert "window" not in re.search(r"^\$\(OBJ\)/%s\.o: (.*)$" % older, mk, re.M).group(1), older
    with open(os.path.join(ROOT, "tools", "build_variant.sh")) as f:
        sh = f.read()
    assert "build/window_kernels.o" in sh and "build/windows.o" in sh
    # the planning code is host-only: no HIP in it
    for f in ("windows.h", "windows.cpp"):
        with open(os.path.join(ROOT, "bnn-pynq_amd", "csrc", f)) as fh:
            text = fh.read()
            assert "#include <hip" not in text and "__global__" not in text and "__device__" not in text, f
