"""CPU build check of the column-interleaved coded weight memories' kernels (csrc/iwecc_kernels.hip) in the
BUILT gfx950 code object: k_iwmem_noise_w<false>, k_iwmem_noise_w<true> and k_iwrepair_state are there, use no scratch, spill
nothing, have no LDS, and their VGPR counts are the ones DESIGN.md states.  The exchange is cross-lane moves alone."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJ = os.path.join(ROOT, "bnn-pynq_amd", "build", "iwecc_kernels.o")
LLVM = "/opt/rocm/llvm/bin"
NAMES = [r"void bnn::\(anonymous namespace\)::k_iwmem_noise_w<false>\(", r"void bnn::\(anonymous namespace\)::k_iwmem_noise_w<true>\(",
         r"bnn::\(anonymous namespace\)::k_iwrepair_state\("]
DESIGN_NAMES = ["k_iwmem_noise_w<false>", "k_iwmem_noise_w<true>", "k_iwrepair_state"]


@pytest.fixture(scope="module")
def code_object():
    if not os.path.exists(OBJ):  # a tree that arrived with prebuilt libraries only: rebuild the object (hipcc cross-compiles)
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "bnn-pynq_amd"), "build/iwecc_kernels.o"], check=True)
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


def design_vgprs(name):
    """the VGPR count DESIGN.md 9 states for a kernel: '`name`: N VGPRs'"""
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        m = re.search(r"`%s`: (\d+) VGPRs" % re.escape(name), f.read())
    assert m, "DESIGN.md does not state the VGPRs of " + name
    return int(m.group(1))


@pytest.mark.parametrize("NAME,DNAME", list(zip(NAMES, DESIGN_NAMES)))
def test_kernels_in_the_code_object(code_object, NAME, DNAME):
    dis, notes = code_object
    m = re.search(r"<%s.*?>:\n(.*?)(?=\n[0-9a-f]+ <[^L]|\Z)" % NAME, dis, re.S)
    assert m, NAME + " not in the code object"
    body = m.group(1)
    # (the exchanges and the wave reductions are cross-lane ds_bpermute / ds_swizzle / DPP moves: no LDS memory is allocated
    # or addressed)
    assert not re.search(r"\bscratch_|\bbuffer_|\bds_(read|write|load|store)", body), "scratch, buffer or LDS traffic"
    cross = len(re.findall(r"\bds_(bpermute|swizzle)|_dpp\b|v_permlane", body))
    print(DNAME, "instructions:", len(body.splitlines()), "cross-lane:", cross)
    assert cross > 0
    n = re.search(r"\.name:\s+%s" % NAME, notes)
    assert n
    start = notes.rfind(".agpr_count", 0, n.start())
    nxt = notes.find(".agpr_count", n.end())
    md = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*$", notes[start:nxt if nxt > 0 else len(notes)], re.M)}
    print({k: md[k] for k in ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size", "kernarg_segment_size")})
    assert md["private_segment_fixed_size"] == 0 and md["vgpr_spill_count"] == 0 and md["sgpr_spill_count"] == 0
    assert md["group_segment_fixed_size"] == 0
    assert md["max_flat_workgroup_size"] == 256
    assert md["vgpr_count"] == design_vgprs(DNAME)


def test_kernel_objects_are_separate_translation_units():
    """the Makefile and tools/build_variant.sh link the interleaved kernels' object next to the four older ones (whose
    byte-identity with the parent's build is recorded in CHANGELOG.md: a test cannot build the parent commit from a tree
    without its history)"""
    with open(os.path.join(ROOT, "bnn-pynq_amd", "Makefile")) as f:
        mk = f.read()
    assert re.search(r"^\$\(OBJ\)/iwecc_kernels\.o: csrc/iwecc_kernels\.hip", mk, re.M)
    assert re.search(r"^\$\(LIBDIR\)/python_sw-%.*\$\(OBJ\)/iwecc_kernels\.o", mk, re.M)
    for older in ("kernels", "ecc_kernels", "repair_kernels", "wecc_kernels"):
        assert "iwecc" not in re.search(r"^\$\(OBJ\)/%s\.o: (.*)$" % older, mk, re.M).group(1), older
    with open(os.path.join(ROOT, "tools", "build_variant.sh")) as f:
        assert "build/iwecc_kernels.o" in f.read()
