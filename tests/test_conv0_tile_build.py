"""CPU build check of layer 0's tile form (k_conv0_tile, DESIGN.md 5 "Layer 0: the tile loop") in the BUILT gfx950 code
object, for the two product forms and the two campaign (MULTI) forms: no scratch and no spills, registers and LDS that
leave two waves per SIMD, and a tile loop of 4 MFMAs (6 with two thresholds), 32 (64) sign-collection instructions and
as many VALU instructions as DESIGN.md states -- fewer than the loop held before the round-24 rework -- whose waits on
LDS all stand in front of the tile's first MFMA (the next tile's fetches are in flight behind it)."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJ = os.path.join(ROOT, "bnn-pynq_amd", "build", "kernels.o")
LLVM = "/opt/rocm/lib/llvm/bin"
# template arguments -> VALU instructions in the tile loop of the build before the rework, counted by loop_counts() below
# on that build's object (the <false, false> loop: 32 sign collection, 5 v_alignbyte, 6 LDS addressing, 1 v_cndmask,
# 4 half merge, 2 store address)
BEFORE = {"false, false": 50, "true, false": 90, "false, true": 50, "true, true": 90}
LDS_PER_CU = 160 * 1024
VGPRS_PER_SIMD = 512
WAVES_PER_BLOCK = 4


@pytest.fixture(scope="module")
def code_object():
    if not os.path.exists(OBJ):  # a tree that arrived with prebuilt libraries only: rebuild the object (hipcc cross-compiles)
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "bnn-pynq_amd"), "build/kernels.o"], check=True)
    return disassemble(OBJ)


def disassemble(obj):
    d = tempfile.mkdtemp()
    try:
        shutil.copy(obj, os.path.join(d, "k.o"))
        subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", "k.o"], cwd=d, check=True, capture_output=True)
        co = os.path.join(d, next(f for f in os.listdir(d) if "gfx950" in f))
        dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--symbolize-operands", "--no-show-raw-insn", co], check=True,
                             capture_output=True, text=True).stdout
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
        dem = subprocess.run(["c++filt"], input=dis + "\n@@@\n" + notes, check=True, capture_output=True, text=True).stdout
        return dem.split("\n@@@\n")
    finally:
        shutil.rmtree(d)


def kernel_body(dis, args):
    m = re.search(r"<void bnn::\(anonymous namespace\)::k_conv0_tile<%s>\(.*?>:\n(.*?)(?=\n[0-9a-f]+ <[^L]|\Z)" % re.escape(args), dis, re.S)
    assert m, "k_conv0_tile<%s> not in the code object" % args
    return m.group(1)


def metadata(notes, args):
    m = re.search(r"\.name:\s+void bnn::\(anonymous namespace\)::k_conv0_tile<%s>" % re.escape(args), notes)
    assert m, args
    start = notes.rfind(".agpr_count", 0, m.start())
    nxt = notes.find(".agpr_count", m.end())
    blk = notes[start:nxt if nxt > 0 else len(notes)]
    return {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*$", blk, re.M)}


def tile_loop(body):
    """the instructions of the tile loop, in address order: from the label the branch behind the last MFMA goes back to,
    through the last branch back to it"""
    lines = [ln.strip() for ln in body.splitlines() if ln.strip()]
    label_at = {m.group(1): i for i, ln in enumerate(lines) for m in [re.match(r"[0-9a-f]+ <(L\d+)>:", ln)] if m}
    mfma = [i for i, ln in enumerate(lines) if ln.startswith("v_mfma")]
    assert mfma, "no MFMA"
    back = [(i, m.group(1)) for i, ln in enumerate(lines) for m in [re.match(r"s_c?branch\w*\s+(L\d+)", ln)]
            if m and i > mfma[-1] and label_at[m.group(1)] < mfma[0]]
    assert back, "no branch back over the MFMAs"
    head = max(label_at[lbl] for _, lbl in back)   # the innermost loop around them
    last = max(i for i, lbl in back if label_at[lbl] == head)
    return [ln.split("//")[0].strip() for ln in lines[head + 1:last + 1] if not re.match(r"[0-9a-f]+ <", ln)]


def loop_counts(body):
    ins = tile_loop(body)
    op = [ln.split()[0] for ln in ins]
    first = next(i for i, o in enumerate(op) if o.startswith("v_mfma"))
    last = max(i for i, o in enumerate(op) if o.startswith("v_mfma"))
    return {
        "mfma": sum(o.startswith("v_mfma") for o in op),
        "valu": sum(o.startswith("v_") and not o.startswith("v_mfma") for o in op),
        # the chains' v_alignbit_b32 and their leading v_lshrrev_b32 by 31
        "sign": sum(o.startswith("v_alignbit_b32") or bool(re.match(r"v_lshrrev_b32\w*\s+v\d+, 31,", ln)) for o, ln in zip(op, ins)),
        "alignbyte_before_mfma": sum(o.startswith("v_alignbyte_b32") for o in op[:first]),
        "waits_among_mfma": [ln for o, ln in zip(op[first:last + 1], ins[first:last + 1]) if o == "s_waitcnt"],
    }


def designed_valu():
    """"... the tile loop of k_conv0_tile holds N VALU instructions (M with two thresholds)" """
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        m = re.search(r"the tile loop of k_conv0_tile holds (\d+) VALU instructions \((\d+) with two thresholds\)", f.read())
    assert m, "DESIGN.md does not state the tile loop's VALU count"
    return {False: int(m.group(1)), True: int(m.group(2))}


@pytest.mark.parametrize("args", sorted(BEFORE))
def test_tile_form_in_the_code_object(code_object, args):
    dis, notes = code_object
    body = kernel_body(dis, args)
    out2 = args.startswith("true")
    assert not re.search(r"\bscratch_|\bbuffer_store", body), "scratch traffic"
    md = metadata(notes, args)
    assert md["private_segment_fixed_size"] == 0 and md["vgpr_spill_count"] == 0 and md["sgpr_spill_count"] == 0
    regs = md["vgpr_count"] + md.get("agpr_count", 0)
    by_regs = VGPRS_PER_SIMD // ((regs + 7) // 8 * 8)
    by_lds = (LDS_PER_CU // md["group_segment_fixed_size"]) * WAVES_PER_BLOCK // 4  # blocks per CU x waves per block / 4 SIMDs
    assert min(by_regs, by_lds) >= 2, (regs, md["group_segment_fixed_size"])
    c = loop_counts(body)
    assert c["mfma"] == (6 if out2 else 4)
    assert c["sign"] == (64 if out2 else 32)
    assert c["valu"] < BEFORE[args]
    assert c["valu"] == designed_valu()[out2], c["valu"]
    # the next tile's fetches are issued behind the first MFMAs: nothing waits for them before the tile's last MFMA
    for w in c["waits_among_mfma"]:
        m = re.fullmatch(r"s_waitcnt lgkmcnt\((\d+)\)", w)
        assert m and int(m.group(1)) > 0, w
