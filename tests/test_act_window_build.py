"""CPU build check of the windowed first stage of activation-fault sweeps (k_win_x / k_win) in the BUILT
gfx950 code object: every instantiation present under its name -- layers 1, 2 and 3 for 1-bit and 2-bit activations,
cnvW2A2's being the -2-aware forms (they test every pair of rows' flag) --, none with scratch, a private segment or
spills, the xor / bcnt chain of the layer's synapses in the 1-bit bodies; and the two switches read inside the sweep, at every call."""
import os
import re

import pytest

from test_conv_matrix_build import ROOT, code_object  # noqa: F401  (the fixture)

# <CW, ID, POOL> of the layer after the site: layer 1 (30 x 30 x 64 in, pooled), layer 2 (14 x 14 x 64), layer 3 (12 x 12 x 128, pooled)
LAYERS = ["1, 30, true", "1, 14, false", "2, 12, true"]
AR_TB, AR_TT = 2, 3
KERNELS = ["k_win_x<%s>" % l for l in LAYERS] + ["k_win<%d, %s>" % (ar, l) for ar in (AR_TB, AR_TT) for l in LAYERS]


def kernel_body(dis, name):
    m = re.search(r"<void bnn::\(anonymous namespace\)::%s\(.*?>:\n(.*?)(?=\n[0-9a-f]+ <[^L]|\Z)" % re.escape(name), dis, re.S)
    assert m, "%s not in the code object" % name
    return m.group(1)


def metadata(notes, name):
    m = re.search(r"\.name:\s+void bnn::\(anonymous namespace\)::%s\(" % re.escape(name), notes)
    assert m, name
    start = notes.rfind(".agpr_count", 0, m.start())
    nxt = notes.find(".agpr_count", m.end())
    blk = notes[start:nxt if nxt > 0 else len(notes)]
    return {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*$", blk, re.M)}


@pytest.mark.parametrize("name", KERNELS)
def test_window_forms_in_the_code_object(code_object, name):  # noqa: F811
    dis, notes = code_object
    body = kernel_body(dis, name)
    assert not re.search(r"\bscratch_|\bbuffer_store", body), "scratch traffic"
    md = metadata(notes, name)
    assert md["private_segment_fixed_size"] == 0 and md["vgpr_spill_count"] == 0 and md["sgpr_spill_count"] == 0
    assert md["group_segment_fixed_size"] == 0 and md["max_flat_workgroup_size"] == 256
    assert md["vgpr_count"] + md.get("agpr_count", 0) <= 128  # (four waves a SIMD at least)
    if name.startswith("k_win_x"):  # two neurons per iteration, each 9 * CW words = 18 * CW (v_xor, v_bcnt) pairs
        cw = int(name[len("k_win_x<")])
        assert len(re.findall(r"\bv_bcnt_u32_b32\b", body)) == 2 * 18 * cw
        assert len(re.findall(r"\bv_xor_b32", body)) >= 2 * 18 * cw


def test_switches_are_read_inside_the_sweep():
    with open(os.path.join(ROOT, "bnn-pynq_amd", "csrc", "runtime.hip")) as f:
        src = f.read()
    body = re.search(r"\nstatic long single_fault_sweep\(.*?\n\}\n", src, re.S).group(0)
    for name in ("BNN_MI355X_ACT_WINDOW", "BNN_MI355X_SWEEP_GROUP"):
        assert src.count('getenv("%s")' % name) == 1 and 'getenv("%s")' % name in body, name
    # ... in the function's body (every call), not in a static initialiser
    for line in body.splitlines():
        if "getenv(" in line:
            assert not re.match(r"\s*static\b", line), line
    with open(os.path.join(ROOT, "include", "bnn_mi355x.h")) as f:
        hdr = f.read()
    assert "BNN_MI355X_ACT_WINDOW" in hdr and "BNN_MI355X_SWEEP_GROUP" in hdr
