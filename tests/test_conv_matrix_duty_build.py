"""CPU build check of how the matrix forms of cnvW1A1 layers 1-3 (k_conv_mfma, DESIGN.md 5 "The matrix pipe") keep the
matrix pipe fed, in the BUILT gfx950 code object: block size, resident waves per SIMD as DESIGN.md states them, no
scratch and no spills, B operands requested a step ahead (no wait for ALL LDS reads inside a tile before the MFMA that
consumes the tile's youngest read), and layer 3's padded planes.  (The branch-free expansion was measured and not
kept, CHANGELOG: there is nothing of it to check.)"""
import os
import re

import pytest

from test_conv_matrix_build import KERNELS, LDS_PER_CU, ROOT, code_object, kernel_body, metadata  # noqa: F401 (fixture)

BLOCK = 256
WAVES_PER_SIMD = 2  # two blocks of four waves per CU, one wave of each on every SIMD


def lines_of(body):
    return [re.sub(r"\s*//.*", "", ln).strip() for ln in body.split("\n")]


def waves_per_simd(md):
    regs = -(-(md["vgpr_count"] + md.get("agpr_count", 0)) // 8) * 8   # allocation granule: 8 registers per lane
    by_regs = min(8, 512 // regs)
    blocks = min(LDS_PER_CU // md["group_segment_fixed_size"], 32 * 64 // BLOCK)
    return min(by_regs, blocks * BLOCK // 64 // 4)


def test_design_states_the_occupancy_checked_here():
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        text = f.read()
    assert re.search(r"resident waves per SIMD \(layers 1 / 2 / 3\): %d / %d / %d" % ((WAVES_PER_SIMD,) * 3), " ".join(text.split()))


@pytest.mark.parametrize("args", sorted(KERNELS))
def test_block_size_occupancy_and_no_scratch(code_object, args):
    dis, notes = code_object
    md = metadata(notes, args)
    assert md["max_flat_workgroup_size"] == BLOCK
    assert waves_per_simd(md) == WAVES_PER_SIMD
    assert md["private_segment_fixed_size"] == 0 and md["vgpr_spill_count"] == 0 and md["sgpr_spill_count"] == 0
    assert not re.search(r"\bscratch_|\bbuffer_store", kernel_body(dis, args)), "scratch traffic"


@pytest.mark.parametrize("args", sorted(KERNELS))
def test_b_operands_are_requested_a_step_ahead(code_object, args):
    """between the first MFMA of a tile and its last but one, every s_waitcnt is a counted lgkmcnt(N > 0): reads of the
    next step are in flight behind the one an MFMA consumes.  The last MFMA consumes the youngest LDS read the wave has
    issued, so the wait in front of it is necessarily lgkmcnt(0)."""
    dis, _ = code_object
    ln = lines_of(kernel_body(dis, args))
    mf = [i for i, x in enumerate(ln) if x.startswith("v_mfma_scale_f32_32x32x64_f8f6f4")]
    assert len(mf) == KERNELS[args][0]
    inner = ln[mf[0]:mf[-2]]
    waits = [x for x in inner if x.startswith("s_waitcnt")]
    assert waits, "no counted waits in the tile"
    for w in waits:
        m = re.fullmatch(r"s_waitcnt lgkmcnt\((\d+)\)", w)
        assert m and int(m.group(1)) > 0, w
    assert not any(x.startswith("s_cbranch") or x.startswith("s_barrier") for x in inner)
    # a read of the next step follows the first MFMA of every step but the last
    reads = [i for i, x in enumerate(ln) if x.startswith("ds_read_b128")]
    assert len(reads) == KERNELS[args][1]
    assert sum(1 for i in reads if i > mf[0]) == KERNELS[args][1] - 4


def test_layer3_planes_are_padded(code_object):
    """8 images x 626 slots of 16 bytes (4 channel blocks x 12 rows x 13 slots, + 2) and the 1 KiB LUT"""
    _, notes = code_object
    assert metadata(notes, "12, 4, 4, true, 8")["group_segment_fixed_size"] == 8 * 626 * 16 + 1024
    assert metadata(notes, "30, 2, 2, true, 2")["group_segment_fixed_size"] == 2 * 1800 * 16 + 1024
    assert metadata(notes, "14, 2, 4, false, 8")["group_segment_fixed_size"] == 8 * 392 * 16 + 1024
