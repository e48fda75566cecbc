"""CPU build check of the matrix forms of CNV layers 4-7 (k_tail_mfma, DESIGN.md 5 "The matrix pipe") in the BUILT gfx950
code object: every instantiation present under its name, the v_mfma_scale_f32_32x32x64_f8f6f4 count of one tile, no
scratch and no spills, registers and LDS that fit the occupancy the launch bounds claim, the table kernels, the committed
policy edges, and the export that tells which path a size takes."""
import ctypes
import os
import re

import pytest

from test_conv_matrix_build import LDS_PER_CU, ROOT, code_object  # noqa: F401  (the fixture)

# template arguments <A2, KS, NT, CONV, WAVES, G> -> (k steps, neuron tiles per wave = NT / WAVES, blocks per CU claimed by
# __launch_bounds__(64 * WAVES, 8 / WAVES)).  One tile = every k step once for each of the wave's neuron tiles.
SHAPES = {"18, 8, true, 8, 32": (18, 1, 1),      # layer 4: K = 9 * 128, 256 neurons, 8 waves x 1 tile
          "36, 8, false, 8, 32": (36, 1, 1),     # layer 5: K = 2304, 256 neurons
          "4, 16, false, 4, 128": (4, 4, 2),     # layer 6: K = 256, 512 neurons, 4 waves x 4 tiles
          "8, 16, false, 8, 128": (8, 2, 1)}     # layer 7: K = 512, 512 neurons, 8 waves x 2 tiles
KERNELS = {"%s, %s" % (a2, args): v for a2 in ("false", "true") for args, v in SHAPES.items()}


def kernel_body(dis, args):
    m = re.search(r"<void bnn::\(anonymous namespace\)::k_tail_mfma<%s>\(.*?>:\n(.*?)(?=\n[0-9a-f]+ <[^L]|\Z)" % re.escape(args), dis, re.S)
    assert m, "k_tail_mfma<%s> not in the code object" % args
    return m.group(1)


def metadata(notes, args):
    m = re.search(r"\.name:\s+void bnn::\(anonymous namespace\)::k_tail_mfma<%s>" % re.escape(args), notes)
    assert m, args
    start = notes.rfind(".agpr_count", 0, m.start())
    nxt = notes.find(".agpr_count", m.end())
    blk = notes[start:nxt if nxt > 0 else len(notes)]
    return {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*$", blk, re.M)}


@pytest.mark.parametrize("args", sorted(KERNELS))
def test_tail_matrix_forms_in_the_code_object(code_object, args):  # noqa: F811
    dis, notes = code_object
    body = kernel_body(dis, args)
    ksteps, tiles_per_wave, blocks = KERNELS[args]
    waves = int(args.split(", ")[4])
    assert len(re.findall(r"\bv_mfma_scale_f32_32x32x64_f8f6f4\b", body)) == ksteps * tiles_per_wave
    assert len(re.findall(r"\bv_mfma_", body)) == ksteps * tiles_per_wave     # (and no other matrix instruction)
    assert not re.search(r"\bscratch_|\bbuffer_store", body), "scratch traffic"
    md = metadata(notes, args)
    assert md["private_segment_fixed_size"] == 0 and md["vgpr_spill_count"] == 0 and md["sgpr_spill_count"] == 0
    # `blocks` blocks of `waves` waves per CU = blocks * waves / 4 waves per SIMD, which share its 512 registers per lane
    assert md["vgpr_count"] + md.get("agpr_count", 0) <= 512 // (blocks * waves // 4)
    assert blocks * md["group_segment_fixed_size"] <= LDS_PER_CU
    assert md["max_flat_workgroup_size"] == 64 * waves


def test_table_kernels_in_the_code_object(code_object):  # noqa: F811
    dis, _ = code_object
    for name in (r"k_conv_mfma_table\(", r"k_conv_mfma_a2_table<true>\(", r"k_conv_mfma_a2_table<false>\("):
        assert re.search(r"<void bnn::\(anonymous namespace\)::%s" % name, dis) or re.search(r"<bnn::\(anonymous namespace\)::%s" % name, dis), name


def test_committed_edges_and_switch():
    with open(os.path.join(ROOT, "bnn-pynq_amd", "csrc", "kernels.hip")) as f:
        src = f.read()
    m = re.search(r"constexpr long long kTailMfmaMinW1A1 = (\d+), kTailMfmaMinW1A2 = (\d+), kTailMfmaMinW2A2 = (\d+);", src)
    assert m and all(1 < int(x) <= 65536 for x in m.groups())
    body = re.search(r"inline long long tail_mfma_min\(\) \{(.*?)\n\}", src, re.S).group(1)
    assert 'getenv("BNN_MI355X_TAIL_MFMA_MIN")' in body
    assert re.search(r"constexpr int kTailMfmaStages = 0xF0;", src)
    # the launcher and the export decide in the same function
    assert len(re.findall(r"tail_mfma_for<ARITH>\(a\)", src)) == 3


@pytest.mark.parametrize("network", ["cnvW1A1", "cnvW1A2", "cnvW2A2"])
def test_matrix_stages_is_exported_and_minus_one_before_load(network):
    lib = ctypes.CDLL(os.path.join(ROOT, "bnn-pynq_amd", "bnn", "libraries", "mi355x", "python_sw-%s-mi355x.so" % network))
    lib.bnn_mi355x_matrix_stages.restype = ctypes.c_int
    assert lib.bnn_mi355x_matrix_stages(8192) == -1
