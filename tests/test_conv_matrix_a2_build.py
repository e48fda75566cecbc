"""CPU build check of the matrix forms of cnvW1A2 / cnvW2A2 layers 1-3 (k_conv_mfma_a2, DESIGN.md 5 "The matrix pipe") in
the BUILT gfx950 code object: the three instantiations with the MFMA and ds_read_b128 counts the tiling implies, no
scratch, no spills, VGPRs and LDS that leave two blocks per CU; the three cnvW1A1 bodies still there under their names;
bnn_mi355x_matrix_stages declared and exported; and the encoding rule of the operand expansion (restated in numpy from
the rule in kernels.hip: nibble = 2 * [non-zero] + 8 * [non-zero & sign]) against test_gpu_layers.unpack."""
import ctypes
import os
import re

import numpy as np
import pytest

import gpu_lib as gl
from test_conv_matrix_build import LDS_PER_CU, code_object  # noqa: F401  (the fixture: disassembly + notes of kernels.o)
from test_gpu_layers import unpack

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# template arguments -> (MFMAs per tile: 9 taps x 2 rows x Cin/64; ds_read_b128 per tile: 3 columns x 4 rows x Cin/64)
A2 = {"30, 2, 2, true, 2": (18, 12), "14, 2, 4, false, 8": (18, 12), "12, 4, 4, true, 8": (36, 24)}
FP4 = {0x0: 0.0, 0x2: 1.0, 0xA: -1.0, 0xC: -2.0, 0x8: -0.0}  # the E2M1 codes the tables and the expansion may produce


def body_of(dis, kernel, args):
    m = re.search(r"<void bnn::\(anonymous namespace\)::%s<%s>\(.*?>:\n(.*?)(?=\n[0-9a-f]+ <[^L]|\Z)" % (kernel, re.escape(args)), dis, re.S)
    assert m, "%s<%s> not in the code object" % (kernel, args)
    return m.group(1)


def metadata(notes, kernel, args):
    m = re.search(r"\.name:\s+void bnn::\(anonymous namespace\)::%s<%s>" % (kernel, re.escape(args)), notes)
    assert m, args
    start = notes.rfind(".agpr_count", 0, m.start())
    nxt = notes.find(".agpr_count", m.end())
    blk = notes[start:nxt if nxt > 0 else len(notes)]
    return {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*$", blk, re.M)}


@pytest.mark.parametrize("args", sorted(A2))
def test_a2_matrix_forms_in_the_code_object(code_object, args):  # noqa: F811
    dis, notes = code_object
    body = body_of(dis, "k_conv_mfma_a2", args)
    mfma, reads = A2[args]
    assert len(re.findall(r"\bv_mfma_scale_f32_32x32x64_f8f6f4\b", body)) == mfma
    assert len(re.findall(r"\bds_read_b128\b", body)) == reads
    assert not re.search(r"\bscratch_|\bbuffer_store", body), "scratch traffic"
    md = metadata(notes, "k_conv_mfma_a2", args)
    print(args, {k: md[k] for k in ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size") if k in md})
    assert md["private_segment_fixed_size"] == 0 and md["vgpr_spill_count"] == 0 and md["sgpr_spill_count"] == 0
    assert md["vgpr_count"] + md.get("agpr_count", 0) <= 256                 # two waves per SIMD: two blocks of 4 waves per CU
    assert 2 * md["group_segment_fixed_size"] <= LDS_PER_CU                  # two blocks per CU


@pytest.mark.parametrize("args", sorted(A2))
def test_w1a1_matrix_forms_keep_their_names(code_object, args):  # noqa: F811
    dis, _ = code_object
    body = body_of(dis, "k_conv_mfma", args)
    assert len(re.findall(r"\bv_mfma_scale_f32_32x32x64_f8f6f4\b", body)) == A2[args][0]


def test_table_kernels_in_the_code_object(code_object):  # noqa: F811
    dis, _ = code_object
    for flavour in ("true", "false"):
        assert "k_conv_mfma_a2_table<%s>" % flavour in dis


def test_matrix_stages_declared_and_exported():
    with open(os.path.join(ROOT, "include", "bnn_mi355x.h")) as f:
        assert re.search(r"^int bnn_mi355x_matrix_stages\(int n_images\);", f.read(), re.M)
    for network in ("cnvW1A1", "cnvW1A2", "cnvW2A2"):
        lib = ctypes.CDLL(gl.lib_path(network))
        assert hasattr(lib, "bnn_mi355x_matrix_stages"), network
        lib.bnn_mi355x_matrix_stages.restype = ctypes.c_int
        assert lib.bnn_mi355x_matrix_stages(4096) == -1, network  # nothing loaded yet


def test_policy_edges_of_the_2bit_nets():
    """each net's edge is a committed constant in the measured range, and both lanes of a forked 131 072-image pass
    (65 536 images each) take the matrix forms; the cnvW1A1 function keeps its text (tests/test_conv_matrix_build.py)"""
    with open(os.path.join(ROOT, "bnn-pynq_amd", "csrc", "kernels.hip")) as f:
        src = f.read()
    m = re.search(r"constexpr long long kConvMfmaMinW1A2 = (\d+), kConvMfmaMinW2A2 = (\d+);", src)
    assert m
    for v in m.groups():
        assert 1 < int(v) <= 65536


# ---- the encoding: kernels.hip nibble_spread / fp4_planes / k_conv_mfma_a2_table, restated ----
def nibble_spread(byte):
    """bit i of a byte -> 0x1 in nibble i of a dword"""
    return sum(((int(byte) >> i) & 1) << (4 * i) for i in range(8))


def expand_byte(sign, nz):
    """what fp4_planes makes of one source byte pair: lutz[nz] | luts[sign & nz]"""
    return (nibble_spread(nz) << 1) | (nibble_spread(sign & nz) << 3)


def decode(dword):
    return [FP4[(dword >> (4 * i)) & 15] for i in range(8)]


def test_activation_expansion_decodes_to_unpack():
    """every (sign, non-zero) byte pair: the 8 FP4 nibbles decode to the values unpack() reads from the same bits
    (the sign bit of a zero activation ignored: the nibble is +0, never -0)"""
    for sign in range(256):
        for nz in range(256):
            raw = np.zeros(2, np.uint64)           # one pixel, 64 channels: [sign, non-zero]
            raw[0], raw[1] = sign, nz
            want = unpack(raw, 1, 64, 2)[:8]
            d = expand_byte(sign, nz)
            assert all((d >> (4 * i)) & 15 in (0x0, 0x2, 0xA) for i in range(8))
            assert decode(d) == want.tolist(), (sign, nz)


def test_weight_encoding_rule():
    """the table rule for cnvW2A2 rows (sign, non-zero, "is -2" planes; a -2 column is set in all three) and for cnvW1A2
    rows (bit = 1 <=> -1), per bit"""
    for sg, nz, two, want in ((0, 0, 0, 0.0), (1, 0, 0, 0.0), (0, 1, 0, 1.0), (1, 1, 0, -1.0), (1, 1, 1, -2.0)):
        nzz = nz | two
        b1, b2, b3 = nzz & ~two & 1, two, (sg & nzz) | two
        code = (b1 << 1) | (b2 << 2) | (b3 << 3)
        assert FP4[code] == want and not (want == 0 and code != 0), (sg, nz, two)
    for bit, want in ((0, 1.0), (1, -1.0)):
        assert FP4[(1 << 1) | (bit << 3)] == want
