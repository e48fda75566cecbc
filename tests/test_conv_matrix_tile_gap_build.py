"""CPU build check of the gap between two tiles of the matrix forms of cnvW1A1 layers 1-3 (k_conv_mfma, DESIGN.md 5
"The matrix pipe") in the BUILT gfx950 code object: the item -> (image, row pair, column) arithmetic is carried from
tile to tile, so no v_mul_hi (division by a constant) is left between the tile loop's head and its back branch, and the
VALU instructions between the head and the tile's first MFMA are fewer than the 19 they were, as many as DESIGN.md
states.  (The packed sign collection by v_cvt_scalef32_pk_fp4_f32 was built, measured slower in every layer and not
kept, CHANGELOG: the loop keeps its v_alignbit_b32 chain and there is nothing of the conversion to check; layer 2's two
rows share one half swap.)"""
import os
import re

import pytest

from test_conv_matrix_build import KERNELS, ROOT, code_object, kernel_body  # noqa: F401 (fixture)
from test_conv_matrix_epilogue_build import LAYERS, is_valu, tile_loop

TOP_BEFORE = 19           # VALU between the loop head and the first MFMA with the divisions (CHANGELOG)


def design_top():
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        text = " ".join(f.read().split())
    m = re.search(r"VALU instructions between the tile loop's head and the tile's first MFMA \(layers 1 / 2 / 3\): (\d+) / (\d+) / (\d+)", text)
    assert m, "DESIGN.md 5 does not state the figures checked here"
    return [int(x) for x in m.groups()]


@pytest.mark.parametrize("layer", range(3))
def test_no_division_in_the_tile_loop(code_object, layer):
    dis, _ = code_object
    ins, mf, head, back = tile_loop(kernel_body(dis, LAYERS[layer]))
    assert len(mf) == KERNELS[LAYERS[layer]][0] and head < mf[0] < mf[-1] < back
    assert not [x for _, x in ins[head:back + 1] if x.startswith("v_mul_hi")]


@pytest.mark.parametrize("layer", range(3))
def test_valu_in_front_of_the_first_mfma(code_object, layer):
    dis, _ = code_object
    ins, mf, head, back = tile_loop(kernel_body(dis, LAYERS[layer]))
    n = sum(1 for _, x in ins[head:mf[0]] if is_valu(x))
    print("layer %d: %d VALU between the loop head and the first MFMA (%d before)" % (layer + 1, n, TOP_BEFORE))
    assert n < TOP_BEFORE
    assert n == design_top()[layer]


def test_layer2_rows_share_one_half_swap(code_object):
    dis, _ = code_object
    ins, mf, head, back = tile_loop(kernel_body(dis, LAYERS[1]))
    assert sum(1 for _, x in ins[head:back + 1] if x.startswith("v_permlane32_swap")) == 1
