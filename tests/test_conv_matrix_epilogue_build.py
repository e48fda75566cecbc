"""CPU build check of the tile epilogue of the matrix forms of cnvW1A1 layers 1-3 (k_conv_mfma, DESIGN.md 5 "The matrix
pipe") in the BUILT gfx950 code object: the vertical pool is an AND of the accumulators' bits (no v_max_f32 in layers 1
and 3), the VALU instructions a tile issues with no MFMA in flight behind it -- between its last MFMA and the tile
loop's back branch -- are as many as DESIGN.md states, fewer than before the AND where there is a pool, and where
DESIGN.md says an instantiation defers its epilogue, the deferred part sits between the tile's first and last MFMA."""
import os
import re

import pytest

from test_conv_matrix_build import KERNELS, ROOT, code_object, kernel_body, metadata  # noqa: F401 (fixture)

LAYERS = ("30, 2, 2, true, 2", "14, 2, 4, false, 8", "12, 4, 4, true, 8")  # layers 1 / 2 / 3
POOLED = (True, False, True)
BEFORE = (84, 57, 84)  # VALU between the last MFMA and the back branch when the pool was fmaxf (CHANGELOG)


def design():
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        text = " ".join(f.read().split())
    m = re.search(r"VALU instructions between a tile's last MFMA and the loop's back branch \(layers 1 / 2 / 3\): (\d+) / (\d+) / (\d+)", text)
    d = re.search(r"deferred epilogue \(layers 1 / 2 / 3\): (none|full|packed) / (none|full|packed) / (none|full|packed)", text)
    assert m and d, "DESIGN.md 5 does not state the figures checked here"
    return [int(x) for x in m.groups()], list(d.groups())


def tile_loop(body):
    """[(address, instruction)] of the kernel, the indices of its MFMAs and the index of the tile loop's back branch:
    the last backward branch behind the last MFMA whose target is the nearest one in front of the tile's first read"""
    ins = []
    for ln in body.split("\n"):
        m = re.match(r"\s*(\S.*?)\s*//\s*([0-9A-F]+):", ln)
        if m:
            ins.append((int(m.group(2), 16), m.group(1)))
    mf = [i for i, (_, x) in enumerate(ins) if x.startswith("v_mfma_scale_f32_32x32x64_f8f6f4")]
    first_read = next(a for a, x in ins[:mf[0]][::-1] if x.startswith("ds_read_b128"))
    back = {}
    for i in range(mf[-1], len(ins)):
        m = re.match(r"s_c?branch\S*\s+(\d+)", ins[i][1])
        if m and int(m.group(1)) >= 32768:
            target = ins[i][0] + 4 + 4 * (int(m.group(1)) - 65536)
            if target <= first_read:
                back.setdefault(target, []).append(i)
    head = max(back)
    return ins, mf, next(i for i, (a, _) in enumerate(ins) if a == head), back[head][-1]


def is_valu(x):
    return x.startswith("v_") and not x.startswith("v_mfma")


def test_design_states_what_is_checked_here():
    after, deferred = design()
    for a, b, pool in zip(after, BEFORE, POOLED):
        assert a < b if pool else a <= b


@pytest.mark.parametrize("layer", range(3))
def test_pool_is_an_and(code_object, layer):
    dis, _ = code_object
    body = kernel_body(dis, LAYERS[layer])
    if POOLED[layer]:
        assert not re.search(r"\bv_max_f32\b", body)
        ins, mf, head, back = tile_loop(body)
        assert sum(1 for _, x in ins[head:back] if x.startswith("v_and_b32")) >= 16


@pytest.mark.parametrize("layer", range(3))
def test_valu_behind_the_last_mfma(code_object, layer):
    dis, _ = code_object
    ins, mf, head, back = tile_loop(kernel_body(dis, LAYERS[layer]))
    assert len(mf) == KERNELS[LAYERS[layer]][0] and head < mf[0] < mf[-1] < back
    n = sum(1 for _, x in ins[mf[-1] + 1:back] if is_valu(x))
    print("layer %d: %d VALU between the last MFMA and the back branch (%d before)" % (layer + 1, n, BEFORE[layer]))
    assert n == design()[0][layer]


@pytest.mark.parametrize("layer", range(3))
def test_deferred_part_is_behind_mfmas(code_object, layer):
    dis, _ = code_object
    kind = design()[1][layer]
    ins, mf, head, back = tile_loop(kernel_body(dis, LAYERS[layer]))
    loop = range(head, back)
    if kind == "full":      # the whole sign collection
        moved = [i for i in loop if ins[i][1].startswith("v_alignbit_b32")]
    elif kind == "packed":  # the half swap and the item -> (image, row pair, column) divisions of the store address
        moved = [i for i in loop if ins[i][1].startswith(("v_permlane32_swap", "v_mul_hi_"))]
    else:                   # nothing deferred: the epilogue follows the tile's last MFMA
        assert all(i > mf[-1] for i in loop if ins[i][1].startswith(("v_alignbit_b32", "v_permlane32_swap")))
        return
    assert moved and all(mf[0] < i < mf[-1] for i in moved)
