"""GPU: form 2 of the clip scan (stages 4 and 5 on the matrix cores too, k_clip_tail_mfma) against the integer kernels,
byte for byte, and the routing.  A band is up to 4 row pairs x 64 columns, a tile 32 pixel pairs.  Stage 4's map is (nx + 2) x (ny + 2),
stage 5's nx x ny: widths 144 .. 160 put both under, at and over 32 columns, 272 .. 288 at 64, heights 48 .. 64 give 7, 8 and 9 rows."""
import os

import numpy as np
import pytest

import gpu_lib as gl
import scan_clip_ref as ref
from test_gpu_scan_clip import check_against_scan_scene
from test_gpu_scan_matrix import L, clip_of, load, param_dirs  # noqa: F401  (L, param_dirs: that module's fixtures)

pytestmark = pytest.mark.gpu

VALU = os.environ.get("BNN_MI355X_CONV") == "valu"  # (no operand tables: the integer kernels run under every form, only the routing is checked)
MASK = {0: 0, 1: 0 if VALU else 0b1110, 2: 0 if VALU else 0b111110}
SHAPES = [(32, (32,), 1, (32,)), (100, (52,), 3, (32, 40))] + [(w, (48, 52, 56, 60, 64), 1, (32,)) for w in range(144, 161, 4)] + \
         [(w, (32, 60), 1, (32,)) for w in range(272, 289, 4)]


def region(L, clip, sizes, stage, form, pdir):
    (frames, h, w), sz = clip.shape[:3], np.asarray(sizes, np.int32)
    out = np.zeros(ref.layout(w, h, sizes, frames)["stage_bytes"][stage], np.uint8)
    load(L, pdir)
    L.bnn_mi355x_scan_form(form)
    assert L.bnn_mi355x_scan_matrix_stages(1) == MASK[form]
    assert L.bnn_mi355x_debug_scan_clip_stage(clip.ctypes.data, frames, 0, w, h, 3, 0, sz.ctypes.data, len(sz), stage, out.ctypes.data,
                                              out.nbytes) == out.nbytes, L.bnn_mi355x_last_error()
    return out


@pytest.mark.parametrize("params", ["cifar10", "random"])
@pytest.mark.parametrize("width,heights,frames,sizes", SHAPES)  # (the picture's width, its heights, frames, window sizes)
def test_stage_maps_equal_the_integer_kernels(L, param_dirs, params, width, heights, frames, sizes):
    """stages 4 and 5, form 2 against form 0; the region is first filled with the maps under the OTHER parameters: a skipped store shows"""
    own, other = param_dirs[params], param_dirs["random" if params == "cifar10" else "cifar10"]
    for h in heights:
        clip = clip_of(frames, width, h)
        for stage in (4, 5):
            want, fill = region(L, clip, sizes, stage, 0, own), region(L, clip, sizes, stage, 0, other)
            assert (want.view(np.uint32) != fill.view(np.uint32)).mean() > 0.5  # (most dwords of the fill are foreign)
            got = region(L, clip, sizes, stage, 2, own)
            assert (want == got).all(), (params, width, h, "stage", stage, "bytes differing", int((want != got).sum()))


@pytest.mark.parametrize("params", ["cifar10", "random"])
@pytest.mark.parametrize("width,height,frames,sizes", [(100, 52, 3, (32, 40)), (156, 60, 1, (32,))])
def test_scores_equal_scan_scene(L, param_dirs, params, width, height, frames, sizes):
    load(L, param_dirs[params])
    L.bnn_mi355x_scan_form(2)
    assert L.bnn_mi355x_scan_matrix_stages(1) == MASK[2]
    check_against_scan_scene(L, clip_of(frames, width, height), sizes, 10, params)


def test_routing(L, param_dirs, monkeypatch):
    """the setter takes 2; the masks of forms 2, 1 and -1 (on both sides of its edge, which form 2 leaves alone); another network"""
    load(L, param_dirs["cifar10"])
    monkeypatch.delenv("BNN_MI355X_SCAN_MFMA_MIN", raising=False)
    L.bnn_mi355x_scan_form(0)
    assert L.bnn_mi355x_scan_form(2) == 0 and L.bnn_mi355x_scan_form(7) == 2 and L.bnn_mi355x_scan_form(3) == 2
    assert [L.bnn_mi355x_scan_matrix_stages(n) for n in (0, 1, 5386, 5387, 1 << 20)] == [MASK[2]] * 5
    assert L.bnn_mi355x_scan_form(1) == 2 and [L.bnn_mi355x_scan_matrix_stages(n) for n in (1, 1 << 20)] == [MASK[1]] * 2
    assert L.bnn_mi355x_scan_form(-1) == 1 and [L.bnn_mi355x_scan_matrix_stages(n) for n in (5386, 5387)] == [0, MASK[1]]
    A2 = gl.load("cnvW1A2")  # no clip scan there: nothing runs on the matrix cores whatever the form
    A2.load_parameters(gl.param_dir("cifar10", "cnvW1A2").encode())
    was = A2.bnn_mi355x_scan_form(2)
    assert A2.bnn_mi355x_scan_matrix_stages(4096) == 0 and A2.bnn_mi355x_scan_form(was) == 2
