"""GPU: the matrix-core form of the clip scan's stages 1-3 (bnn_mi355x_scan_form, k_clip_conv_mfma; DESIGN.md 9 "Clip
scan") against the shipped integer kernels, byte for byte, and the routing.  A block owns a band of kClipMfmaRowPairs = 8
output row pairs x kClipMfmaChunk = 64 conv-output columns.  With ny window rows the layers have 14 + 2 (ny - 1), 6 + (ny - 1)
and 5 + (ny - 1) row pairs: heights 32 .. 48 (ny = 1 .. 5) give layer 2 seven, eight and nine at ny = 2, 3, 4, layer 3 at
ny = 3, 4, 5, and layer 1, whose count is even, 14, 16 and 18 around its two bands.  The widths put each layer under, at and
over one 32-column tile; 72 and 100 put a chunk boundary into layer 1's rows (68, 96 columns), 140 into layer 2's (66)."""
import os

import numpy as np
import pytest

import gpu_lib as gl
import scan_clip_ref as ref
from test_gpu_scan_clip import check_against_scan_scene

pytestmark = pytest.mark.gpu

# (BNN_MI355X_CONV=valu: no operand tables, the integer kernels run under every form and only the routing is checked)
ALL = 0b1110 if os.environ.get("BNN_MI355X_CONV") != "valu" else 0
SHAPES = [(w, (32, 36, 40, 44, 48), 1, (32,)) for w in (32, 36, 40, 72, 76, 100)] + [(140, (32, 44), 1, (32,)), (100, (52,), 3, (32, 40))]


@pytest.fixture(scope="module")
def param_dirs(tmp_path_factory):
    import random_params
    d = tmp_path_factory.mktemp("rp_scan_matrix")
    random_params.make(str(d), "cnvW1A1", 733)
    return {"cifar10": gl.param_dir("cifar10", "cnvW1A1"), "random": str(d)}


@pytest.fixture(scope="module")
def L():
    lib = gl.load("cnvW1A1")
    was = lib.bnn_mi355x_scan_form(7)
    yield lib
    lib.bnn_mi355x_scan_form(was)
    lib.load_parameters(gl.param_dir("cifar10", "cnvW1A1").encode())  # leave the library as found


def load(L, pdir):
    L.load_parameters(pdir.encode())
    assert L.bnn_mi355x_last_error() == b"", L.bnn_mi355x_last_error()


def clip_of(frames, w, h):  # seeded random RGB frames, every frame different
    return np.random.default_rng(100000 * frames + 1000 * w + h).integers(0, 256, (frames, h, w, 3), dtype=np.uint8)


def stage_region(L, clip, sizes, stage, form, fill=None):
    """the stage's region under `form`.  The map buffers are never cleared.  fill = (other, own) parameter directories: the
    region is first filled with the integer kernels' maps under the OTHER set, so that a store the run under test skips shows"""
    frames, h, w = clip.shape[:3]
    sz = np.asarray(sizes, np.int32)
    out = [np.zeros(ref.layout(w, h, sizes, frames)["stage_bytes"][stage], np.uint8) for _ in range(2)]
    for o, f, pdir in ((out[0], 0, fill[0]), (out[1], form, fill[1])) if fill else ((out[1], form, None),):
        if pdir:
            load(L, pdir)
        L.bnn_mi355x_scan_form(f)
        assert f < 0 or L.bnn_mi355x_scan_matrix_stages(1) == (ALL if f else 0)
        assert L.bnn_mi355x_debug_scan_clip_stage(clip.ctypes.data, frames, 0, w, h, 3, 0, sz.ctypes.data, len(sz), stage, o.ctypes.data,
                                                  o.nbytes) == o.nbytes, L.bnn_mi355x_last_error()
    assert not fill or (out[0].view(np.uint32) != out[1].view(np.uint32)).mean() > 0.5  # (most dwords of the fill are foreign)
    return out[1]


@pytest.mark.parametrize("params", ["cifar10", "random"])
@pytest.mark.parametrize("width,heights,frames,sizes", SHAPES)  # (the picture's width, its heights, frames, window sizes)
def test_stage_maps_equal_the_integer_kernels(L, param_dirs, params, width, heights, frames, sizes):
    """stages 1, 2, 3: the whole region of debug_scan_clip_stage under form 1, over a foreign fill, equals the one under form 0"""
    fill = (param_dirs["random" if params == "cifar10" else "cifar10"], param_dirs[params])
    load(L, param_dirs[params])
    for h in heights:
        clip = clip_of(frames, width, h)
        for stage in (1, 2, 3):
            want, got = stage_region(L, clip, sizes, stage, 0), stage_region(L, clip, sizes, stage, 1, fill)
            assert (want == got).all(), (params, width, h, "stage", stage, "bytes differing", int((want != got).sum()))


@pytest.mark.parametrize("params", ["cifar10", "random"])
@pytest.mark.parametrize("width,height,frames,sizes", [(100, 52, 3, (32, 40)), (76, 44, 1, (32,))])
def test_scores_equal_scan_scene(L, param_dirs, params, width, height, frames, sizes):
    """all 64 raw scores and the classes of every window under form 1 against bnn_mi355x_scan_scene on each frame"""
    load(L, param_dirs[params])
    L.bnn_mi355x_scan_form(1)
    assert L.bnn_mi355x_scan_matrix_stages(1) == ALL
    check_against_scan_scene(L, clip_of(frames, width, height), sizes, 10, params)


def test_routing(L, param_dirs, monkeypatch):
    """the setter, the mask under the three forms, the automatic form's edge, another network, and a second parameter set"""
    load(L, param_dirs["cifar10"])
    monkeypatch.delenv("BNN_MI355X_SCAN_MFMA_MIN", raising=False)
    L.bnn_mi355x_scan_form(0)
    assert L.bnn_mi355x_scan_form(1) == 0 and L.bnn_mi355x_scan_form(7) == 1 and L.bnn_mi355x_scan_form(-2) == 1
    assert [L.bnn_mi355x_scan_matrix_stages(n) for n in (0, 1, 1 << 20)] == [ALL] * 3
    assert L.bnn_mi355x_scan_form(0) == 1 and [L.bnn_mi355x_scan_matrix_stages(n) for n in (1, 1 << 20)] == [0, 0]
    assert L.bnn_mi355x_scan_form(-1) == 0 and [L.bnn_mi355x_scan_matrix_stages(n) for n in (5386, 5387)] == [0, ALL]  # the built-in edge
    monkeypatch.setenv("BNN_MI355X_SCAN_MFMA_MIN", "300")
    assert [L.bnn_mi355x_scan_matrix_stages(n) for n in (1, 299, 300, 1 << 20)] == [0, 0, ALL, ALL]
    clip, small = clip_of(3, 100, 52), clip_of(2, 44, 40)  # (3 x 147 windows: the matrix form under automatic from that edge on)
    want = stage_region(L, clip, (32, 40), 3, 0)
    assert (stage_region(L, clip, (32, 40), 3, -1, (param_dirs["random"], param_dirs["cifar10"])) == want).all()
    load(L, param_dirs["random"])  # the operand tables are remade
    for stage in (1, 2, 3):
        want = stage_region(L, small, (32,), stage, 0)
        assert (stage_region(L, small, (32,), stage, 1, (param_dirs["cifar10"], param_dirs["random"])) == want).all(), stage
    A2 = gl.load("cnvW1A2")  # no clip scan there: nothing runs on the matrix cores whatever the form
    A2.load_parameters(gl.param_dir("cifar10", "cnvW1A2").encode())
    was = A2.bnn_mi355x_scan_form(1)
    assert A2.bnn_mi355x_scan_matrix_stages(4096) == 0 and A2.bnn_mi355x_scan_form(was) == 1
