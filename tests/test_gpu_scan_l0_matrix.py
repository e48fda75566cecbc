"""GPU: the matrix-core form of the clip scan's stage 0 (bnn_mi355x_scan_stage0_form, k_clip_conv0_mfma; DESIGN.md 9 "Clip
scan") against the integer kernel k_clip_conv0, byte for byte, and the routing.  A block owns a band of kClipL0Rows = 16
output rows x kClipL0Cols = 128 output columns, a tile is 32 pixels of one row, a level's stage-0 map is its used width - 2
wide.  The shapes are the smallest at which the kernel can go wrong, derived from those constants:
  alignment   widths 44 .. 47 at height 37, two frames: row strides 0 .. 3 mod 4, odd plane sizes: every byte phase
  tile edge   widths 36, 64, 68: maps 30, 62, 66 wide -- under one tile, under two, two tiles and two pixels
  band edges  200 x 52: a map of 198 x 50, chunks 128 + 70, row bands 16 + 16 + 16 + 2; 164 x 50: a last chunk of 34 columns
  several     90 x 74, three frames, sizes (32, 64): a resized level of 45 x 37 beside the frames' own, one launch
  quantiser   100 x 52 of the bytes 0, 1, 127, 128, 254, 255 alone"""
import os
import shutil

import numpy as np
import pytest

import gpu_lib as gl
import scan_clip_ref as ref
from test_gpu_scan_clip import check_against_scan_scene
from test_gpu_scan_matrix import clip_of, load, param_dirs  # noqa: F401  (param_dirs: the fixture)

pytestmark = pytest.mark.gpu

BIT0 = 1 if os.environ.get("BNN_MI355X_L0") != "valu" else 0  # (valu: no layer-0 table, only the routing is checked)
REST = 0b111110 if os.environ.get("BNN_MI355X_CONV") != "valu" else 0  # scan_form 2's stages
SHAPES = ([(w, 37, 2, (32,), False) for w in (44, 45, 46, 47)] + [(w, 36, 1, (32,), False) for w in (36, 64, 68)] +
          [(200, 52, 1, (32,), False), (164, 50, 1, (32,), False), (90, 74, 3, (32, 64), False), (100, 52, 1, (32,), True)])


@pytest.fixture(scope="module")
def L():
    lib = gl.load("cnvW1A1")
    was, was0 = lib.bnn_mi355x_scan_form(7), lib.bnn_mi355x_scan_stage0_form(7)
    yield lib
    lib.bnn_mi355x_scan_form(was)
    lib.bnn_mi355x_scan_stage0_form(was0)
    lib.load_parameters(gl.param_dir("cifar10", "cnvW1A1").encode())  # leave the library as found


def stage0_region(L, clip, sizes, form, fill=None):
    """stage 0's region under stage-0 form `form`, over the integer kernel's maps under fill[0] (test_gpu_scan_matrix.stage_region)"""
    frames, h, w = clip.shape[:3]
    sz = np.asarray(sizes, np.int32)
    out = [np.zeros(ref.layout(w, h, sizes, frames)["stage_bytes"][0], np.uint8) for _ in range(2)]
    for o, f, pdir in ((out[0], 0, fill[0]), (out[1], form, fill[1])) if fill else ((out[1], form, None),):
        if pdir:
            load(L, pdir)
        L.bnn_mi355x_scan_stage0_form(f)
        assert L.bnn_mi355x_scan_matrix_stages(1) & 1 == (BIT0 if f else 0)
        assert L.bnn_mi355x_debug_scan_clip_stage(clip.ctypes.data, frames, 0, w, h, 3, 0, sz.ctypes.data, len(sz), 0, o.ctypes.data,
                                                  o.nbytes) == o.nbytes, L.bnn_mi355x_last_error()
    assert not fill or (out[0].view(np.uint32) != out[1].view(np.uint32)).mean() > 0.5  # (most dwords of the fill are foreign)
    return out[1]


@pytest.mark.parametrize("params", ["cifar10", "random"])
@pytest.mark.parametrize("width,height,frames,sizes,edges", SHAPES)
def test_stage0_maps_equal_the_integer_kernel(L, param_dirs, params, width, height, frames, sizes, edges):
    """the whole stage-0 region of debug_scan_clip_stage under form 1, over a foreign fill, equals the one under form 0"""
    fill = (param_dirs["random" if params == "cifar10" else "cifar10"], param_dirs[params])
    load(L, param_dirs[params])
    clip = clip_of(frames, width, height)
    if edges:  # the bytes around the quantiser's steps
        clip = np.array([0, 1, 127, 128, 254, 255], np.uint8)[clip % 6]
    want, got = stage0_region(L, clip, sizes, 0), stage0_region(L, clip, sizes, 1, fill)
    assert (want == got).all(), (params, width, height, "bytes differing", int((want != got).sum()))


@pytest.mark.parametrize("params", ["cifar10", "random"])
@pytest.mark.parametrize("form", [0, 2])
def test_scores_equal_scan_scene(L, param_dirs, params, form):
    """all 64 raw scores and the classes of every window under stage-0 form 1 against bnn_mi355x_scan_scene on each frame"""
    load(L, param_dirs[params])
    L.bnn_mi355x_scan_form(form)
    L.bnn_mi355x_scan_stage0_form(1)
    assert L.bnn_mi355x_scan_matrix_stages(1) == (REST if form else 0) | BIT0
    check_against_scan_scene(L, clip_of(3, 100, 52), (32, 40), 10, params)


def test_routing(L, param_dirs, tmp_path):
    """the setter, bit 0 of the mask, a library with nothing loaded, another network, and a second parameter set"""
    load(L, param_dirs["cifar10"])
    L.bnn_mi355x_scan_form(0)
    L.bnn_mi355x_scan_stage0_form(0)
    assert L.bnn_mi355x_scan_stage0_form(1) == 0 and L.bnn_mi355x_scan_stage0_form(7) == 1 and L.bnn_mi355x_scan_stage0_form(-1) == 1
    assert L.bnn_mi355x_scan_stage0_form(2) == 1 and [L.bnn_mi355x_scan_matrix_stages(n) for n in (0, 1, 1 << 20)] == [BIT0] * 3
    L.bnn_mi355x_scan_form(2)
    assert L.bnn_mi355x_scan_matrix_stages(1) == REST | BIT0 and L.bnn_mi355x_scan_stage0_form(0) == 1
    assert L.bnn_mi355x_scan_matrix_stages(1) == REST and L.bnn_mi355x_scan_form(0) == 2 and L.bnn_mi355x_scan_matrix_stages(1) == 0
    small = clip_of(2, 45, 37)
    load(L, param_dirs["random"])  # the kernel reads the table of the parameters now loaded
    want = stage0_region(L, small, (32,), 0)
    assert (stage0_region(L, small, (32,), 1, (param_dirs["cifar10"], param_dirs["random"])) == want).all()
    fresh = gl.abi.load_path(shutil.copy(gl.lib_path("cnvW1A1"), str(tmp_path / "fresh.so")))  # its own state: nothing loaded
    assert fresh.bnn_mi355x_scan_stage0_form(1) == (1 if os.environ.get("BNN_MI355X_SCAN_L0") == "mfma" else 0)
    assert fresh.bnn_mi355x_scan_stage0_form(7) == 1 and fresh.bnn_mi355x_scan_matrix_stages(4096) == 0
    A2 = gl.load("cnvW1A2")  # no clip scan there: nothing runs on the matrix cores whatever the form
    A2.load_parameters(gl.param_dir("cifar10", "cnvW1A2").encode())
    was = A2.bnn_mi355x_scan_stage0_form(1)
    assert A2.bnn_mi355x_scan_matrix_stages(4096) == 0 and A2.bnn_mi355x_scan_stage0_form(was) == 1
