"""CPU: the fine scan's host-only side (bnn_mi355x_scan_fine_boxes; csrc/scan_fine.cpp) against a few lines of numpy that
state the rule, and the refusals that must come before anything touches a GPU.  No test here touches one."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import gpu_lib as gl

sys.path.insert(0, os.path.join(gl.ROOT, "bnn-pynq_amd"))


@pytest.fixture(scope="module")
def L():
    return gl.load("cnvW1A1")


def fine_boxes(w, h, s):
    """the rule: level = (w * 32 // s, h * 32 // s); window (I, J) at level offset (2I, 2J) is (I s // 16, J s // 16, + s, + s);
    order: phase (py, then px), then raster"""
    lw, lh = w * 32 // s, h * 32 // s
    nx2, ny2 = (lw - 32) // 2 + 1, (lh - 32) // 2 + 1
    b = [(I * s // 16, J * s // 16, I * s // 16 + s, J * s // 16 + s)
         for py in (0, 1) for px in (0, 1) for J in range(py, ny2, 2) for I in range(px, nx2, 2)]
    return (lw, lh), np.asarray(b, np.int32).reshape(-1, 4)


def fine_call(L, w, h, sizes, frames=1):
    """bnn_mi355x_scan_clip_fine on a clip it must refuse before it reads a pixel"""
    sz, px, boxes = np.asarray(sizes, np.int32), np.zeros(16, np.uint8), np.zeros(4, np.int32)
    return L.bnn_mi355x_scan_clip_fine(px.ctypes.data, frames, 0, w, h, 3, 0, sz.ctypes.data, len(sz), 10, boxes.ctypes.data, None, None, 0)


@pytest.mark.parametrize("size", [32, 48, 72])
@pytest.mark.parametrize("w,h", [(150, 101), (151, 100), (75, 72)])
def test_boxes_state_the_rule(L, size, w, h):
    """widths and heights whose (side - 32) is even and odd; 75 x 72 at size 72 is one 33 x 32 level: one window, three empty phases"""
    (lw, lh), want = fine_boxes(w, h, size)
    glw, glh = C.c_int(-1), C.c_int(-1)
    n = L.bnn_mi355x_scan_fine_boxes(w, h, size, None, 0, C.byref(glw), C.byref(glh))
    assert (n, glw.value, glh.value) == (len(want), lw, lh) and n == ((lw - 32) // 2 + 1) * ((lh - 32) // 2 + 1)
    got = np.full((n, 4), -1, np.int32)
    assert L.bnn_mi355x_scan_fine_boxes(w, h, size, got.ctypes.data, n, None, None) == n
    assert (got == want).all()
    assert got[:, 2].max() <= w and got[:, 3].max() <= h
    # phase (0, 0) is the stride-4 scan
    coarse = np.full((n, 4), -1, np.int32)
    nc = L.bnn_mi355x_scan_boxes(w, h, size, coarse.ctypes.data, n, None, None)
    assert (got[:nc] == coarse[:nc]).all()
    # ... and the Python statement agrees
    import bnn
    (plw, plh), pb = bnn.CnvClassifier.scan_fine_boxes((w, h), size)
    assert (plw, plh) == (lw, lh) and (pb == want).all()


@pytest.mark.parametrize("w,h,size,words", [(31, 64, 32, "32 x 32 pixels or more"), (64, 64, 36, "not a multiple of 8"),
                                            (64, 64, 72, "leaves a level below 32 x 32")])
def test_refused_sides_and_sizes(L, w, h, size, words):
    assert L.bnn_mi355x_scan_fine_boxes(w, h, size, None, 0, None, None) == -1
    assert words in L.bnn_mi355x_last_error().decode()
    assert not fine_call(L, w, h, (size,)) and words in L.bnn_mi355x_last_error().decode()


@pytest.mark.parametrize("net", ["cnvW1A2", "cnvW2A2", "lfcW1A1", "lfcW1A2"])
def test_refused_on_other_libraries(net):
    lib = gl.load(net)
    words = "built for cnvW1A1 only" if net.startswith("cnv") else "CNV networks only"
    assert lib.bnn_mi355x_scan_fine_boxes(64, 64, 32, None, 0, None, None) == -1 and words in lib.bnn_mi355x_last_error().decode()
    assert not fine_call(lib, 64, 64, (32,)) and words in lib.bnn_mi355x_last_error().decode()
    out = np.zeros(16, np.uint8)
    sz = np.asarray([32], np.int32)
    assert lib.bnn_mi355x_debug_scan_clip_fine_stage(out.ctypes.data, 1, 0, 64, 64, 3, 0, sz.ctypes.data, 1, 2, 0, out.ctypes.data, 16) == -1
    assert words in lib.bnn_mi355x_last_error().decode()


def test_refused_over_the_window_limit_once_phases_are_counted(L):
    """1280 x 720 at size 32: 313 x 173 = 54 149 windows a frame at stride 4 and 625 x 345 = 215 625 at stride 2.  Five frames
    stay far below 2^20 windows at stride 4 (scan_clip takes them) and pass it at stride 2: refused, with the count"""
    sz = np.asarray([32], np.int32)
    assert 5 * 54149 < (1 << 20) < 5 * 215625
    assert L.bnn_mi355x_scan_clip_capacity(1280, 720, sz.ctypes.data, 1) >= 5
    assert not fine_call(L, 1280, 720, (32,), frames=5)
    assert "has %d windows at stride 2, more than the limit of %d" % (5 * 215625, 1 << 20) in L.bnn_mi355x_last_error().decode()
