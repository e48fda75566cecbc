"""CPU: what bnn_mi355x_windows_to_cifar and bnn_mi355x_classify_windows refuse, they refuse before anything touches a
GPU, with the offending box's index in last_error; an LFC library has no CIFAR records; no windows is no error."""
import ctypes as C

import numpy as np
import pytest

import gpu_lib as gl

W, H = 40, 30


@pytest.fixture(scope="module")
def lib():
    return gl.load("cnvW1A1")


def to_cifar(lib, boxes, scene=None, width=W, height=H, bands=3, stride=0, records=True):
    scene = np.zeros((H, W, 4), np.uint8) if scene is None else scene
    b = np.ascontiguousarray(np.asarray(boxes, np.int32).reshape(-1, 4))
    out = np.zeros((max(len(b), 1), 3073), np.uint8)
    rc = lib.bnn_mi355x_windows_to_cifar(scene.ctypes.data, width, height, bands, stride, b.ctypes.data, len(b),
                                         out.ctypes.data if records else None)
    return rc, lib.bnn_mi355x_last_error().decode()


def classify(lib, boxes, bands=3, stride=0, detail=0):
    scene = np.zeros((H, W, 4), np.uint8)
    b = np.ascontiguousarray(np.asarray(boxes, np.int32).reshape(-1, 4))
    usec, pre = C.c_float(-1), C.c_float(-1)
    p = lib.bnn_mi355x_classify_windows(scene.ctypes.data, W, H, bands, stride, b.ctypes.data, len(b), 10, C.byref(usec), C.byref(pre), detail)
    return p, lib.bnn_mi355x_last_error().decode()


GOOD = [0, 0, 40, 30]
BAD_BOXES = [
    ([5, 5, 5, 10], "empty"),      # right == left
    ([6, 5, 5, 10], "empty"),      # right < left
    ([5, 10, 9, 10], "empty"),     # lower == upper
    ([5, 11, 9, 10], "empty"),     # lower < upper
    ([-1, 0, 10, 10], "leaves"),   # off the left edge
    ([0, -1, 10, 10], "leaves"),   # off the upper edge
    ([31, 0, 41, 10], "leaves"),   # off the right edge
    ([0, 21, 10, 31], "leaves"),   # off the lower edge
]


@pytest.mark.parametrize("box,word", BAD_BOXES)
@pytest.mark.parametrize("position", [0, 2])
def test_bad_box_is_named(lib, box, word, position):
    boxes = [GOOD] * position + [box] + [GOOD]
    rc, err = to_cifar(lib, boxes)
    assert rc == -1 and "windows_to_cifar" in err and ("box %d " % position) in err and word in err, err
    p, err = classify(lib, boxes)
    assert not p and "classify_windows" in err and ("box %d " % position) in err and word in err, err


@pytest.mark.parametrize("bands", [0, 2, 5, -1])
def test_bad_bands(lib, bands):
    rc, err = to_cifar(lib, [GOOD], bands=bands)
    assert rc == -1 and "bands" in err
    p, err = classify(lib, [GOOD], bands=bands)
    assert not p and "bands" in err


def test_bad_row_stride(lib):
    rc, err = to_cifar(lib, [GOOD], stride=W * 3 - 1)
    assert rc == -1 and "row stride" in err
    rc, err = to_cifar(lib, [GOOD], stride=-5)
    assert rc == -1 and "row stride" in err
    p, err = classify(lib, [GOOD], bands=4, stride=W * 4 - 1)
    assert not p and "row stride" in err


def test_bad_picture_size(lib):
    for w, h in ((0, 30), (40, 0), (65536, 30), (-3, 30)):
        rc, err = to_cifar(lib, [[0, 0, 1, 1]], width=w, height=h)
        assert rc == -1 and "picture" in err


def test_null_pointers(lib):
    b = np.asarray([GOOD], np.int32)
    scene = np.zeros((H, W, 3), np.uint8)
    out = np.zeros((1, 3073), np.uint8)
    assert lib.bnn_mi355x_windows_to_cifar(None, W, H, 3, 0, b.ctypes.data, 1, out.ctypes.data) == -1
    assert b"null" in lib.bnn_mi355x_last_error()
    assert lib.bnn_mi355x_windows_to_cifar(scene.ctypes.data, W, H, 3, 0, None, 1, out.ctypes.data) == -1
    assert lib.bnn_mi355x_windows_to_cifar(scene.ctypes.data, W, H, 3, 0, b.ctypes.data, 1, None) == -1
    assert not lib.bnn_mi355x_classify_windows(None, W, H, 3, 0, b.ctypes.data, 1, 10, None, None, 0)
    assert b"null" in lib.bnn_mi355x_last_error()
    assert not lib.bnn_mi355x_classify_windows(scene.ctypes.data, W, H, 3, 0, None, 1, 10, None, None, 0)
    assert lib.bnn_mi355x_windows_to_cifar(scene.ctypes.data, W, H, 3, 0, b.ctypes.data, -1, out.ctypes.data) == -1
    assert not lib.bnn_mi355x_classify_windows(scene.ctypes.data, W, H, 3, 0, b.ctypes.data, 1, 0, None, None, 0)  # number_class
    assert not lib.bnn_mi355x_classify_windows(scene.ctypes.data, W, H, 3, 0, b.ctypes.data, 1, 65, None, None, 0)


def test_no_windows_is_no_error(lib):
    assert lib.bnn_mi355x_windows_to_cifar(None, 0, 0, 0, 0, None, 0, None) == 0
    usec, pre = C.c_float(-1), C.c_float(-1)
    for detail in (0, 1):
        p = lib.bnn_mi355x_classify_windows(None, 0, 0, 0, 0, None, 0, 10, C.byref(usec), C.byref(pre), detail)
        assert p
        lib.free_results(p)
        assert usec.value == 0 and pre.value == 0
    p = lib.bnn_mi355x_classify_windows(None, 0, 0, 0, 0, None, 0, 10, None, None, 0)  # (the times are optional)
    assert p
    lib.free_results(p)


def test_lfc_library_refuses():
    lfc = gl.load("lfcW1A1")
    rc, err = to_cifar(lfc, [GOOD])
    assert rc == -1 and "CNV" in err
    p, err = classify(lfc, [GOOD])
    assert not p and "CNV" in err
    assert lfc.bnn_mi355x_windows_to_cifar(None, 0, 0, 0, 0, None, 0, None) == -1  # as images_to_cifar: not even of nothing
    buf = np.zeros((4, 4), np.int32)
    assert lfc.bnn_mi355x_tile_boxes(80, 81, 64, buf.ctypes.data, 4) == -1
    assert b"CNV" in lfc.bnn_mi355x_last_error()
