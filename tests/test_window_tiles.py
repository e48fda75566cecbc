"""CPU: bnn_mi355x_tile_boxes is the tiling rule of CNV-BNN_Road-Signs.ipynb cell 13 ("Locate objects within a scene"),
including its asymmetry: `right <= width` but `lower < height`.  Host only, no GPU."""
import types

import numpy as np
import pytest

import gpu_lib as gl

SIZES = [4, 5, 31, 32, 33, 64, 96]


def notebook(width, height, size):
    """cell 13 for one window size, as the notebook writes it"""
    bounds = []
    stride = size // 4
    x_tiles = width // stride
    y_tiles = height // stride
    for j in range(y_tiles):
        for i in range(x_tiles):
            bound = (stride * i, stride * j, stride * i + size, stride * j + size)
            if bound[2] <= width and bound[3] < height:
                bounds.append(bound)
    return np.array(bounds, np.int32).reshape(-1, 4)


def notebook_vectorised(width, height, size):
    """the same loop over index grids (rows outer, columns inner): the stride-1 sizes would cost 10^8 interpreted
    iterations over the 130 x 130 pictures below; pinned against the loop itself in test_vectorised_form_is_the_loop"""
    stride = size // 4
    j, i = np.meshgrid(np.arange(height // stride), np.arange(width // stride), indexing="ij")
    b = np.stack([stride * i, stride * j, stride * i + size, stride * j + size], axis=-1).reshape(-1, 4)
    return b[(b[:, 2] <= width) & (b[:, 3] < height)].astype(np.int32)


@pytest.fixture(scope="module")
def lib():
    return gl.load("cnvW1A1")


def tiles(lib, width, height, size, buf):
    n = lib.bnn_mi355x_tile_boxes(width, height, size, buf.ctypes.data, len(buf))
    assert 0 <= n <= len(buf)
    return buf[:n]


def test_vectorised_form_is_the_loop():
    for size in SIZES:
        for w in list(range(1, 24)) + [64, 65, 96, 97, 130]:
            for h in list(range(1, 24)) + [64, 65, 96, 97, 130]:
                assert (notebook(w, h, size) == notebook_vectorised(w, h, size)).all(), (w, h, size)


def test_tile_boxes_equal_the_notebook(lib):
    buf = np.zeros((130 * 130, 4), np.int32)
    for size in SIZES:
        ref = notebook_vectorised if size // 4 == 1 else notebook
        for w in range(1, 131):
            for h in range(1, 131):
                got = tiles(lib, w, h, size, buf)
                want = ref(w, h, size)
                assert got.shape == want.shape and (got == want).all(), (w, h, size)
    # the strict `<` on the height, not on the width: a height that is a multiple of the stride loses its last row of
    # windows, a width that is one does not lose its last column
    assert tiles(lib, 64, 65, 64, buf).tolist() == [[0, 0, 64, 64]]
    assert tiles(lib, 64, 64, 64, buf).tolist() == []
    assert tiles(lib, 80, 81, 64, buf).tolist() == [[0, 0, 64, 64], [16, 0, 80, 64], [0, 16, 64, 80], [16, 16, 80, 80]]
    assert tiles(lib, 80, 80, 64, buf).tolist() == [[0, 0, 64, 64], [16, 0, 80, 64]]


def test_the_notebooks_scene_gives_1330_tiles(lib):
    buf = np.zeros((1000, 4), np.int32)
    counts = []
    for size in (64, 96):
        got = tiles(lib, 640, 480, size, buf)
        assert (got == notebook(640, 480, size)).all()
        counts.append(len(got))
    assert counts == [962, 368] and sum(counts) == 1330  # the number cell 13 prints


def test_cap_and_refusals(lib):
    buf = np.full((11, 4), -7, np.int32)
    assert lib.bnn_mi355x_tile_boxes(640, 480, 64, buf.ctypes.data, 10) == 962  # the count, whatever the room
    assert (buf[:10] == notebook(640, 480, 64)[:10]).all()
    assert (buf[10] == -7).all()  # no more than `cap` boxes written
    assert lib.bnn_mi355x_tile_boxes(640, 480, 64, None, 0) == 962
    assert lib.bnn_mi355x_tile_boxes(640, 480, 3, buf.ctypes.data, 10) == -1
    assert b"tile_boxes" in lib.bnn_mi355x_last_error()
    assert lib.bnn_mi355x_tile_boxes(640, 480, 0, None, 0) == -1
    assert lib.bnn_mi355x_tile_boxes(640, 480, -64, None, 0) == -1


def test_python_tile_boxes_is_size_major():
    """CnvClassifier.tile_boxes: the notebook's order, all windows of 64 and then all of 96 (no GPU: the method needs
    the library alone)"""
    import bnn
    clf = bnn.CnvClassifier.__new__(bnn.CnvClassifier)
    clf.bnn = types.SimpleNamespace(interface=gl.load("cnvW1A1"))
    got = clf.tile_boxes((640, 480))
    want = [tuple(b) for s in (64, 96) for b in notebook(640, 480, s).tolist()]
    assert got == want and len(got) == 1330
    assert clf.tile_boxes((200, 150), sizes=(33, 40)) == [tuple(b) for s in (33, 40) for b in notebook(200, 150, s).tolist()]
