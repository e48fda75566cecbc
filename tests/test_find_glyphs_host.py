"""CPU: bnn_mi355x_find_glyphs_host -- the model's statement in csrc/components.cpp (two-pass union-find, then filter,
order and cap) -- against the separate oracle tests/ccl_ref.py on every picture the GPU tests use, and, where scipy is
there, against scipy.ndimage.label with the 3 x 3 structure at reach (1, 1).  Boxes, pixel counts, total and the whole
label map must be equal.  Also: what it refuses, NULL options, row strides."""
import ctypes as C

import numpy as np
import pytest

import ccl_ref
import gpu_lib as gl
from bnn import abi


@pytest.fixture(scope="module")
def lib():
    return gl.load("lfcW1A1")


find_host, same = ccl_ref.find_host, ccl_ref.same


@pytest.mark.parametrize("i", range(len(ccl_ref.CASES)), ids=ccl_ref.CASE_IDS)
def test_host_equals_the_oracle(lib, i):
    name, picture, kw = ccl_ref.CASES[i]
    same(find_host(lib, picture, **kw), ccl_ref.expected(i), name)


def test_the_shapes_are_what_they_are_meant_to_be():
    """one component for the chains, two for the combs that never touch, one per ring, a quarter of the pixels for the grid"""
    total = {name: ccl_ref.expected(i)[2] for i, (name, _, _) in enumerate(ccl_ref.CASES)}
    for name in ("all ink", "diagonal", "anti-diagonal", "cross", "spiral", "serpentine", "comb joined at the bottom", "comb joined at the top"):
        assert total[name] == 1, name
    assert total["two combs"] == 2 and total["rings"] == 34 and total["blank"] == 0
    assert total["grid 64 cap 10"] == 1024 and total["grid 128 cap 4096"] == 4096
    boxes = ccl_ref.expected(ccl_ref.CASE_IDS.index("two combs"))[0]
    assert boxes[0, 2] > boxes[1, 0] and boxes[0, 3] > boxes[1, 1]  # the two combs' boxes overlap
    assert (np.count_nonzero(ccl_ref.spiral(96) == 0)) > 4000  # a chain of thousands
    ring_boxes = ccl_ref.expected(ccl_ref.CASE_IDS.index("rings"))[0]
    assert (np.diff(ring_boxes[:, 0]) == 3).all() and (np.diff(ring_boxes[:, 2]) == -3).all()  # nested


@pytest.mark.parametrize("reach", [(1, 1), (2, 1), (1, 5), (16, 16)])
def test_pairs_join_exactly_within_reach(lib, reach):
    for name, picture, joined in ccl_ref.pair_pictures(reach):
        got = find_host(lib, picture, reach=reach)
        assert got[2] == (1 if joined else 2), (reach, name)
        same(got, ccl_ref.label(picture, reach=reach), name)


def test_against_scipy(lib):
    ndimage = pytest.importorskip("scipy.ndimage")
    for i, (name, picture, kw) in enumerate(ccl_ref.CASES):
        if kw:
            continue  # reach (1, 1), no filter, raster order: scipy numbers components in raster order of their first pixel
        lab, n = ndimage.label(picture < 255, structure=np.ones((3, 3)))
        boxes, counts, total, labels = find_host(lib, picture)
        assert total == n, name
        assert np.array_equal(labels, lab.astype(np.int32) - 1), name
        for k, sl in enumerate(ndimage.find_objects(lab)):
            assert boxes[k].tolist() == [sl[1].start, sl[0].start, sl[1].stop, sl[0].stop], (name, k)
        assert np.array_equal(counts, np.bincount(lab.reshape(-1))[1:]), name


def test_null_find_is_the_defaults(lib):
    picture = ccl_ref.noise(70, 50, 0.3, 11)
    picture[picture == 0] = 254  # ink at the default level only
    same(find_host(lib, picture, null_find=True), find_host(lib, picture), "NULL")
    same(find_host(lib, picture, null_find=True), ccl_ref.label(picture), "NULL")
    assert find_host(lib, picture, ink_level=254)[2] == 0


def test_optional_outputs(lib):
    picture = ccl_ref.noise(40, 30, 0.2, 12)
    want = find_host(lib, picture)
    got = find_host(lib, picture, want_labels=False, want_counts=False)
    assert got[2] == want[2] and np.array_equal(got[0], want[0]) and (got[1] == -7).all() and (got[3] == -7).all()


@pytest.mark.parametrize("reach", [(1, 1), (3, 2)])
def test_row_stride_views_equal_packed_copies(lib, reach):
    big = ccl_ref.noise(100, 60, 0.3, 13)
    view = big[:, 10:77]  # 67 columns of 100: the bytes past the view's width are ink and background of other columns
    packed = np.ascontiguousarray(view)
    f = abi.FindOpts(255, reach[0], reach[1], 1, 0)
    outs = []
    for data, stride in ((packed.ctypes.data, 0), (packed.ctypes.data, 67), (big.ctypes.data + 10, 100)):
        boxes = np.zeros((2000, 4), np.int32); counts = np.zeros(2000, np.int32); labels = np.zeros((60, 67), np.int32)
        total = lib.bnn_mi355x_find_glyphs_host(data, 67, 60, stride, C.byref(f), boxes.ctypes.data, counts.ctypes.data, labels.ctypes.data, 2000)
        outs.append((boxes[:total], counts[:total], total, labels))
    same(outs[1], outs[0], "stride = width")
    same(outs[2], outs[0], "view")
    same(outs[0], ccl_ref.label(packed, reach=reach), "packed")


REFUSALS = [
    (dict(ink_level=0), "ink_level"), (dict(ink_level=256), "ink_level"), (dict(reach=(0, 1)), "reach"), (dict(reach=(1, 0)), "reach"),
    (dict(reach=(17, 1)), "reach"), (dict(reach=(1, 17)), "reach"), (dict(min_pixels=0), "min_pixels"), (dict(order=2), "order"),
    (dict(order=-1), "order"), (dict(cap=0), "cap"), (dict(cap=-3), "cap"), (dict(width=0), "picture"), (dict(height=0), "picture"),
    (dict(width=65536), "picture"), (dict(width=4097, height=4096), "pixels"), (dict(stride=29), "row stride"), (dict(stride=-1), "row stride"),
    (dict(plane=False), "null"), (dict(boxes=False), "null"),
]


@pytest.mark.parametrize("kw,word", REFUSALS)
def test_refusals(lib, kw, word):
    picture = ccl_ref.blank(30, 20)
    boxes = np.zeros((200, 4), np.int32)
    f = abi.FindOpts(kw.get("ink_level", 255), *kw.get("reach", (1, 1)), kw.get("min_pixels", 1), kw.get("order", 0))
    rc = lib.bnn_mi355x_find_glyphs_host(picture.ctypes.data if kw.get("plane", True) else None, kw.get("width", 30), kw.get("height", 20),
                                         kw.get("stride", 0), C.byref(f), boxes.ctypes.data if kw.get("boxes", True) else None, None, None,
                                         kw.get("cap", 200))
    err = lib.bnn_mi355x_last_error().decode()
    assert rc == -1 and "find_glyphs_host" in err and word in err, err


def test_any_library_states_the_model():
    """host only: a CNV library answers too"""
    cnv = gl.load("cnvW1A1")
    same(find_host(cnv, ccl_ref.blobs()), ccl_ref.label(ccl_ref.blobs()), "cnv")
