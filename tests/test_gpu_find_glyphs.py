"""GPU: the glyphs of a picture -- connected components of its ink, labelled on the device (bnn_mi355x_find_glyphs,
bnn_mi355x_read_glyphs, LfcClassifier.find_glyphs / read_glyphs / read_text; csrc/component_kernels.hip).

Labelling has an exact answer: boxes, pixel counts, total and the WHOLE label map must be equal to the oracle
(tests/ccl_ref.py, plain numpy) and to the host statement of the model (bnn_mi355x_find_glyphs_host).  The pictures are L
arrays fed with the options {1, 1, -1}, where the enhancement is the identity, unless a test says otherwise.  lfcW1A1
with the mnist parameters throughout.  read_glyphs must equal classify_glyphs on find_glyphs' boxes, and the host route
classify_mnists on glyph_ref's records of those boxes.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import ccl_ref
import gpu_lib as gl
import glyph_ref

PIL = pytest.importorskip("PIL")
from PIL import Image, ImageDraw, ImageFont  # noqa: E402

sys.path.insert(0, os.path.join(gl.ROOT, "bnn-pynq_amd"))
from bnn import abi  # noqa: E402

pytestmark = pytest.mark.gpu
find_host, same = ccl_ref.find_host, ccl_ref.same

IDENTITY = (1.0, 1.0, -1)
MNIST = (3.0, 4.0, -1)
CHARS = (5.0, 2.0, 180)


@pytest.fixture(scope="module")
def clf():
    import bnn
    return bnn.LfcClassifier(bnn.NETWORK_LFCW1A1, "mnist", bnn.RUNTIME_SW)


def find_gpu(clf, a, ink_level=255, reach=(1, 1), min_pixels=1, order=0, cap=1 << 20, opts=IDENTITY, stride=0, width=None, want_labels=True):
    L = clf.bnn.interface
    h = a.shape[0]
    w = a.shape[1] if width is None else width
    bands = 1 if a.ndim == 2 else a.shape[2]
    n = min(cap, (w + 1) // 2 * ((h + 1) // 2))
    boxes = np.full((max(n, 1), 4), -7, np.int32)
    counts = np.full(max(n, 1), -7, np.int32)
    labels = np.full((h, w), -7, np.int32)
    o = abi.GlyphOpts(opts[0], opts[1], opts[2], 3, 0)
    f = abi.FindOpts(ink_level, reach[0], reach[1], min_pixels, order)
    total = L.bnn_mi355x_find_glyphs(a.ctypes.data, w, h, bands, stride, C.byref(o), C.byref(f), boxes.ctypes.data, counts.ctypes.data,
                                     labels.ctypes.data if want_labels else None, cap)
    assert total >= 0, L.bnn_mi355x_last_error().decode()
    k = min(total, cap)
    assert (boxes[k:] == -7).all() and (counts[k:] == -7).all()  # nothing is written past what is returned
    return boxes[:k], counts[:k], total, labels


# ---- every picture of ccl_ref.CASES: degenerate sizes, internal boundaries, long chains, late merges, nested rings,
#      noise on both sides of the percolation point, reach, filter / order / cap, ink_level -------------------------------
@pytest.mark.parametrize("i", range(len(ccl_ref.CASES)), ids=ccl_ref.CASE_IDS)
def test_gpu_equals_the_oracle_and_the_host(clf, i):
    name, picture, kw = ccl_ref.CASES[i]
    got = find_gpu(clf, picture, **kw)
    same(got, ccl_ref.expected(i), name)
    same(got, find_host(clf.bnn.interface, picture, **kw), name + " (host)")


@pytest.mark.parametrize("reach", [(1, 1), (2, 1), (1, 5), (16, 16)])
def test_pairs_join_exactly_within_reach(clf, reach):
    for name, picture, joined in ccl_ref.pair_pictures(reach):
        got = find_gpu(clf, picture, reach=reach)
        assert got[2] == (1 if joined else 2), (reach, name)
        same(got, find_host(clf.bnn.interface, picture, reach=reach), name)


def test_grid_beyond_the_cap(clf):
    """1 024 components, 10 returned: total says so, the first 10 in order, label -1 beyond"""
    boxes, counts, total, labels = find_gpu(clf, ccl_ref.grid(64), cap=10)
    assert total == 1024 and len(boxes) == 10 and (counts == 1).all()
    assert boxes.tolist() == [[2 * k, 0, 2 * k + 1, 1] for k in range(10)]
    assert labels[0, :20:2].tolist() == list(range(10)) and (labels[0, 20:] == -1).all() and (labels[1:] == -1).all()


def test_without_the_label_map(clf):
    picture = ccl_ref.noise(160, 200, 0.2, 1)
    got = find_gpu(clf, picture, want_labels=False)
    want = ccl_ref.expected(ccl_ref.CASE_IDS.index("noise 0.20 seed 1"))
    assert got[2] == want[2] and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and (got[3] == -7).all()


def test_twice_in_a_row(clf):
    """the arrival order of the atomics must not show"""
    picture = ccl_ref.noise(160, 200, 0.45, 1)
    first = find_gpu(clf, picture, order=1)
    second = find_gpu(clf, picture, order=1)
    same(second, first, "repeat")
    same(first, ccl_ref.label(picture, order=1), "repeat")


# ---- the real plane -------------------------------------------------------------------------------------------------
def sheet(text, lines=1):
    """examples/read_glyphs.py's sheet: dark print on a sheet that is not quite white"""
    img = Image.new("RGB", (40 + 50 * len(text), 100 * lines), (238, 236, 230))
    draw = ImageDraw.Draw(img)
    font = ImageFont.load_default(size=64)
    for j in range(lines):
        for i, ch in enumerate(text):
            draw.text((30 + 50 * i, 12 + 100 * j), ch if j == 0 else text[len(text) - 1 - i], font=font, fill=(25, 25, 40))
    return img


def column_split(plane):
    ink_columns = (plane != 255).any(axis=0)
    edges = np.flatnonzero(np.diff(np.concatenate([[0], ink_columns.astype(np.int8), [0]])))
    return [(int(a), int(b)) for a, b in zip(edges[::2], edges[1::2])]


def test_the_example_sheet(clf):
    img = sheet("3141592")
    a = np.asarray(img)
    plane = np.asarray(glyph_ref.enhance(img, *MNIST[:2])[0])
    got = find_gpu(clf, a, order=1, opts=MNIST)
    same(got, ccl_ref.label(plane, order=1), "sheet")
    assert got[2] == 7
    assert [(int(b[0]), int(b[2])) for b in got[0]] == column_split(plane)
    assert [(int(b[0]), int(b[2])) for b in got[0]] == [(33, 64), (88, 106), (132, 165), (188, 206), (233, 264), (283, 314), (334, 364)]
    # an RGBA view with a row stride: the same sheet inside a wider picture
    wide = np.zeros((a.shape[0], a.shape[1] + 9, 4), np.uint8)
    wide[:, 5:5 + a.shape[1], :3] = a
    wide[..., 3] = 77
    view = wide[:, 5:]
    L = clf.bnn.interface
    o, f = abi.GlyphOpts(*MNIST, 3, 0), abi.FindOpts(255, 1, 1, 1, 1)
    boxes = np.zeros((50, 4), np.int32); counts = np.zeros(50, np.int32); labels = np.zeros(a.shape[:2], np.int32)
    total = L.bnn_mi355x_find_glyphs(view.ctypes.data, a.shape[1], a.shape[0], 4, wide.strides[0], C.byref(o), C.byref(f), boxes.ctypes.data,
                                     counts.ctypes.data, labels.ctypes.data, 50)
    same((boxes[:total], counts[:total], total, labels), got, "RGBA view")


def test_dots_and_bars_join_with_the_reach(clf):
    img = sheet("i j = 5")
    plane = np.asarray(glyph_ref.enhance(img, CHARS[0], CHARS[1], CHARS[2])[0])
    for reach, n in (((1, 1), 7), ((1, 8), 5), ((1, 16), 4)):
        got = find_gpu(clf, np.asarray(img), reach=reach, order=1, opts=CHARS)
        assert got[2] == n, (reach, got[2])
        same(got, ccl_ref.label(plane, reach=reach, order=1), reach)


# ---- composition: read_glyphs = classify_glyphs on find_glyphs' boxes = the host route on those boxes -------------------
def read_gpu(clf, a, cap=64, reach=(1, 1), order=1, opts=MNIST):
    L = clf.bnn.interface
    bands = 1 if a.ndim == 2 else a.shape[2]
    o, f = abi.GlyphOpts(opts[0], opts[1], opts[2], 3, 0), abi.FindOpts(255, reach[0], reach[1], 1, order)
    boxes = np.full((cap, 4), -7, np.int32); status = np.full(cap, -7, np.int32)
    found, usec, pre = C.c_int(-1), C.c_float(-1), C.c_float(-1)
    p = L.bnn_mi355x_read_glyphs(a.ctypes.data, a.shape[1], a.shape[0], bands, 0, C.byref(o), C.byref(f), 10, cap, C.byref(found), boxes.ctypes.data,
                                 C.byref(usec), C.byref(pre), status.ctypes.data)
    assert p, L.bnn_mi355x_last_error().decode()
    k = min(found.value, cap)
    classes = np.ctypeslib.as_array(p, shape=(max(k, 1),))[:k].astype(np.int32, copy=True)
    L.free_results(p)
    assert (boxes[k:] == -7).all() and (status[k:] == -7).all()
    return classes, boxes[:k], status[:k], found.value, usec.value, pre.value


@pytest.mark.parametrize("text,lines", [("3141592", 1), ("27183", 2)])
def test_read_glyphs_is_find_then_classify(clf, tmp_path, text, lines):
    img = sheet(text, lines)
    a = np.asarray(img)
    order = 1 if lines == 1 else 0
    classes, boxes, status, found, usec, pre = read_gpu(clf, a, order=order)
    want_boxes = find_gpu(clf, a, order=order, opts=MNIST)[0]
    assert found == len(text) * lines == len(want_boxes) and np.array_equal(boxes, want_boxes)
    want = np.asarray(clf.classify_glyphs(img, boxes))
    assert np.array_equal(classes, want) and np.array_equal(status, clf.glyph_status)
    assert usec > 0 and pre > 0
    # the host route: Pillow's records of those boxes through classify_mnists
    recs, _, wstatus = glyph_ref.glyphs(img, boxes)
    path = str(tmp_path / "found-idx3-ubyte")
    with open(path, "wb") as fh:
        fh.write(glyph_ref.idx_file(recs))
    host = np.asarray(clf.classify_mnists(path))
    host[wstatus == 2] = -1
    assert np.array_equal(classes, host) and np.array_equal(status, wstatus)


def test_read_glyphs_beyond_the_cap_and_too_thin(clf):
    """a 1 x 60 stroke is a glyph of status 2 (class -1) like any caller's box; a cap below the total returns the first"""
    a = np.full((80, 120), 255, np.uint8)
    a[10:70, 5] = 0          # too thin
    a[20:50, 30:50] = 0      # a block
    a[20:24, 70:110] = 0     # a bar
    classes, boxes, status, found, _, _ = read_gpu(clf, a, opts=IDENTITY)
    assert found == 3 and boxes.tolist() == [[5, 10, 6, 70], [30, 20, 50, 50], [70, 20, 110, 24]]
    want = np.asarray(clf.classify_glyphs(a, boxes, contrast=1.0, brightness=1.0))
    assert np.array_equal(classes, want) and status.tolist() == [2, 0, 0] == clf.glyph_status.tolist() and classes[0] == -1
    classes2, boxes2, status2, found2, _, _ = read_gpu(clf, a, cap=2, opts=IDENTITY)
    assert found2 == 3 and np.array_equal(boxes2, boxes[:2]) and np.array_equal(classes2, classes[:2]) and np.array_equal(status2, status[:2])


def test_a_blank_sheet_reads_as_nothing(clf):
    a = np.full((60, 90, 3), 240, np.uint8)
    classes, boxes, status, found, usec, pre = read_gpu(clf, a)
    assert found == 0 and len(classes) == 0 and len(boxes) == 0 and usec == 0 and pre == 0
    assert clf.read_text(Image.fromarray(a)) == "" and clf.glyphs_found == 0


# ---- Python -------------------------------------------------------------------------------------------------------------
def test_python_entry_points(clf):
    img = sheet("3141592")
    plane = np.asarray(glyph_ref.enhance(img, *MNIST[:2])[0])
    want = ccl_ref.label(plane, order=1)
    boxes = clf.find_glyphs(img)
    assert boxes.dtype == np.int32 and np.array_equal(boxes, want[0]) and clf.glyphs_found == 7
    same(clf.find_glyphs(img, details=True), want, "details")
    same(clf.find_glyphs(img, details=True, order="raster", min_pixels=3, max_glyphs=4), ccl_ref.label(plane, order=0, min_pixels=3, cap=4), "knobs")
    classes, rboxes = clf.read_glyphs(img)
    assert np.array_equal(rboxes, boxes) and np.array_equal(classes, np.asarray(clf.classify_glyphs(img, boxes)))
    assert clf.glyphs_found == 7 and len(clf.glyph_status) == 7 and clf.usecPreprocess > 0 and clf.usecPerImage > 0
    assert clf.read_text(img) == "".join(clf.class_name(c) for c in classes)
    chars = sheet("i j = 5")
    assert [len(clf.find_glyphs(chars, preset="chars", reach=r)) for r in ((1, 1), (1, 8), (1, 16))] == [7, 5, 4]
    with pytest.raises(ValueError):
        clf.find_glyphs(img, order="up")
    with pytest.raises(RuntimeError, match="reach"):
        clf.find_glyphs(img, reach=(0, 1))
    assert clf.bnn.interface.bnn_mi355x_last_find_usec() > 0
