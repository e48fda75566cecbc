"""GPU: every window of one scene in one call (bnn_mi355x_windows_to_cifar, bnn_mi355x_classify_windows,
CnvClassifier.classify_windows / locate; CNV-BNN_Road-Signs.ipynb cells 13-16).

The reference for records is Pillow itself: record i must equal, on all 3073 bytes, what the reference's procedure writes
for scene.crop(boxes[i]).  The reference for classes and scores is this runtime's own classification of those records
(bnn_mi355x_inference_buffer / bnn_mi355x_inference_raw), and classify_images on the crops.  The notebook pins no tile
(it holds pictures only): parity with it is the count of 1 330 windows (tests/test_window_tiles.py) and nothing more.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import gpu_lib as gl

PIL = pytest.importorskip("PIL")
from PIL import Image  # noqa: E402

sys.path.insert(0, os.path.join(gl.ROOT, "bnn-pynq_amd"))

pytestmark = pytest.mark.gpu

STREET = os.path.join(gl.ROOT, "tests", "golden", "street_with_stop.jpg")
STOP = 14  # the class cell 14 of the notebook outlines


def pil_record(img):
    """the reference's procedure, on the host (bnn.py:226-242; as in tests/test_image_to_cifar.py)"""
    img = img.copy()
    img.thumbnail((32, 32), Image.LANCZOS, reducing_gap=None)
    canvas = Image.new("RGBA", (32, 32), (255, 255, 255, 0))
    canvas.paste(img, (int((32 - img.size[0]) / 2), int((32 - img.size[1]) / 2)))
    px = np.array(canvas)
    return np.concatenate([np.array([1], np.uint8)] + [px[:, :, c].flatten() for c in range(3)])


def picture(w, h, mode, seed, kind):
    """as in tests/test_image_to_cifar.py"""
    rng = np.random.default_rng(seed)
    shape = (h, w) if mode == "L" else (h, w, 3)
    if kind == "noise":
        a = rng.integers(0, 256, shape, dtype=np.uint8)
    elif kind == "blocks":  # saturated blocks: the Lanczos lobes overshoot, clip8 works at both ends
        by, bx = max(h // 7, 1), max(w // 5, 1)
        yy, xx = np.mgrid[0:h, 0:w]
        base = (((yy // by) + (xx // bx)) % 2 * 255).astype(np.uint8)
        a = base if mode == "L" else np.stack([base, 255 - base, np.roll(base, bx // 2 + 1, axis=1)], axis=2)
    else:  # smooth gradient + a little noise
        yy, xx = np.mgrid[0:h, 0:w]
        g = (yy * 255.0 / max(h - 1, 1) * 0.5 + xx * 255.0 / max(w - 1, 1) * 0.5)
        a = np.clip(g + rng.normal(0, 3, (h, w)), 0, 255).astype(np.uint8)
        if mode != "L":
            a = np.stack([a, a[::-1], a[:, ::-1]], axis=2)
    if mode == "RGBA":  # colour planes as for RGB, alpha: every regime of the premultiply / unpremultiply pair
        alpha = rng.choice(np.array([0, 1, 2, 17, 128, 200, 254, 255], np.uint8), size=(h, w), p=[.15, .05, .05, .1, .15, .15, .1, .25])
        if kind == "smooth":
            alpha = np.clip(np.mgrid[0:h, 0:w][1] * 255.0 / max(w - 1, 1) + rng.normal(0, 2, (h, w)), 0, 255).astype(np.uint8)
        a = np.dstack([a, alpha])
    return Image.fromarray(np.ascontiguousarray(a), mode)


def notebook_tiles(width, height, sizes):
    """cell 13"""
    bounds = []
    for s in sizes:
        stride = s // 4
        for j in range(height // stride):
            for i in range(width // stride):
                bound = (stride * i, stride * j, stride * i + s, stride * j + s)
                if bound[2] <= width and bound[3] < height:
                    bounds.append(bound)
    return bounds


def same_records(got, scene, boxes):
    assert got.shape == (len(boxes), 3073)
    for r, b in zip(got, boxes):
        want = pil_record(scene.crop(tuple(b)))
        assert (r == want).all(), ("box", tuple(b), "first differing byte", int(np.argmax(r != want)))


@pytest.fixture(scope="module")
def clf():
    import bnn
    return bnn.CnvClassifier(bnn.NETWORK_CNVW1A1, "road-signs", bnn.RUNTIME_SW)


SMALL = (200, 150)
HAND_PICKED = [
    (0, 0, 32, 32), (0, 0, 31, 32), (13, 12, 18, 19),   # pasted unresampled, at offsets 0, 0 and (13, 12)
    (7, 9, 47, 29), (100, 50, 120, 90),                  # 40 x 20 and 20 x 40: not square, pasted off-centre
    (55, 3, 56, 67),                                     # 1 x 64: no horizontal pass
    (0, 0, 200, 150),                                    # the whole scene
    (0, 40, 64, 104), (50, 0, 114, 64), (136, 20, 200, 84), (30, 86, 94, 150),  # on each edge; the last one: lower == height
    (199, 149, 200, 150), (0, 149, 200, 150), (199, 0, 200, 150),                # the last pixel, the last row, the last column
    (16, 16, 80, 80), (16, 16, 80, 80),                  # twice the same box
]


def small_boxes():
    tiles = notebook_tiles(SMALL[0], SMALL[1], (33, 40, 64, 96))
    assert len(tiles) == 571
    boxes = tiles + HAND_PICKED
    order = np.random.default_rng(12).permutation(len(boxes))
    return [boxes[i] for i in order]


@pytest.mark.parametrize("mode,kind", [("RGB", "noise"), ("L", "blocks"), ("RGBA", "noise"), ("RGBA", "smooth"), ("RGB", "blocks")])
def test_records_equal_pillow(clf, mode, kind):
    scene = picture(SMALL[0], SMALL[1], mode, 3 + len(kind), kind)
    before = scene.tobytes()
    boxes = small_boxes()
    got = clf.windows_to_cifar(scene, boxes)
    assert scene.tobytes() == before and scene.size == SMALL  # the caller's image is left as it is
    same_records(got, scene, boxes)
    assert (clf.windows_to_cifar(np.asarray(scene), boxes) == got).all()  # a decoded picture takes the same route


@pytest.mark.parametrize("mode", ["RGB", "RGBA"])
def test_fallback_routes_equal_pillow(clf, mode):
    """windows Pillow resamples vertical pass first, and windows on both sides of the LDS budget (height x out_w x bands
    <= 32768: RGB 341 / 342 rows of 32 x 3 bytes, RGBA 256 / 257 rows of 32 x 4), next to windows of the fused route"""
    scene = picture(345, 701, mode, 21, "noise")
    boxes = [(0, 0, 2, 201), (1, 0, 8, 701), (343, 500, 345, 701), (0, 0, 2, 200),
             (0, 0, 341, 341), (2, 100, 344, 442), (3, 359, 345, 701),
             (0, 0, 256, 256), (5, 7, 262, 264), (88, 444, 345, 701),
             (10, 10, 74, 74), (0, 0, 345, 701), (100, 100, 132, 132)]
    same_records(clf.windows_to_cifar(scene, boxes), scene, boxes)


def test_row_stride(clf):
    """the scene as a view into a larger array (C ABI, rows 1500 bytes apart) == its packed copy"""
    L = clf.bnn.interface
    big = np.random.default_rng(3).integers(0, 256, (300, 500, 3), dtype=np.uint8)
    view = big[10:210, 50:350]  # 200 rows of 300 pixels
    packed = np.ascontiguousarray(view)
    boxes = notebook_tiles(300, 200, (64, 96)) + [(0, 0, 300, 200), (299, 199, 300, 200), (0, 0, 20, 20), (236, 136, 300, 200)]
    b = np.asarray(boxes, np.int32)
    out_view = np.zeros((len(b), 3073), np.uint8)
    out_packed = np.zeros((len(b), 3073), np.uint8)
    assert L.bnn_mi355x_windows_to_cifar(view.ctypes.data, 300, 200, 3, 1500, b.ctypes.data, len(b), out_view.ctypes.data) == 0
    assert L.bnn_mi355x_windows_to_cifar(packed.ctypes.data, 300, 200, 3, 0, b.ctypes.data, len(b), out_packed.ctypes.data) == 0
    assert (out_view == out_packed).all()
    out_exact = np.zeros((len(b), 3073), np.uint8)
    assert L.bnn_mi355x_windows_to_cifar(packed.ctypes.data, 300, 200, 3, 900, b.ctypes.data, len(b), out_exact.ctypes.data) == 0
    assert (out_exact == out_packed).all()
    same_records(out_packed, Image.fromarray(packed, "RGB"), boxes)


@pytest.fixture(scope="module")
def street():
    return Image.open(STREET).convert("RGB")


@pytest.fixture(scope="module")
def street_reference(clf, street):
    """the parent's route on the notebook's 1 330 crops, once: classes and scores of classify_images(_details)"""
    assert street.size == (640, 480)
    boxes = notebook_tiles(640, 480, (64, 96))
    assert len(boxes) == 1330
    crops = [street.crop(b) for b in boxes]
    classes = np.asarray(clf.classify_images(crops))
    details = np.asarray(clf.classify_images_details(crops)).reshape(len(boxes), len(clf.classes))
    return boxes, classes, details


def raw_reference(clf, records):
    """this runtime's classification of the records' bodies: classes (inference_buffer) and scores (inference_raw)"""
    L = clf.bnn.interface
    ncls = len(clf.classes)
    bodies = np.ascontiguousarray(records[:, 1:])
    n = len(bodies)
    p = L.bnn_mi355x_inference_buffer(bodies.ctypes.data, n, ncls, None, 0)
    assert p
    classes = np.ctypeslib.as_array(p, shape=(n,)).astype(np.int32, copy=True)
    L.free_results(p)
    scores = np.zeros((n, 64), np.int16)
    assert L.bnn_mi355x_inference_raw(bodies.ctypes.data, n, scores.ctypes.data, None, None) == 0
    return classes, scores[:, :ncls].astype(np.int32)


@pytest.mark.parametrize("n", [1, 33, 571, 1330])
def test_classify_windows(clf, street, street_reference, n):
    """n crosses the direct path of the host entry points (n <= 32), the integer-pipe pass and the matrix-core pass"""
    L = clf.bnn.interface
    ncls = len(clf.classes)
    if n == 1330:
        scene, boxes = street, street_reference[0]
        assert L.bnn_mi355x_matrix_stages(1330) > 0  # the pass classify_windows enqueues for them runs on the matrix cores
    else:
        scene = picture(SMALL[0], SMALL[1], "RGB", 40, "smooth")
        boxes = small_boxes()[:n] if n < 571 else notebook_tiles(SMALL[0], SMALL[1], (33, 40, 64, 96))
    assert len(boxes) == n
    records = clf.windows_to_cifar(scene, boxes)
    if n == 1330:
        same_records(records, scene, boxes)
    want_classes, want_scores = raw_reference(clf, records)
    got = np.asarray(clf.classify_windows(scene, boxes))
    assert got.shape == (n,) and (got == want_classes).all()
    assert clf.usecPerImage > 0 and clf.usecPreprocess > 0
    details = np.asarray(clf.classify_windows_details(scene, boxes)).reshape(n, ncls)
    assert (details == want_scores).all()
    if n == 1330:
        _, ref_classes, ref_details = street_reference
    else:
        crops = [scene.crop(b) for b in boxes]
        ref_classes = np.asarray(clf.classify_images(crops))
        ref_details = np.asarray(clf.classify_images_details(crops)).reshape(n, ncls)
    assert (got == ref_classes).all() and (details == ref_details).all()
    # the C ABI itself, without the optional preprocess time
    b = np.asarray(boxes, np.int32)
    a = np.ascontiguousarray(np.asarray(scene))
    usec = C.c_float(0)
    p = L.bnn_mi355x_classify_windows(a.ctypes.data, a.shape[1], a.shape[0], 3, 0, b.ctypes.data, n, ncls, C.byref(usec), None, 0)
    assert p and usec.value > 0
    assert (np.ctypeslib.as_array(p, shape=(n,)) == want_classes).all()
    L.free_results(p)


def test_locate(clf, street, street_reference):
    boxes, classes, details = street_reference
    assert clf.tile_boxes(street.size) == boxes
    want = [b for b, c in zip(boxes, classes) if c == STOP]
    assert clf.locate(street, STOP) == want
    want_scored = [b for b, d in zip(boxes, details) if d[STOP] > 455]
    assert clf.locate(street, STOP, min_score=455) == want_scored
    assert clf.locate(np.asarray(street), STOP, sizes=(96,)) == [b for b in want if b[2] - b[0] == 96]
    print("class %d (%s): %d of %d windows; score > 455: %d" % (STOP, clf.classes[STOP], len(want), len(boxes), len(want_scored)))


def test_other_modes_take_the_host_route(clf):
    """palette and LA scenes: classify_images on the crops, as the docstring says"""
    scene = picture(120, 90, "RGB", 8, "smooth").convert("P")
    boxes = notebook_tiles(120, 90, (40,))[:6] + [(0, 0, 120, 90)]
    recs = clf.windows_to_cifar(scene, boxes)
    same_records(recs, scene, boxes)
    assert list(clf.classify_windows(scene, boxes)) == list(clf.classify_images([scene.crop(b) for b in boxes]))
    assert clf.windows_to_cifar(picture(50, 50, "RGB", 1, "noise"), []).shape == (0, 3073)
    assert len(clf.classify_windows(picture(50, 50, "RGB", 1, "noise"), [])) == 0
    with pytest.raises(RuntimeError, match="box 1 "):
        clf.windows_to_cifar(picture(50, 50, "RGB", 1, "noise"), [(0, 0, 10, 10), (45, 45, 51, 50)])


def test_second_call_after_other_sizes(clf):
    """coefficient tables and buffers hold no state from one call to the next"""
    a = picture(SMALL[0], SMALL[1], "RGB", 77, "noise")
    boxes_a = notebook_tiles(SMALL[0], SMALL[1], (64, 96)) + [(0, 0, 20, 20)]
    first = clf.windows_to_cifar(a, boxes_a)
    same_records(first, a, boxes_a)
    b = picture(345, 400, "RGBA", 78, "noise")
    boxes_b = notebook_tiles(345, 400, (33, 140)) + [(0, 0, 345, 400), (0, 0, 2, 201), (0, 0, 257, 257)]
    clf.windows_to_cifar(b, boxes_b)
    clf.classify_windows(b, boxes_b[:40])
    assert (clf.windows_to_cifar(a, boxes_a) == first).all()
    got = np.asarray(clf.classify_windows(a, boxes_a))
    clf.classify_windows(b, boxes_b)
    assert (np.asarray(clf.classify_windows(a, boxes_a)) == got).all()
