"""GPU: what the picture entry points share (csrc/runtime.hip: the result frame of the `int *` entry points, the workspace
buffers that deinit() frees).

Two things no other test reaches.  read_glyphs and read_page with more than 47 classes, where the raw words come back and
the host decodes them -- only classify_glyphs is tested there (test_gpu_glyphs.py).  And deinit() between picture calls: it
frees every workspace buffer, so the next call must find every capacity zeroed and grow again; a buffer freed with its
capacity left standing would be used after its release.  Everything is compared with this runtime's own earlier answers:
what those answers must be is the business of test_gpu_glyphs.py, test_gpu_read_page.py, test_gpu_windows.py,
test_gpu_scan.py and test_image_to_cifar.py."""
import ctypes as C

import numpy as np
import pytest

import gpu_lib as gl
import scan_ref
from gpu_lib import abi

pytestmark = pytest.mark.gpu

IDENTITY = (1.0, 1.0, -1)


def err(L):
    return L.bnn_mi355x_last_error().decode()


def taken(L, p, n):
    out = np.ctypeslib.as_array(p, shape=(max(n, 1),))[:n].astype(np.int32, copy=True)
    L.free_results(p)
    return out


def ink(shape, seed):
    """black ink, one pixel in eight a grey below 100"""
    rng = np.random.default_rng(seed)
    return np.where(rng.random(shape) < 0.125, rng.integers(1, 100, shape), 0).astype(np.uint8)


def sheet(w=64, h=48):
    """an L picture: a block, a stroke one pixel wide and 40 tall (aspect 40: status 2), a "U" and a second block"""
    a = np.full((h, w), 255, np.uint8)
    a[5:19, 2:12] = ink((14, 10), 1)
    a[2:42, 20] = ink(40, 2)
    a[24:45, 26:28] = ink((21, 2), 3); a[24:45, 44:46] = ink((21, 2), 4); a[43:45, 26:46] = ink((2, 20), 5)
    a[8:30, w - 12:w - 2] = ink((22, 10), 6)
    return a


# ---- the LFC entry points through the C ABI -------------------------------------------------------------------------------
def structs(mask=0, lines=0):
    return abi.GlyphOpts(*IDENTITY, 3, 0), abi.FindOpts(255, 1, 1, 1, 1), abi.PageOpts(mask, lines, 0)


def find_glyphs(L, a, cap=64):
    o, f, _ = structs()
    boxes = np.zeros((cap, 4), np.int32)
    total = L.bnn_mi355x_find_glyphs(a.ctypes.data, a.shape[1], a.shape[0], 1, 0, C.byref(o), C.byref(f), boxes.ctypes.data, None, None, cap)
    assert 0 <= total <= cap, err(L)
    return boxes[:total].copy()


def classify_glyphs(L, a, boxes, ncls):
    o, _, _ = structs()
    status = np.full(len(boxes), -7, np.int32)
    p = L.bnn_mi355x_classify_glyphs(a.ctypes.data, a.shape[1], a.shape[0], 1, 0, boxes.ctypes.data, len(boxes), C.byref(o), ncls, None, None,
                                     status.ctypes.data)
    assert p, err(L)
    return taken(L, p, len(boxes)), status


def read_glyphs(L, a, ncls, cap=64):
    o, f, _ = structs()
    boxes, status, found = np.full((cap, 4), -7, np.int32), np.full(cap, -7, np.int32), C.c_int(-1)
    p = L.bnn_mi355x_read_glyphs(a.ctypes.data, a.shape[1], a.shape[0], 1, 0, C.byref(o), C.byref(f), ncls, cap, C.byref(found), boxes.ctypes.data,
                                 None, None, status.ctypes.data)
    assert p, err(L)
    k = min(found.value, cap)
    return taken(L, p, k), boxes[:k], status[:k]


def read_page(L, a, ncls, mask, lines, cap=64):
    o, f, g = structs(mask, lines)
    boxes, found = np.full((cap, 4), -7, np.int32), C.c_int(-1)
    status, line, gap = np.full(cap, -7, np.int32), np.full(cap, -7, np.int32), np.full(cap, -7, np.int32)
    p = L.bnn_mi355x_read_page(a.ctypes.data, a.shape[1], a.shape[0], 1, 0, C.byref(o), C.byref(f), C.byref(g), ncls, cap, C.byref(found),
                               boxes.ctypes.data, line.ctypes.data, gap.ctypes.data, None, None, status.ctypes.data)
    assert p, err(L)
    k = min(found.value, cap)
    return taken(L, p, k), boxes[:k], status[:k], line[:k], gap[:k]


def glyphs_to_mnist(L, a, boxes):
    o, _, _ = structs()
    n = max(len(boxes), 1)
    recs, inkb, status = np.full((n, 784), 0xAB, np.uint8), np.full((n, 4), -7, np.int32), np.full(n, -7, np.int32)
    rc = L.bnn_mi355x_glyphs_to_mnist(a.ctypes.data, a.shape[1], a.shape[0], 1, 0, boxes.ctypes.data if len(boxes) else None, len(boxes), C.byref(o),
                                      recs.ctypes.data, inkb.ctypes.data, status.ctypes.data)
    assert rc == 0, err(L)
    return recs, inkb, status


def test_read_glyphs_and_read_page_decode_words_on_the_host():
    """number_class = 64: the words come back and the host decodes them.  The classes are classify_glyphs' at 64 on the boxes
    find_glyphs returns, and the 10-class call's; the stroke reads -1 with status 2"""
    L = gl.Net("lfcW1A1", "mnist").L
    a = sheet()
    boxes = find_glyphs(L, a)
    assert len(boxes) == 4 and [20, 2, 21, 42] in boxes.tolist()
    thin = boxes.tolist().index([20, 2, 21, 42])
    want, want_status = classify_glyphs(L, a, boxes, 64)
    assert want_status.tolist() == [2 if i == thin else 0 for i in range(4)]
    assert want[thin] == -1 and (np.delete(want, thin) >= 0).all() and (np.delete(want, thin) < 10).all()
    assert classify_glyphs(L, a, boxes, 10)[0].tolist() == want.tolist()
    for ncls in (64, 10):
        classes, got_boxes, status = read_glyphs(L, a, ncls)
        assert classes.tolist() == want.tolist() and got_boxes.tolist() == boxes.tolist() and status.tolist() == want_status.tolist(), ncls
        classes, got_boxes, status, line, gap = read_page(L, a, ncls, mask=0, lines=0)
        assert classes.tolist() == want.tolist() and got_boxes.tolist() == boxes.tolist() and status.tolist() == want_status.tolist(), ncls
        assert not line.any() and not gap.any()
    assert err(L) == ""


def as_bytes(results):
    return [np.ascontiguousarray(x).tobytes() for x in results]


def around_deinit(L, first, other):
    """first(), deinit(), other() on a picture of another size, deinit(), first() again -> the two answers of first()"""
    before = as_bytes(first())
    L.deinit()
    other()
    L.deinit()
    after = as_bytes(first())
    L.deinit()
    L.deinit()  # (nothing is allocated now: returns at once)
    return before, after


def test_deinit_between_picture_calls_lfc():
    """read_page (masked, in lines) and glyphs_to_mnist"""
    L = gl.Net("lfcW1A1", "mnist").L
    a, b = sheet(), sheet(90, 70)
    boxes = np.asarray([[2, 5, 12, 19], [20, 2, 21, 42], [26, 24, 46, 45], [52, 8, 62, 30]], np.int32)

    def calls(p, bx):
        return lambda: read_page(L, p, 10, mask=1, lines=1) + glyphs_to_mnist(L, p, bx)

    before, after = around_deinit(L, calls(a, boxes), calls(b, boxes[:0]))
    assert before == after
    assert np.frombuffer(before[2], np.int32).tolist().count(2) == 1  # (the sheet does hold its status-2 glyph)
    assert err(L) == ""


# ---- the CNV entry points ---------------------------------------------------------------------------------------------------
def picture(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def classify_windows(L, a, boxes, detail):
    p = L.bnn_mi355x_classify_windows(a.ctypes.data, a.shape[1], a.shape[0], 3, 0, boxes.ctypes.data, len(boxes), 10, None, None, detail)
    assert p, err(L)
    return taken(L, p, len(boxes) * (10 if detail else 1))


def scan_planes(L, planes, detail):
    _, h, w = planes.shape
    nx, ny = C.c_int(0), C.c_int(0)
    p = L.bnn_mi355x_scan_planes(planes.ctypes.data, w, h, 10, C.byref(nx), C.byref(ny), None, detail)
    assert p, err(L)
    assert (nx.value, ny.value) == ((w - 32) // 4 + 1, (h - 32) // 4 + 1)
    return taken(L, p, nx.value * ny.value * (10 if detail else 1))


def scan_scene(L, a, size, detail):
    sz = np.asarray([size], np.int32)
    windows = len(scan_ref.boxes(a.shape[1], a.shape[0], size))
    boxes = np.full((windows, 4), -1, np.int32)
    p = L.bnn_mi355x_scan_scene(a.ctypes.data, a.shape[1], a.shape[0], 3, 0, sz.ctypes.data, 1, 10, boxes.ctypes.data, None, None, detail)
    assert p, err(L)
    assert (boxes >= 0).all()
    return taken(L, p, windows * (10 if detail else 1)), boxes


def image_to_cifar(L, a):
    one = lambda v: (C.c_int * 1)(v)  # noqa: E731
    out = np.zeros(3073, np.uint8)
    assert L.bnn_mi355x_images_to_cifar((C.c_void_p * 1)(a.ctypes.data), one(a.shape[1]), one(a.shape[0]), one(3), None, 1, out.ctypes.data) == 0, err(L)
    return out


def test_deinit_between_picture_calls_cnv():
    """classify_windows, scan_planes (a 3 x 3 grid), scan_scene (one size, a resized level) and images_to_cifar; classes first,
    then scores"""
    L = gl.Net("cnvW1A1", "cifar10").L
    scene, planes, small = picture(64, 48, 1), np.ascontiguousarray(picture(40, 40, 2).transpose(2, 0, 1)), picture(40, 30, 3)
    scene2, planes2, small2 = picture(80, 56, 4), np.ascontiguousarray(picture(48, 44, 5).transpose(2, 0, 1)), picture(52, 36, 6)
    boxes = np.asarray([[0, 0, 40, 40], [20, 8, 64, 48]], np.int32)

    def calls(sc, pl, sm, size):
        def run():
            out = []
            for detail in (0, 1):
                out.append(classify_windows(L, sc, boxes, detail))
                out.append(scan_planes(L, pl, detail))
                out.extend(scan_scene(L, sc, size, detail))
            return out + [image_to_cifar(L, sm)]
        return run

    assert scan_ref.level(64, 48, 48) == (42, 32) and scan_ref.level(80, 56, 56) == (45, 32)  # resized levels: 3 x 1 and 4 x 1 windows
    before, after = around_deinit(L, calls(scene, planes, small, 48), calls(scene2, planes2, small2, 56))
    assert before == after
    assert len(before[1]) == 9 * 4 and len(before[5]) == 90 * 4  # (scan_planes: 9 classes; with scores: 9 x 10 ints)
    assert err(L) == ""
