"""GPU: read a page -- lines of text, every glyph masked to its own ink (bnn_mi355x_page_to_mnist, bnn_mi355x_read_page,
LfcClassifier.read_page / page_to_mnist / read_text; csrc/page_kernels.hip, csrc/page.h).

Everything has an exact answer.  The oracle: tests/ccl_ref.py gives the components, their boxes and the label map;
tests/lines_ref.py the line order; for returned glyph i, np.where(labels == i, plane, 255) goes through tests/glyph_ref.py
(the notebooks' Pillow route) with box i; the classes are this runtime's classify_mnists on the oracle's records.  Every
record byte, box, status, line, gap and class must be equal.  The pictures are L arrays fed with the options {1, 1, -1},
where the enhancement is the identity, unless a test says otherwise.  lfcW1A1 with the mnist parameters throughout.

About the routes of the record kernel.  A glyph exactly 28 wide (and no taller) or 28 x 28 comes out at ratio 1: the COPY
route.  The vertical-only route needs out_w == w with out_h != h, which the fit rule gives only to narrow glyphs a little
less than 28 tall (5 x 24 -> 5 x 28), the horizontal-only one to their transposes; `routes` holds all of them, each
with foreign ink inside its box, and test_the_cases_cover_what_they_claim checks the fits."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

import ccl_ref
import glyph_ref
import gpu_lib as gl
import lines_ref

PIL = pytest.importorskip("PIL")
from PIL import Image, ImageDraw, ImageFont  # noqa: E402

sys.path.insert(0, os.path.join(gl.ROOT, "bnn-pynq_amd"))
from bnn import abi  # noqa: E402

pytestmark = pytest.mark.gpu

IDENTITY = (1.0, 1.0, -1)
MNIST = (3.0, 4.0, -1)


@pytest.fixture(scope="module")
def clf():
    import bnn
    return bnn.LfcClassifier(bnn.NETWORK_LFCW1A1, "mnist", bnn.RUNTIME_SW)


# ---- the oracle ---------------------------------------------------------------------------------------------------------
def enhanced(a, opts):
    """the enhanced L plane of a picture (array), as glyph_ref makes it"""
    if opts == IDENTITY and a.ndim == 2:
        return a
    return np.asarray(glyph_ref.enhance(Image.fromarray(a), opts[0], opts[1], None if opts[2] < 0 else opts[2])[0])


def oracle(a, mask=1, lines=1, word_gap=0, ink_level=255, reach=(1, 1), min_pixels=1, order=1, cap=64, opts=IDENTITY, filter=3, square_blank=0):
    """-> dict(records [n, 784] (zeros for status 2), boxes, status, line, gap, total, labels)"""
    plane = enhanced(a, opts)
    if lines:
        boxes, _, total, labels = ccl_ref.label(plane, ink_level=ink_level, reach=reach, min_pixels=min_pixels, order=0)
        # raster order IS ascending first pixel: the first pixel of component k is the first place its label shows
        flat = labels.reshape(-1)
        first = [int(np.argmax(flat == k)) for k in range(total)]
        sequence, line, gap = lines_ref.order_lines(boxes, first, word_gap)
        sequence, line, gap = sequence[:cap], line[:cap], gap[:cap]
        new_index = np.full(total + 1, -1, np.int32)  # (the last entry: background)
        new_index[sequence] = np.arange(len(sequence))
        labels = new_index[labels]
        boxes = boxes[sequence].reshape(-1, 4)
    else:
        boxes, _, total, labels = ccl_ref.label(plane, ink_level=ink_level, reach=reach, min_pixels=min_pixels, order=order, cap=cap)
        line, gap = [0] * len(boxes), [0] * len(boxes)
    n = len(boxes)
    recs, status = np.zeros((n, 784), np.uint8), np.zeros(n, np.int32)
    kw = dict(contrast=1.0, brightness=1.0, square_blank=bool(square_blank))
    if filter != 3:
        kw["filter"] = filter
    for i in range(n):
        picture = np.where(labels == i, plane, 255).astype(np.uint8) if mask else plane
        r, ink, s = glyph_ref.glyphs(Image.fromarray(picture), [boxes[i]], **kw)
        if mask:
            assert ink[0].tolist() == boxes[i].tolist() and s[0] != 1  # the model's consequences: the ink box IS the component's box
        recs[i], status[i] = r[0], s[0]
    return dict(records=recs, boxes=boxes, status=status, line=np.asarray(line, np.int32), gap=np.asarray(gap, np.int32), total=total,
                labels=labels)


# ---- the device -----------------------------------------------------------------------------------------------------------
def structs(mask, lines, word_gap, ink_level, reach, min_pixels, order, opts, filter, square_blank):
    return (abi.GlyphOpts(opts[0], opts[1], opts[2], filter, square_blank), abi.FindOpts(ink_level, reach[0], reach[1], min_pixels, order),
            abi.PageOpts(mask, lines, word_gap))


def page_gpu(clf, a, mask=1, lines=1, word_gap=0, ink_level=255, reach=(1, 1), min_pixels=1, order=1, cap=64, opts=IDENTITY, filter=3,
             square_blank=0, null_page=False, want_side=True):
    L = clf.bnn.interface
    bands = 1 if a.ndim == 2 else a.shape[2]
    o, f, g = structs(mask, lines, word_gap, ink_level, reach, min_pixels, order, opts, filter, square_blank)
    boxes = np.full((cap + 1, 4), -7, np.int32)
    recs = np.full((cap + 1, 784), 0xAB, np.uint8)
    status, line, gap = np.full(cap + 1, -7, np.int32), np.full(cap + 1, -7, np.int32), np.full(cap + 1, -7, np.int32)
    found = C.c_int(-1)
    rc = L.bnn_mi355x_page_to_mnist(a.ctypes.data, a.shape[1], a.shape[0], bands, 0, C.byref(o), C.byref(f), None if null_page else C.byref(g), cap,
                                    C.byref(found), boxes.ctypes.data, recs.ctypes.data, status.ctypes.data if want_side else None,
                                    line.ctypes.data if want_side else None, gap.ctypes.data if want_side else None)
    assert rc == 0, L.bnn_mi355x_last_error().decode()
    k = min(found.value, cap)
    assert (boxes[k:] == -7).all() and (recs[k:] == 0xAB).all() and (status[k:] == -7).all() and (line[k:] == -7).all() and (gap[k:] == -7).all()
    return dict(records=recs[:k], boxes=boxes[:k], status=status[:k], line=line[:k], gap=gap[:k], total=found.value)


def read_gpu(clf, a, mask=1, lines=1, word_gap=0, ink_level=255, reach=(1, 1), min_pixels=1, order=1, cap=64, opts=IDENTITY, filter=3,
             square_blank=0, null_page=False):
    L = clf.bnn.interface
    bands = 1 if a.ndim == 2 else a.shape[2]
    o, f, g = structs(mask, lines, word_gap, ink_level, reach, min_pixels, order, opts, filter, square_blank)
    boxes = np.full((cap + 1, 4), -7, np.int32)
    status, line, gap = np.full(cap + 1, -7, np.int32), np.full(cap + 1, -7, np.int32), np.full(cap + 1, -7, np.int32)
    found, usec, pre = C.c_int(-1), C.c_float(-1), C.c_float(-1)
    p = L.bnn_mi355x_read_page(a.ctypes.data, a.shape[1], a.shape[0], bands, 0, C.byref(o), C.byref(f), None if null_page else C.byref(g), 10, cap,
                               C.byref(found), boxes.ctypes.data, line.ctypes.data, gap.ctypes.data, C.byref(usec), C.byref(pre), status.ctypes.data)
    assert p, L.bnn_mi355x_last_error().decode()
    k = min(found.value, cap)
    classes = np.ctypeslib.as_array(p, shape=(max(k, 1),))[:k].astype(np.int32, copy=True)
    L.free_results(p)
    assert (boxes[k:] == -7).all() and (status[k:] == -7).all() and (line[k:] == -7).all() and (gap[k:] == -7).all()
    return dict(classes=classes, boxes=boxes[:k], status=status[:k], line=line[:k], gap=gap[:k], total=found.value, usec=usec.value, pre=pre.value)


def classes_of_records(clf, tmp_path, records, status):
    if len(records) == 0:
        return np.zeros(0, np.int32)
    path = str(tmp_path / "page-idx3-ubyte")
    with open(path, "wb") as fh:
        fh.write(glyph_ref.idx_file(records))
    want = np.asarray(clf.classify_mnists(path)).astype(np.int32).reshape(-1)
    want[np.asarray(status) == 2] = -1
    return want


def same_page(got, want, what):
    assert got["total"] == want["total"], (what, "total", got["total"], want["total"])
    for key in ("boxes", "status", "line", "gap"):
        assert got[key].tolist() == want[key].tolist(), (what, key, got[key].tolist(), want[key].tolist())
    if "records" in got:
        assert got["records"].shape == want["records"].shape
        for i, (r, w) in enumerate(zip(got["records"], want["records"])):
            w = np.full(784, 0xAB, np.uint8) if want["status"][i] == 2 else w  # a status-2 record stays as the caller left it
            assert (r == w).all(), (what, "glyph", i, "first differing byte", int(np.argmax(r != w)))


def check(clf, tmp_path, a, what, **kw):
    """page_to_mnist and read_page against the oracle on one picture and one set of options -> (records form, oracle)"""
    want = oracle(a, **kw)
    got = page_gpu(clf, a, **kw)
    same_page(got, want, what)
    read = read_gpu(clf, a, **kw)
    same_page(read, want, what + " (read_page)")
    assert read["classes"].tolist() == classes_of_records(clf, tmp_path, want["records"], want["status"]).tolist(), what
    if len(want["boxes"]):
        assert read["usec"] > 0 and read["pre"] > 0 and clf.bnn.interface.bnn_mi355x_last_find_usec() > 0
    return got, want


# ---- the pictures: 255 is background; ink is black with one pixel in eight a grey below 100 -- a record marks the pixels
#      that come out of the resampling as exactly 0, so black ink is what shows in it, and the greys break it up -------------
def blank(w, h):
    return np.full((h, w), 255, np.uint8)


def greys(shape, seed):
    rng = np.random.default_rng(seed)
    return np.where(rng.random(shape) < 0.125, rng.integers(1, 100, shape), 0).astype(np.uint8)


def paint(a, mask, seed):
    a[mask] = greys(int(mask.sum()), seed)


def outline(a, l, u, r, b, t, seed):
    """a rectangular outline of thickness t: (l, u, r, b) is its box"""
    m = np.zeros(a.shape, bool)
    m[u:b, l:r] = True
    m[u + t:b - t, l + t:r - t] = False
    paint(a, m, seed)


def block(a, l, u, r, b, seed):
    a[u:b, l:r] = greys((b - u, r - l), seed)


def ring_with_dot():
    """37 x 29 (off the 16 and 64 grids): a ring and, inside it, a dot that is not part of it"""
    a = blank(37, 29)
    outline(a, 3, 2, 31, 26, 2, 1)
    block(a, 15, 12, 19, 16, 2)
    return a


def crossed_strokes():
    """45 x 33: a "/" and a "\\" two pixels thick that do not touch; the upper end of the "/" lies inside the box of the "\\" """
    a = blank(45, 33)
    for x in range(2, 21):
        a[30 - x, x:x + 2] = 0 if x % 5 else 77
    for x in range(18, 37):
        a[x - 16, x:x + 2] = 0 if x % 7 else 33
    return a


def tiny_glyphs():
    """24 x 24: 3 x 5 glyphs of black ink enlarged to 28 high, where every source pixel shows -- the first pixel of each, which
    the label plane marks differently from the others, included; an "L" with a foreign dot in its upper right corner"""
    a = blank(24, 24)
    a[2:7, 3] = 0; a[6, 3:6] = 0; a[2, 5] = 0               # "L" (3 x 5) and the dot (5, 2)
    a[10:15, 12:15] = 0; a[11:14, 13] = 255; a[14, 14] = 90  # "0" (3 x 5), hollow, one grey corner
    a[17:22, 18] = 0; a[17, 19:21] = 0; a[19, 19:21] = 0     # "F"
    return a


def all_borders():
    """24 x 27: one glyph touching all four borders of the picture, a dot of another component in each quadrant"""
    a = blank(24, 27)
    a[13, :] = greys(24, 4)
    a[:, 11] = greys(27, 5)
    for x, y in ((4, 4), (18, 5), (3, 20), (19, 22)):
        block(a, x, y, x + 2, y + 3, 6 + x)
    return a


def routes():
    """70 x 40 (wider than one ink word): glyphs of every route of the record kernel, each with foreign ink inside its box --
    28 x 20 (copy), 28 x 28 (copy; square), 5 x 24 (vertical pass only), 24 x 5 (horizontal pass only), and the foreign ink
    itself: dots of 2 x 3 (both passes, enlarged)"""
    a = blank(70, 40)
    outline(a, 1, 1, 29, 21, 2, 11); block(a, 12, 8, 14, 11, 12)        # 28 x 20 and a dot inside
    outline(a, 33, 2, 61, 30, 1, 13); block(a, 40, 10, 42, 13, 14)      # 28 x 28 and a dot inside
    m = np.zeros(a.shape, bool)                                          # "[" 5 x 24 at (63, 3) and a dot inside
    m[3:27, 63] = True; m[3, 63:68] = True; m[26, 63:68] = True
    paint(a, m, 15); block(a, 66, 12, 68, 15, 16)
    m = np.zeros(a.shape, bool)                                          # the same lying down, 24 x 5 at (2, 32)
    m[32, 2:26] = True; m[32:37, 2] = True; m[32:37, 25] = True
    paint(a, m, 17); block(a, 12, 35, 15, 37, 18)
    return a


def grey_background():
    """41 x 30: ink below 128; pixels of 200 inside the glyph's box are background under ink_level 128 -- whitened under the
    mask, kept without it"""
    a = blank(41, 30)
    outline(a, 4, 3, 35, 27, 3, 21)
    a[10:20, 12:25] = 200
    a[14:17, 16:20] = 0  # and a second component in the middle of the grey
    return a


def speck():
    """33 x 31: a ring and a single pixel inside it, which min_pixels = 2 drops: it is in nobody's record under the mask"""
    a = blank(33, 31)
    outline(a, 2, 3, 30, 25, 2, 22)
    a[14, 15] = 0
    return a


def thin_among_valid():
    """50 x 48: a 1 x 40 stroke (aspect 40: status 2) between valid glyphs; the stroke's lower end hangs into the box of a "U"
    without touching it"""
    a = blank(50, 48)
    block(a, 2, 5, 12, 19, 23)
    a[2:42, 20] = greys(40, 24)
    m = np.zeros(a.shape, bool)
    m[26:47, 6:8] = True; m[26:47, 47:49] = True; m[45:47, 6:49] = True
    paint(a, m, 25)
    return a


def stems_and_dots():
    """47 x 40: two stems with a bar to the right at the top and a dot 4 rows above -- six glyphs at reach (1, 1) with the two
    dashes below the bars, four at (1, 8), where each dot joins its stem; the dashes lie inside the stems' boxes at either
    reach and are within reach of nothing"""
    a = blank(47, 40)
    for x in (8, 30):
        block(a, x, 4, x + 3, 7, 26 + x)
        block(a, x, 11, x + 3, 36, 27 + x)
        block(a, x, 11, x + 11, 13, 28 + x)
        a[25, x + 7:x + 10] = 0
    return a


PICTURES = {
    "ring with dot": (ring_with_dot, {}),
    "crossed strokes": (crossed_strokes, {}),
    "tiny glyphs": (tiny_glyphs, {}),
    "all borders": (all_borders, {}),
    "routes": (routes, {}),
    "routes nearest": (routes, dict(filter=0)),
    "routes square_blank": (routes, dict(square_blank=1)),
    "routes nearest square_blank": (routes, dict(filter=0, square_blank=1)),
    "tiny glyphs nearest": (tiny_glyphs, dict(filter=0)),
    "grey background": (grey_background, dict(ink_level=128)),
    "speck": (speck, dict(min_pixels=2)),
    "thin among valid": (thin_among_valid, {}),
    "cap below the total": (routes, dict(cap=3)),
    "cap 1": (all_borders, dict(cap=1)),
    "reach (1, 1)": (stems_and_dots, dict(reach=(1, 1))),
    "reach (1, 8)": (stems_and_dots, dict(reach=(1, 8))),
    "left order, no lines": (routes, dict(lines=0, order=1)),
    "raster order, no lines": (all_borders, dict(lines=0, order=0, cap=3)),
}


@pytest.mark.parametrize("mask", [1, 0])
@pytest.mark.parametrize("name", sorted(PICTURES))
def test_records_boxes_lines_and_classes_equal_the_oracle(clf, tmp_path, name, mask):
    make, kw = PICTURES[name]
    check(clf, tmp_path, make(), name, mask=mask, **kw)


def test_the_cases_cover_what_they_claim(clf):
    """counts, fits and overlaps as the oracle sees them: each case holds what its name says"""
    L = clf.bnn.interface

    def fit(w, h):
        out = (C.c_int * 5)()
        L.bnn_mi355x_glyph_fit(w, h, out)
        return out[0], out[1]

    want = oracle(routes())
    sizes = [(int(b[2] - b[0]), int(b[3] - b[1])) for b in want["boxes"]]
    assert sorted(sizes) == sorted([(28, 20), (28, 28), (5, 24), (24, 5)] + [(2, 3)] * 3 + [(3, 2)])
    assert fit(28, 20) == (28, 20) and fit(28, 28) == (28, 28) and fit(5, 24) == (5, 28) and fit(24, 5) == (28, 5)
    assert (want["status"] == 0).all()
    assert oracle(ring_with_dot())["total"] == 2 and oracle(crossed_strokes())["total"] == 2
    tiny = oracle(tiny_glyphs())
    assert tiny["total"] == 4 and sorted((int(b[2] - b[0]), int(b[3] - b[1])) for b in tiny["boxes"]) == [(1, 1), (3, 5), (3, 5), (3, 5)]
    b = oracle(all_borders())
    assert b["total"] == 5 and [0, 0, 24, 27] in b["boxes"].tolist()
    assert oracle(speck())["total"] == 2 and oracle(speck(), min_pixels=2)["total"] == 1
    thin = oracle(thin_among_valid())
    assert thin["status"].tolist().count(2) == 1 and thin["total"] == 3
    assert oracle(stems_and_dots(), reach=(1, 1))["total"] == 6 and oracle(stems_and_dots(), reach=(1, 8))["total"] == 4
    assert oracle(grey_background(), ink_level=128)["total"] == 2 and oracle(routes(), cap=3)["total"] == 8


@pytest.mark.parametrize("name", ["ring with dot", "crossed strokes", "grey background", "speck", "tiny glyphs", "routes"])
def test_the_mask_shows(clf, tmp_path, name):
    """a glyph with foreign ink inside its box: its masked record differs from its unmasked one, so a
    kernel that forgot the mask cannot pass; both are the oracle's"""
    make, kw = PICTURES[name]
    a = make()
    masked, want_masked = check(clf, tmp_path, a, name, mask=1, **kw)
    cropped, want_cropped = check(clf, tmp_path, a, name, mask=0, **kw)
    assert masked["boxes"].tolist() == cropped["boxes"].tolist()
    differing = [i for i in range(len(masked["boxes"])) if (masked["records"][i] != cropped["records"][i]).any()]
    assert differing, name
    assert differing == [i for i in range(len(masked["boxes"])) if (want_masked["records"][i] != want_cropped["records"][i]).any()]


def test_tall_glyph_takes_the_global_temporary(clf, tmp_path):
    """an outline of 1250 x 1300: its horizontal pass leaves 26 x 1300 = 33800 bytes, more than the 32768 of LDS; inside its
    box a second component, which is a glyph of the LDS route in the same call"""
    a = blank(1300, 1300)
    outline(a, 10, 0, 1260, 1300, 4, 31)
    outline(a, 600, 500, 680, 640, 5, 32)
    got, want = check(clf, tmp_path, a, "tall", mask=1)
    assert want["boxes"].tolist() == [[10, 0, 1260, 1300], [600, 500, 680, 640]]
    cropped = page_gpu(clf, a, mask=0)
    assert (cropped["records"][1] == got["records"][1]).all()  # the inner glyph's box holds nothing else
    same_page(cropped, oracle(a, mask=0), "tall, cropped")


# ---- lines: sheets of drawn digits through the notebooks' enhancement ---------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sheet(rows, bar):
    """rows of digits, 50 pixels apart, a missing digit for a word gap; `bar`: (left, upper, right, lower) of a tall glyph"""
    width = 40 + 50 * max(len(r) for r in rows)
    img = Image.new("RGB", (width + 30, 100 * len(rows)), (238, 236, 230))
    draw = ImageDraw.Draw(img)
    font = ImageFont.load_default(size=64)
    for j, row in enumerate(rows):
        for i, ch in enumerate(row):
            if ch != " ":
                draw.text((30 + 50 * i, 12 + 100 * j), ch, font=font, fill=(25, 25, 40))
    if bar:
        draw.rectangle((bar[0], bar[1], bar[2] - 1, bar[3] - 1), fill=(25, 25, 40))
    return np.asarray(img)


def test_two_rows_a_word_gap_and_a_tall_glyph(clf, tmp_path):
    """"314 15" over "92 653"; a bar from the lower half of row 0 to the foot of row 1 overlaps row 0's band [30, 76) by 16 rows,
    less than half of it: it opens the second line, which row 1's digits then join"""
    a = sheet(("314 15", "92 653"), (352, 60, 360, 170))
    got, want = check(clf, tmp_path, a, "two rows", mask=1, word_gap=40, opts=MNIST)
    assert want["total"] == 11
    assert want["line"].tolist() == [0] * 5 + [1] * 6
    assert want["gap"].tolist() == [0, 0, 0, 1, 0] + [0, 0, 1, 0, 0, 0]
    assert want["boxes"][-1].tolist() == [352, 60, 360, 170]
    assert (np.diff(want["boxes"][:5, 0]) > 0).all() and (np.diff(want["boxes"][5:, 0]) > 0).all()
    names = [clf.class_name(c) if c >= 0 else "?" for c in classes_of_records(clf, tmp_path, want["records"], want["status"])]
    text = clf.read_text(Image.fromarray(a), lines=True, word_gap=40)
    assert text == lines_ref.text_of(names, want["line"], want["gap"])
    assert [len(t) for t in text.split("\n")] == [6, 7] and text[3] == " " and text.split("\n")[1][2] == " " and text.count(" ") == 2
    assert clf.glyph_status.tolist() == [0] * 11 and clf.glyphs_found == 11
    # read_text without the new keywords does what it did: one string in read_glyphs' order
    classes, _ = clf.read_glyphs(Image.fromarray(a))
    assert clf.read_text(Image.fromarray(a)) == "".join(clf.class_name(c) if c >= 0 else "?" for c in classes)
    check(clf, tmp_path, a, "two rows, cropped", mask=0, word_gap=40, opts=MNIST)


def test_three_rows_and_a_glyph_that_joins_two_of_them(clf, tmp_path):
    """a bar from the head of row 1 to the foot of row 2 joins row 1's line and stretches its band over row 2, whose digits
    then join it too: two lines, as the model states (a glyph as tall as two rows makes them one)"""
    a = sheet(("27", "18", "45"), (150, 115, 170, 270))
    got, want = check(clf, tmp_path, a, "three rows", mask=1, word_gap=0, opts=MNIST)
    assert want["total"] == 7 and want["line"].tolist() == [0, 0, 1, 1, 1, 1, 1] and not want["gap"].any()
    assert want["boxes"][-1].tolist() == [150, 115, 170, 270]
    # without the bar: three lines
    plain = sheet(("27", "18", "45"), None)
    got, want = check(clf, tmp_path, plain, "three rows, plain", mask=1, word_gap=30, opts=MNIST)
    assert want["line"].tolist() == [0, 0, 1, 1, 2, 2] and not want["gap"].any()
    assert clf.read_text(Image.fromarray(plain), lines=True).count("\n") == 2
    # the cap takes the first of that order
    got, want = check(clf, tmp_path, plain, "three rows, cap 3", mask=1, opts=MNIST, cap=3)
    assert want["total"] == 6 and want["line"].tolist() == [0, 0, 1]


# ---- nothing moved ------------------------------------------------------------------------------------------------------------
def read_glyphs_gpu(clf, a, order, cap=64, opts=MNIST):
    L = clf.bnn.interface
    bands = 1 if a.ndim == 2 else a.shape[2]
    o, f = abi.GlyphOpts(opts[0], opts[1], opts[2], 3, 0), abi.FindOpts(255, 1, 1, 1, order)
    boxes = np.full((cap, 4), -7, np.int32); status = np.full(cap, -7, np.int32)
    found = C.c_int(-1)
    p = L.bnn_mi355x_read_glyphs(a.ctypes.data, a.shape[1], a.shape[0], bands, 0, C.byref(o), C.byref(f), 10, cap, C.byref(found), boxes.ctypes.data,
                                 None, None, status.ctypes.data)
    assert p, L.bnn_mi355x_last_error().decode()
    k = min(found.value, cap)
    classes = np.ctypeslib.as_array(p, shape=(max(k, 1),))[:k].astype(np.int32, copy=True)
    L.free_results(p)
    return classes, boxes[:k], status[:k], found.value


@pytest.mark.parametrize("order", [0, 1])
def test_page_zero_is_read_glyphs(clf, order):
    """with page = {0, 0, 0} read_page returns exactly what read_glyphs returns on the same arguments"""
    for a, cap in ((sheet(("314 15", "92 653"), (352, 60, 360, 170)), 64), (sheet(("27", "18", "45"), None), 4), (crossed_strokes(), 64)):
        opts = MNIST if a.ndim == 3 else IDENTITY
        classes, boxes, status, found = read_glyphs_gpu(clf, a, order, cap, opts)
        got = read_gpu(clf, a, mask=0, lines=0, word_gap=0, order=order, cap=cap, opts=opts)
        assert got["total"] == found and got["classes"].tolist() == classes.tolist()
        assert got["boxes"].tolist() == boxes.tolist() and got["status"].tolist() == status.tolist()
        assert not got["line"].any() and not got["gap"].any()


def test_without_overlap_the_mask_changes_nothing(clf, tmp_path):
    """boxes that do not overlap, ink of 255-free greys on white: mask 1 and mask 0 give identical records"""
    a = blank(70, 40)
    block(a, 2, 3, 20, 30, 41)
    outline(a, 25, 5, 45, 20, 3, 42)   # (its hollow holds white only)
    block(a, 50, 1, 69, 12, 43)
    a[25:38, 48:52] = greys((13, 4), 44)
    masked, _ = check(clf, tmp_path, a, "apart", mask=1)
    cropped, _ = check(clf, tmp_path, a, "apart", mask=0)
    assert masked["total"] == 4 and (masked["records"] == cropped["records"]).all()


def test_twice_in_a_row(clf):
    """the arrival order of the atomics (root numbers are handed out in it, and they are half of a glyph's key) must not show"""
    a = np.where(ccl_ref.noise(150, 90, 0.3, 9) == 0, greys((90, 150), 45), 255).astype(np.uint8)
    first = page_gpu(clf, a, cap=200)
    second = page_gpu(clf, a, cap=200)
    assert first["total"] > 200
    same_page(second, first, "repeat")
    same_page(first, oracle(a, cap=200), "repeat")


def test_null_page_and_null_outputs(clf):
    """page == NULL is {1, 1, 0}; status, line and gap may be NULL"""
    a = sheet(("27", "18", "45"), None)
    want = page_gpu(clf, a, mask=1, lines=1, word_gap=0, opts=MNIST)
    same_page(page_gpu(clf, a, mask=0, lines=0, null_page=True, opts=MNIST), want, "NULL page")
    assert want["line"].tolist() == [0, 0, 1, 1, 2, 2]
    ring = ring_with_dot()
    assert (page_gpu(clf, ring, null_page=True)["records"] == oracle(ring)["records"]).all()  # masked, not cropped
    bare = page_gpu(clf, a, opts=MNIST, want_side=False)
    assert (bare["records"] == want["records"]).all() and bare["boxes"].tolist() == want["boxes"].tolist()
    got = read_gpu(clf, a, null_page=True, opts=MNIST)
    assert got["line"].tolist() == want["line"].tolist() and got["boxes"].tolist() == want["boxes"].tolist()


def test_a_blank_sheet_reads_as_nothing(clf):
    a = np.full((60, 90, 3), 240, np.uint8)
    got = read_gpu(clf, a, opts=MNIST)
    assert got["total"] == 0 and len(got["classes"]) == 0 and got["usec"] == 0 and got["pre"] == 0
    assert page_gpu(clf, a, opts=MNIST)["total"] == 0
    assert clf.read_text(Image.fromarray(a), lines=True) == "" and clf.glyphs_found == 0


# ---- Python -------------------------------------------------------------------------------------------------------------------
def test_python_entry_points(clf, tmp_path):
    a = sheet(("314 15", "92 653"), (352, 60, 360, 170))
    img = Image.fromarray(a)
    want = oracle(a, word_gap=40, opts=MNIST)
    classes, boxes, lines, gaps = clf.read_page(img, word_gap=40)
    assert classes.dtype == np.int32 and boxes.dtype == np.int32
    assert boxes.tolist() == want["boxes"].tolist() and lines.tolist() == want["line"].tolist() and gaps.tolist() == want["gap"].tolist()
    assert classes.tolist() == classes_of_records(clf, tmp_path, want["records"], want["status"]).tolist()
    assert clf.glyphs_found == 11 and clf.glyph_status.tolist() == want["status"].tolist() and clf.usecPreprocess > 0 and clf.usecPerImage > 0
    recs, rboxes, status, rlines, rgaps = clf.page_to_mnist(img, word_gap=40)
    assert (recs == want["records"]).all() and rboxes.tolist() == boxes.tolist() and status.tolist() == want["status"].tolist()
    assert rlines.tolist() == lines.tolist() and rgaps.tolist() == gaps.tolist()
    # the knobs: no mask, no lines, a cap
    want = oracle(a, mask=0, lines=0, order=0, cap=4, opts=MNIST)
    recs, rboxes, status, rlines, rgaps = clf.page_to_mnist(img, mask=False, lines=False, order="raster", max_glyphs=4)
    assert (recs == want["records"]).all() and rboxes.tolist() == want["boxes"].tolist() and clf.glyphs_found == 11 and not rlines.any()
    with pytest.raises(RuntimeError, match="word_gap needs line_order 1"):
        clf.read_page(img, lines=False, word_gap=3)
    with pytest.raises(ValueError):
        clf.read_page(img, order="up")
