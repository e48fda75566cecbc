"""GPU: from a picture to MNIST-format records and classes in one call (bnn_mi355x_enhance_picture,
bnn_mi355x_glyphs_to_mnist, bnn_mi355x_classify_glyphs, LfcClassifier.enhance / glyphs_to_mnist / classify_glyphs /
classify_image; LFC-BNN_MNIST_Webcam.ipynb and LFC-BNN_Chars_Webcam.ipynb cells 9-13).

The reference is Pillow running the notebooks' cells (tests/glyph_ref.py): enhanced planes, means, records, ink boxes
and status must equal it on every byte.  The reference for classes is this runtime's own classify_mnists on an idx file
of glyph_ref's records.  lfcW1A1 with the mnist parameters throughout.
"""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

import gpu_lib as gl
import glyph_ref

PIL = pytest.importorskip("PIL")
from PIL import Image, ImageDraw, ImageFont  # noqa: E402

sys.path.insert(0, os.path.join(gl.ROOT, "bnn-pynq_amd"))
from bnn import abi  # noqa: E402

pytestmark = pytest.mark.gpu

W, H = 200, 160
FACTORS = [3, 4, 5, 2, 0.5, 1.7, 0.3, 1.0]


@pytest.fixture(scope="module")
def clf():
    import bnn
    return bnn.LfcClassifier(bnn.NETWORK_LFCW1A1, "mnist", bnn.RUNTIME_SW)


# ---- enhance_picture ------------------------------------------------------------------------------------------------
def ramp_picture(width, height, filler):
    """the 256 values 0..255 in the first pixels (every input of the blend), the rest `filler`, which steers the mean"""
    a = np.full(width * height, filler, np.uint8)
    a[:256] = np.arange(256)
    return a.reshape(height, width)


# (height, filler) of 200-pixel-wide ramp pictures -> 16 means from 0 to 255.  Mean 0 (255) needs the ramp's 32640 drowned
# in more than 65280 pixels of 0 (255): 328 rows; the others are 40 rows
MEANS = [(328, 0), (40, 0), (40, 7), (40, 20), (40, 41), (40, 64), (40, 85), (40, 100), (40, 127), (40, 128), (40, 150), (40, 180), (40, 200),
         (40, 230), (40, 254), (328, 255)]


def enhance_gpu(clf, a, contrast, brightness, threshold=-1, stride=0, width=None):
    L = clf.bnn.interface
    h = a.shape[0]
    w = a.shape[1] if width is None else width
    bands = 1 if a.ndim == 2 else a.shape[2]
    o = abi.GlyphOpts(contrast, brightness, threshold, 3, 0)
    out = np.zeros((h, w), np.uint8)
    mean = C.c_int(-1)
    assert L.bnn_mi355x_enhance_picture(a.ctypes.data, w, h, bands, stride, C.byref(o), out.ctypes.data, C.byref(mean)) == 0, \
        L.bnn_mi355x_last_error().decode()
    return out, mean.value


def same_enhancement(clf, a, contrast, brightness, threshold=-1):
    img = Image.fromarray(a)
    want, want_mean = glyph_ref.enhance(img, contrast, brightness, None if threshold < 0 else threshold)
    got, got_mean = enhance_gpu(clf, a, contrast, brightness, threshold)
    assert got_mean == want_mean, (contrast, brightness, threshold, got_mean, want_mean)
    want = np.asarray(want)
    assert (got == want).all(), (contrast, brightness, threshold, "first differing pixel", int(np.argmax(got != want)))
    return want_mean


@pytest.mark.parametrize("height,filler", MEANS)
def test_enhance_equals_pillow(clf, height, filler):
    """every pair of the factors on every input value, around one mean; the thresholds on the notebooks' pairs"""
    a = ramp_picture(W, height, filler)
    means = set()
    for c in FACTORS:
        for b in FACTORS:
            means.add(same_enhancement(clf, a, c, b))
    for t in (-1, 0, 180, 255):
        for c, b in ((3, 4.0), (5, 2.0), (1.0, 1.0), (1.7, 0.3)):
            same_enhancement(clf, a, c, b, t)
    assert len(means) == 1
    if (height, filler) == (328, 0):
        assert means == {0}
    if (height, filler) == (328, 255):
        assert means == {255}


def test_enhance_means_are_sixteen():
    got = {glyph_ref.enhance(Image.fromarray(ramp_picture(W, h, f)))[1] for h, f in MEANS}
    assert len(got) == 16 and 0 in got and 255 in got


@pytest.mark.parametrize("mode", ["RGB", "RGBA"])
def test_enhance_colour_pictures(clf, mode):
    """greyscale as Pillow's convert("L") does it (alpha ignored), on a width that is no multiple of 16"""
    rng = np.random.default_rng(9)
    a = rng.integers(0, 256, (37, 131, 3 if mode == "RGB" else 4), dtype=np.uint8)
    a[0, :, :3] = np.arange(131)[:, None] * [1, 0, 0]  # pure channels: every weight on its own
    a[1, :, :3] = np.arange(131)[:, None] * [0, 1, 0]
    a[2, :, :3] = np.arange(131)[:, None] * [0, 0, 1]
    a[3, :, :3] = 255
    for c, b, t in ((3, 4.0, -1), (5, 2.0, 180), (1.0, 1.0, -1), (1.7, 0.5, 0), (0.3, 2, 255), (0.5, 1.7, -1)):
        same_enhancement(clf, a, c, b, t)


@pytest.mark.parametrize("bands", [1, 3, 4])
def test_enhance_row_stride(clf, bands):
    """a picture 131 pixels wide as a view into a larger array == its packed copy"""
    rng = np.random.default_rng(bands)
    big = rng.integers(0, 256, (60, 180, bands), dtype=np.uint8)
    view = big[5:45, 20:151]
    packed = np.ascontiguousarray(view)
    for c, b in ((3, 4.0), (1.7, 0.3)):
        got_view = enhance_gpu(clf, view, c, b, stride=180 * bands, width=131)
        got_packed = enhance_gpu(clf, packed, c, b)
        assert got_view[1] == got_packed[1] and (got_view[0] == got_packed[0]).all()
        same_enhancement(clf, packed[:, :, 0] if bands == 1 else packed, c, b)


def test_enhance_mean_on_the_rounding_edge(clf):
    """n = 8000 pixels: sum 796000 puts 2 sum + n exactly on 200 n (mean 99.5 -> 100), one less leaves it below (-> 99)"""
    a = np.full(W * 40, 99, np.uint8)
    a[:4000] = 100
    a = a.reshape(40, W)
    assert int(a.sum()) == 796000
    b = a.copy()
    b[39, 199] = 98
    for pic, want in ((a, 100), (b, 99)):
        for c in (3, 1.7, 0.5):
            assert same_enhancement(clf, pic, c, 1.0) == want
        assert enhance_gpu(clf, pic, 1.0, 1.0)[1] == want


# ---- glyphs_to_mnist ------------------------------------------------------------------------------------------------
IDENTITY = dict(contrast=1.0, brightness=1.0)


def white(w=W, h=H):
    return Image.new("L", (w, h), 255)


def noise_block(img, box, seed):
    """ink of every grey but white, so that the resampling sees more than 0 and 255"""
    rng = np.random.default_rng(seed)
    w, h = box[2] - box[0], box[3] - box[1]
    img.paste(Image.fromarray(rng.integers(0, 255, (h, w), dtype=np.uint8)), (box[0], box[1]))


def case_edges():
    """ink touching each picture edge and each edge of its box; ink inside its box; boxes that overlap"""
    img = white()
    d = ImageDraw.Draw(img)
    d.rectangle((0, 50, 10, 70), fill=0)      # left edge of the picture
    d.rectangle((90, 0, 110, 8), fill=30)     # upper edge
    d.rectangle((190, 60, 199, 90), fill=0)   # right edge
    d.rectangle((60, 150, 100, 159), fill=90)  # lower edge
    d.line((30, 20, 70, 44), fill=0, width=3)
    noise_block(img, (120, 100, 150, 141), 1)
    boxes = [(0, 40, 30, 80), (80, 0, 120, 20), (170, 50, 200, 100), (50, 140, 110, 160),  # ink on a picture edge, box larger
             (0, 50, 11, 71), (90, 0, 111, 9), (190, 60, 200, 91), (60, 150, 101, 160),    # the box IS the ink box
             (20, 10, 80, 50), (25, 15, 75, 48), (0, 0, 200, 160),                          # overlapping; the whole picture
             (120, 100, 150, 141), (110, 95, 160, 150), (125, 105, 140, 120)]               # noise: around it, and inside it
    return img, boxes, IDENTITY


def case_sizes():
    """w' and h' odd and even, w' = 1, a 1 x 1 glyph, a glyph smaller than 28 next to a larger one, a blank box, squares"""
    img = white()
    noise_block(img, (5, 5, 45, 25), 2)       # 40 x 20 -> 28 x 14
    noise_block(img, (50, 5, 90, 35), 3)      # 40 x 30 -> 28 x 21
    noise_block(img, (95, 5, 115, 45), 4)     # 20 x 40 -> 14 x 28
    noise_block(img, (120, 5, 150, 45), 5)    # 30 x 40 -> 21 x 28
    noise_block(img, (192, 5, 194, 60), 6)    # 2 x 55 -> 1 x 28 (aspect 27.5)
    noise_block(img, (170, 5, 171, 33), 7)    # 1 x 28 -> 1 x 28: the aspect of exactly 28, no pass at all
    img.putpixel((180, 80), 17)               # 1 x 1 -> 28 x 28
    noise_block(img, (5, 60, 15, 74), 8)      # 10 x 14 -> 20 x 28: enlarged
    noise_block(img, (20, 60, 80, 140), 9)    # 60 x 80 -> 21 x 28
    noise_block(img, (90, 60, 118, 88), 10)   # 28 x 28: square, copied
    noise_block(img, (125, 60, 160, 95), 11)  # 35 x 35: square, shrunk
    noise_block(img, (90, 100, 103, 113), 12)  # 13 x 13: square, enlarged
    noise_block(img, (110, 120, 166, 148), 13)  # 56 x 28 -> 28 x 14: the height halves exactly
    boxes = [(0, 0, 48, 30), (48, 0, 92, 40), (93, 0, 117, 50), (118, 0, 155, 50), (188, 0, 198, 65), (167, 0, 175, 40), (175, 70, 190, 90),
             (0, 55, 17, 80), (18, 55, 85, 145), (0, 55, 85, 145), (88, 58, 120, 90), (122, 58, 165, 98), (85, 98, 108, 118), (105, 115, 170, 150),
             (176, 100, 199, 159), (199, 159, 200, 160)]  # the last two: blank
    return img, boxes, IDENTITY


def case_corners(which):
    """ink only in the first or only in the last pixel of the picture, the whole picture as the box"""
    img = white(37, 23)
    img.putpixel((0, 0) if which == "first" else (36, 22), 0)
    return img, None, IDENTITY


@functools.lru_cache(maxsize=None)
def font(size):
    return ImageFont.load_default(size=size)


def case_digits(boxes_only=None):
    """64 boxes: an 8 x 8 grid of digits from Pillow's own font, antialiased, through the notebooks' enhancement"""
    img = Image.new("RGB", (W, H), (250, 246, 240))
    d = ImageDraw.Draw(img)
    boxes = []
    for j in range(8):
        for i in range(8):
            x, y = 25 * i, 20 * j
            d.text((x + 4 + (i + j) % 5, y + (j % 3)), "0123456789"[(3 * i + j) % 10], font=font(13 + (i + 2 * j) % 6), fill=(20, 10 * i, 30))
            boxes.append((x, y, x + 25, y + 20))
    return img, boxes, {}


def case_thin():
    """a 1 x 30 line (aspect 30: status 2) in the same call as valid glyphs, which it must not affect"""
    img = white()
    d = ImageDraw.Draw(img)
    d.line((100, 10, 100, 39), fill=0)        # 1 x 30
    d.rectangle((20, 130, 79, 131), fill=0)   # 60 x 2: aspect 30 lying down
    noise_block(img, (10, 10, 50, 60), 14)
    noise_block(img, (130, 20, 190, 50), 15)
    d.text((60, 60), "8", font=font(40), fill=0)
    boxes = [(5, 5, 55, 65), (95, 5, 105, 45), (125, 15, 195, 55), (10, 125, 90, 140), (55, 55, 100, 120), (100, 10, 101, 40)]
    return img, boxes, IDENTITY


CASES = {
    "edges": case_edges, "sizes": case_sizes, "first": lambda: case_corners("first"), "last": lambda: case_corners("last"),
    "digits": case_digits, "thin": case_thin,
    "one_box": lambda: (case_digits()[0], [(50, 40, 75, 60)], {}),
    "chars": lambda: (case_digits()[0], case_digits()[1], dict(contrast=5, brightness=2.0, threshold=180)),
    "rgba": lambda: (case_digits()[0].convert("RGBA"), case_digits()[1][:9], {}),
}
VARIANTS = [dict(), dict(square_blank=True), dict(filter=0), dict(filter=0, square_blank=True)]


@functools.lru_cache(maxsize=None)
def reference(name, variant):
    """glyph_ref on a case, once for all tests that need it"""
    img, boxes, opts = CASES[name]()
    kw = dict(opts, **VARIANTS[variant])
    if kw.get("filter") is None:
        kw.pop("filter", None)  # Pillow's own default
    return img, boxes, dict(opts, **VARIANTS[variant]), glyph_ref.glyphs(img, boxes, **kw)


def same_glyphs(got, want):
    recs, ink, status = got
    wrecs, wink, wstatus = want
    assert status.tolist() == wstatus.tolist()
    assert ink.tolist() == wink.tolist()
    assert recs.shape == wrecs.shape
    for i, (r, w) in enumerate(zip(recs, wrecs)):
        assert (r == w).all(), ("glyph", i, "first differing byte", int(np.argmax(r != w)))


@pytest.mark.parametrize("variant", range(len(VARIANTS)))
@pytest.mark.parametrize("name", sorted(CASES))
def test_records_equal_the_notebooks(clf, name, variant):
    img, boxes, opts, want = reference(name, variant)
    before = img.tobytes()
    got = clf.glyphs_to_mnist(img, boxes, details=True, **opts)
    assert img.tobytes() == before  # the caller's image is left as it is
    same_glyphs(got, want)
    if name == "thin":
        assert want[2].tolist() == [0, 2, 0, 2, 0, 2]
    if name == "sizes":
        assert want[2].tolist() == [0] * 14 + [1, 1]
    if name in ("first", "last"):
        assert want[2].tolist() == [0] and (want[0] == 255).all() != VARIANTS[variant].get("square_blank", False)


def test_the_cases_cover_what_they_claim():
    """fit sizes of the `sizes` case as Pillow sees them: odd and even on both axes, w' = 1, squares on every route"""
    _, boxes, _, (recs, ink, status) = reference("sizes", 0)
    sizes = [(int(b[2] - b[0]), int(b[3] - b[1])) for b in ink]
    assert sizes[:14] == [(40, 20), (40, 30), (20, 40), (30, 40), (2, 55), (1, 28), (1, 1), (10, 14), (60, 80), (75, 80), (28, 28), (35, 35),
                          (13, 13), (56, 28)]
    _, boxes, _, (_, ink, status) = reference("digits", 0)
    assert len(boxes) == 64 and (status == 0).all() and len({(b[2] - b[0], b[3] - b[1]) for b in ink.tolist()}) >= 10


def test_status_two_leaves_the_record_alone(clf):
    """the C ABI itself: records of status-2 glyphs keep the caller's bytes; ink_boxes and status may be NULL"""
    img, boxes, opts, (wrecs, wink, wstatus) = reference("thin", 0)
    L = clf.bnn.interface
    a = np.ascontiguousarray(np.asarray(img))
    b = np.asarray(boxes, np.int32)
    o = abi.GlyphOpts(1.0, 1.0, -1, 3, 0)
    recs = np.full((len(b), 784), 0xAB, np.uint8)
    assert L.bnn_mi355x_glyphs_to_mnist(a.ctypes.data, W, H, 1, 0, b.ctypes.data, len(b), C.byref(o), recs.ctypes.data, None, None) == 0
    for i, s in enumerate(wstatus):
        assert (recs[i] == (0xAB if s == 2 else wrecs[i])).all()


def test_tall_glyph_takes_the_global_temporary(clf):
    """an ink box of 1250 x 1300: its horizontal pass leaves 26 x 1300 = 33800 bytes, more than the 32768 of LDS; next to
    it, in the same call, glyphs of the LDS route.  (A glyph this tall has to be this wide as well: one 28 times as tall
    as wide is status 2.)"""
    img = white(1300, 1300)
    noise_block(img, (10, 0, 1260, 1300), 21)
    boxes = [(0, 0, 1300, 1300), (20, 20, 60, 90), (1262, 100, 1300, 200), (10, 0, 1260, 1300), (100, 0, 1270, 1171)]
    want = glyph_ref.glyphs(img, boxes, **IDENTITY)
    assert [(int(b[2] - b[0]), int(b[3] - b[1])) for b in want[1]] == [(1250, 1300), (40, 70), (38, 100), (1250, 1300), (1160, 1171)]
    same_glyphs(clf.glyphs_to_mnist(img, boxes, details=True, **IDENTITY), want)
    same_glyphs(clf.glyphs_to_mnist(img, boxes, details=True, filter=0, **IDENTITY), glyph_ref.glyphs(img, boxes, filter=0, **IDENTITY))


def test_second_call_after_other_sizes(clf):
    """tables and buffers hold no state from one call to the next"""
    img, boxes, opts, want = reference("sizes", 0)
    same_glyphs(clf.glyphs_to_mnist(img, boxes, details=True, **opts), want)
    img2, boxes2, opts2, want2 = reference("digits", 2)
    same_glyphs(clf.glyphs_to_mnist(img2, boxes2, details=True, **opts2), want2)
    same_glyphs(clf.glyphs_to_mnist(img, boxes, details=True, **opts), want)


# ---- classify_glyphs ------------------------------------------------------------------------------------------------
def classes_of_records(clf, tmp_path, records):
    path = str(tmp_path / "glyphs-idx3-ubyte")
    with open(path, "wb") as f:
        f.write(glyph_ref.idx_file(records))
    return np.asarray(clf.classify_mnists(path))


@pytest.mark.parametrize("name", ["digits", "thin", "one_box", "chars"])
def test_classify_glyphs(clf, tmp_path, name):
    img, boxes, opts, (wrecs, _, wstatus) = reference(name, 0)
    want = classes_of_records(clf, tmp_path, wrecs)
    want[wstatus == 2] = -1
    got = np.asarray(clf.classify_glyphs(img, boxes, **opts))
    assert got.tolist() == want.tolist()
    assert clf.glyph_status.tolist() == wstatus.tolist()
    assert clf.usecPerImage > 0 and clf.usecPreprocess > 0
    # the C ABI itself, without the optional outputs; more than 47 classes: decoded on the host from the words
    L = clf.bnn.interface
    a = np.ascontiguousarray(np.asarray(img))
    b = np.asarray(boxes, np.int32)
    o = clf._glyph_opts(**opts)
    for ncls in (10, 64):
        p = L.bnn_mi355x_classify_glyphs(a.ctypes.data, W, H, 1 if a.ndim == 2 else a.shape[2], 0, b.ctypes.data, len(b), C.byref(o), ncls, None,
                                         None, None)
        assert p, L.bnn_mi355x_last_error().decode()
        res = np.ctypeslib.as_array(p, shape=(len(b),)).copy()
        L.free_results(p)
        if ncls == 10:
            assert res.tolist() == want.tolist()
        else:
            assert (res[wstatus == 2] == -1).all() and ((res >= 0) & (res < 64))[wstatus != 2].all()


def test_whole_picture_and_classify_image(clf, tmp_path):
    """boxes=None == one box around the whole picture == classify_image == the notebook's file through classify_mnist"""
    img = Image.new("RGB", (120, 100), (245, 245, 250))
    ImageDraw.Draw(img).text((40, 10), "7", font=font(70), fill=(10, 10, 10))
    wrecs, wink, wstatus = glyph_ref.glyphs(img)
    assert wstatus.tolist() == [0]
    want = classes_of_records(clf, tmp_path, wrecs)
    assert np.asarray(clf.classify_glyphs(img)).tolist() == want.tolist()
    assert np.asarray(clf.classify_glyphs(img, [(0, 0, 120, 100)])).tolist() == want.tolist()
    assert clf.classify_image(img) == int(want[0])
    assert clf.classify_image(np.asarray(img)) == int(want[0])
    path = str(tmp_path / "one-idx3-ubyte")
    with open(path, "wb") as f:
        clf.image_to_mnist(img, f)
    assert open(path, "rb").read() == glyph_ref.idx_file(wrecs)
    assert clf.classify_mnist(path) == int(want[0])
    png = str(tmp_path / "seven.png")
    img.save(png)
    assert clf.classify_path(png) == int(want[0])
    same = clf.enhance(img)
    assert same.mode == "L" and same.tobytes() == glyph_ref.enhance(img)[0].tobytes()
    thin = white(40, 40)
    ImageDraw.Draw(thin).line((5, 5, 5, 34), fill=0)
    with pytest.raises(ValueError):
        clf.classify_image(thin, **IDENTITY)
    with pytest.raises(ValueError):
        clf.image_to_mnist(thin, open(os.devnull, "wb"), **IDENTITY)


def test_cnv_library_refuses(clf):
    cnv = gl.load("cnvW1A1")
    a = np.zeros((30, 40), np.uint8)
    o = abi.GlyphOpts(3, 4, -1, 3, 0)
    out = np.zeros((30, 40), np.uint8)
    rec = np.zeros(784, np.uint8)
    assert cnv.bnn_mi355x_enhance_picture(a.ctypes.data, 40, 30, 1, 0, C.byref(o), out.ctypes.data, None) == -1
    assert b"enhance_picture" in cnv.bnn_mi355x_last_error() and b"LFC" in cnv.bnn_mi355x_last_error()
    assert cnv.bnn_mi355x_glyphs_to_mnist(a.ctypes.data, 40, 30, 1, 0, None, 0, C.byref(o), rec.ctypes.data, None, None) == -1
    assert b"glyphs_to_mnist" in cnv.bnn_mi355x_last_error() and b"LFC" in cnv.bnn_mi355x_last_error()
    assert not cnv.bnn_mi355x_classify_glyphs(a.ctypes.data, 40, 30, 1, 0, None, 0, C.byref(o), 10, None, None, None)
    assert b"classify_glyphs" in cnv.bnn_mi355x_last_error() and b"LFC" in cnv.bnn_mi355x_last_error()
