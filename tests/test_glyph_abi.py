"""CPU: what bnn_mi355x_enhance_picture, bnn_mi355x_glyphs_to_mnist and bnn_mi355x_classify_glyphs refuse, they refuse
before anything touches a GPU, and last_error names the reason (and the offending box); a CNV library has no MNIST-format
records."""
import ctypes as C

import numpy as np
import pytest

import gpu_lib as gl
from bnn import abi

W, H = 40, 30
GOOD = [0, 0, 40, 30]


@pytest.fixture(scope="module")
def lib():
    return gl.load("lfcW1A1")


def opts(contrast=3.0, brightness=4.0, threshold=-1, filt=3, square_blank=0):
    return abi.GlyphOpts(contrast, brightness, threshold, filt, square_blank)


def call_all(lib, boxes=(GOOD,), o=None, width=W, height=H, bands=3, stride=0, pixels=True, out=True, n=None, use_opts=True):
    """the three entry points on one set of arguments -> [(name, refused, last_error)]"""
    o = opts() if o is None else o
    scene = np.zeros((H, W, 4), np.uint8)
    b = None if boxes is None else np.ascontiguousarray(np.asarray(boxes, np.int32).reshape(-1, 4))
    nb = (0 if b is None else len(b)) if n is None else n
    bp = None if b is None else b.ctypes.data
    px = scene.ctypes.data if pixels else None
    op = C.byref(o) if use_opts else None
    plane = np.zeros((H, W), np.uint8)
    recs = np.zeros((max(nb, 1), 784), np.uint8)
    res = []
    rc = lib.bnn_mi355x_enhance_picture(px, width, height, bands, stride, op, plane.ctypes.data if out else None, None)
    res.append(("enhance_picture", rc == -1, lib.bnn_mi355x_last_error().decode()))
    rc = lib.bnn_mi355x_glyphs_to_mnist(px, width, height, bands, stride, bp, nb, op, recs.ctypes.data if out else None, None, None)
    res.append(("glyphs_to_mnist", rc == -1, lib.bnn_mi355x_last_error().decode()))
    p = lib.bnn_mi355x_classify_glyphs(px, width, height, bands, stride, bp, nb, op, 10, None, None, None)
    res.append(("classify_glyphs", not p, lib.bnn_mi355x_last_error().decode()))
    if p:
        lib.free_results(p)
    return res


BAD_BOXES = [
    ([5, 5, 5, 10], "empty"), ([6, 5, 5, 10], "empty"), ([5, 10, 9, 10], "empty"), ([5, 11, 9, 10], "empty"),
    ([-1, 0, 10, 10], "leaves"), ([0, -1, 10, 10], "leaves"), ([31, 0, 41, 10], "leaves"), ([0, 21, 10, 31], "leaves"),
]


@pytest.mark.parametrize("box,word", BAD_BOXES)
@pytest.mark.parametrize("position", [0, 2])
def test_bad_box_is_named(lib, box, word, position):
    boxes = [GOOD] * position + [box] + [GOOD]
    for name, refused, err in call_all(lib, boxes)[1:]:  # (enhance_picture takes no boxes)
        assert refused and name in err and ("box %d " % position) in err and word in err, err


@pytest.mark.parametrize("bands", [0, 2, 5, -1])
def test_bad_bands(lib, bands):
    for name, refused, err in call_all(lib, bands=bands):
        assert refused and name in err and "bands" in err, err


def test_bad_row_stride(lib):
    for stride in (W * 3 - 1, -5):
        for name, refused, err in call_all(lib, stride=stride):
            assert refused and name in err and "row stride" in err, err


@pytest.mark.parametrize("w,h", [(0, 30), (40, 0), (65536, 30), (-3, 30)])
def test_bad_picture_size(lib, w, h):
    for name, refused, err in call_all(lib, boxes=None, width=w, height=h):
        assert refused and name in err and "picture" in err, err


def test_null_pointers_and_counts(lib):
    for kw in (dict(pixels=False), dict(use_opts=False)):
        for name, refused, err in call_all(lib, **kw):
            assert refused and name in err and "null" in err, err
    for name, refused, err in call_all(lib, out=False)[:2]:  # (classify_glyphs has no output buffer of the caller's)
        assert refused and name in err and "null" in err, err
    for name, refused, err in call_all(lib, n=-1)[1:]:
        assert refused and name in err and "negative" in err, err
    scene = np.zeros((H, W, 3), np.uint8)
    o = opts()
    for ncls in (0, 65):
        assert not lib.bnn_mi355x_classify_glyphs(scene.ctypes.data, W, H, 3, 0, None, 0, C.byref(o), ncls, None, None, None)
        assert b"number_class" in lib.bnn_mi355x_last_error()


@pytest.mark.parametrize("o,word", [
    (opts(contrast=-0.5), "contrast"), (opts(contrast=float("nan")), "contrast"), (opts(contrast=float("inf")), "contrast"),
    (opts(brightness=-1e-9), "brightness"), (opts(brightness=float("nan")), "brightness"), (opts(brightness=float("-inf")), "brightness"),
    (opts(threshold=-2), "threshold"), (opts(threshold=256), "threshold"),
    (opts(filt=1), "filter"), (opts(filt=2), "filter"), (opts(filt=-1), "filter"), (opts(filt=4), "filter"),
])
def test_bad_options(lib, o, word):
    for name, refused, err in call_all(lib, o=o):
        assert refused and name in err and word in err, err


def test_cnv_library_refuses():
    cnv = gl.load("cnvW1A1")
    for name, refused, err in call_all(cnv):
        assert refused and name in err and "LFC" in err, err
    for name, refused, err in call_all(cnv, boxes=None):  # not even the whole-picture form
        assert refused and "LFC" in err, err
    # the two host-only symbols are plain arithmetic on any library
    out = (C.c_int * 5)()
    assert cnv.bnn_mi355x_glyph_fit(10, 20, out) == 0 and list(out) == [14, 28, 7, 0, 0]
