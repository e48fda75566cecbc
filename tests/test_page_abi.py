"""CPU: bnn_mi355x_page_to_mnist and bnn_mi355x_read_page as bnn/abi.py declares them; what they refuse, they refuse before
anything touches a GPU, and last_error names the entry point and the reason; a CNV library has no MNIST-format records and
refuses both with the glyph entry points' sentence (bnn_mi355x_order_lines works on any library: test_page_lines.py)."""
import ctypes as C
import re

import numpy as np
import pytest

import gpu_lib as gl
from bnn import abi

W, H = 40, 30


@pytest.fixture(scope="module")
def lib():
    return gl.load("lfcW1A1")


def test_signatures_and_layouts():
    L = gl.load("lfcW1A1")
    for name in ("bnn_mi355x_order_lines", "bnn_mi355x_page_to_mnist", "bnn_mi355x_read_page"):
        assert name in abi.EXT and hasattr(L, name)
    assert [n for n, _ in abi.PageOpts._fields_] == ["mask", "line_order", "word_gap"]
    assert C.sizeof(abi.PageOpts) == 12 and [getattr(abi.PageOpts, n).offset for n, _ in abi.PageOpts._fields_] == [0, 4, 8]
    # the structs the new entry points share with the old ones keep their layouts
    assert C.sizeof(abi.FindOpts) == 20 and C.sizeof(abi.GlyphOpts) == 20
    assert len(L.bnn_mi355x_order_lines.argtypes) == 7 and L.bnn_mi355x_order_lines.restype is C.c_int
    assert len(L.bnn_mi355x_page_to_mnist.argtypes) == 15 and L.bnn_mi355x_page_to_mnist.restype is C.c_int
    assert len(L.bnn_mi355x_read_page.argtypes) == 17 and L.bnn_mi355x_read_page.restype == C.POINTER(C.c_int)
    with open(gl.ROOT + "/include/bnn_mi355x.h") as f:
        header = f.read()
    assert re.search(r"typedef struct \{\s*int mask, line_order, word_gap;\s*\} bnn_mi355x_page_opts;", header)
    assert "page:      NULL is {1, 1, 0}" in header
    assert int(re.search(r"#define BNN_MI355X_PAGE_MAX_LINE_COMPONENTS (\d+)", header).group(1)) == 65536
    with open(gl.ROOT + "/bnn-pynq_amd/csrc/page.h") as f:
        assert re.search(r"constexpr int kMaxLineComponents = 65536;", f.read())


def call_both(lib, page=None, find=None, o=None, width=W, height=H, bands=3, stride=0, pixels=True, boxes=True, cap=50, use_opts=True, ncls=10,
              n_found=True, records=True, null_page=False, only_read_page=False):
    """the two device entry points on one set of arguments -> [(name, refused, last_error)]"""
    o = abi.GlyphOpts(3.0, 4.0, -1, 3, 0) if o is None else o
    f = abi.FindOpts(255, 1, 1, 1, 0) if find is None else find
    g = abi.PageOpts(1, 1, 0) if page is None else page
    scene = np.zeros((H, W, 4), np.uint8)
    out = np.zeros((max(cap, 1), 4), np.int32)
    recs = np.zeros((max(cap, 1), 784), np.uint8)
    side = np.zeros((3, max(cap, 1)), np.int32)
    px = scene.ctypes.data if pixels else None
    op = C.byref(o) if use_opts else None
    gp = None if null_page else C.byref(g)
    bp = out.ctypes.data if boxes else None
    found = C.c_int(-5)
    res = []
    if not only_read_page:  # (page_to_mnist has no argument behind the page options to be refused for)
        rc = lib.bnn_mi355x_page_to_mnist(px, width, height, bands, stride, op, C.byref(f), gp, cap, C.byref(found) if n_found else None, bp,
                                          recs.ctypes.data if records else None, side[0].ctypes.data, side[1].ctypes.data, side[2].ctypes.data)
        res.append(("page_to_mnist", rc == -1, lib.bnn_mi355x_last_error().decode()))
    p = lib.bnn_mi355x_read_page(px, width, height, bands, stride, op, C.byref(f), gp, ncls, cap, C.byref(found) if n_found else None, bp,
                                 side[1].ctypes.data, side[2].ctypes.data, None, None, side[0].ctypes.data)
    res.append(("read_page", not p, lib.bnn_mi355x_last_error().decode()))
    if p:
        lib.free_results(p)
    assert found.value == -5 and not out.any() and not recs.any() and not side.any()  # a refused call writes nothing
    return res


@pytest.mark.parametrize("page,sentence", [
    (abi.PageOpts(2, 1, 0), "mask must be 0 (the crop of the box) or 1 (the glyph's own ink)"),
    (abi.PageOpts(-1, 1, 0), "mask must be 0 (the crop of the box) or 1 (the glyph's own ink)"),
    (abi.PageOpts(1, 2, 0), "line_order must be 0 (the order of find) or 1 (line by line)"),
    (abi.PageOpts(1, -1, 0), "line_order must be 0 (the order of find) or 1 (line by line)"),
    (abi.PageOpts(1, 1, -1), "word_gap must be 0 (none) or more"),
    (abi.PageOpts(1, 0, 3), "word_gap needs line_order 1"),
])
def test_bad_page_options(lib, page, sentence):
    for name, refused, err in call_both(lib, page=page):
        assert refused and err == "%s: %s" % (name, sentence), err


@pytest.mark.parametrize("find,sentence", [
    (abi.FindOpts(0, 1, 1, 1, 0), "ink_level must be 1..255"), (abi.FindOpts(256, 1, 1, 1, 0), "ink_level must be 1..255"),
    (abi.FindOpts(255, 0, 1, 1, 0), "reach must be 1..16 in x and in y"), (abi.FindOpts(255, 1, 17, 1, 0), "reach must be 1..16 in x and in y"),
    (abi.FindOpts(255, 1, 1, 0, 0), "min_pixels must be 1 or more"),
    (abi.FindOpts(255, 1, 1, 1, 2), "order must be 0 (raster) or 1 (left to right)"),
    (abi.FindOpts(255, 1, 1, 1, -1), "order must be 0 (raster) or 1 (left to right)"),
])
def test_bad_find_options(lib, find, sentence):
    """what read_glyphs refuses, in its words -- order 2 included, with and without the line order"""
    for page in (abi.PageOpts(1, 1, 0), abi.PageOpts(0, 0, 0)):
        for name, refused, err in call_both(lib, find=find, page=page):
            assert refused and err == "%s: %s" % (name, sentence), err


def test_bad_cap_and_size(lib):
    for cap in (0, -1):
        for name, refused, err in call_both(lib, cap=cap):
            assert refused and err == name + ": cap must be 1 or more", err
    for name, refused, err in call_both(lib, width=4097, height=4096):  # one row more than 2^24 pixels
        assert refused and err == name + ": need a picture of at most 16777216 pixels to label (4097 x 4096 given)", err
    for w, h in ((0, 30), (40, 0), (65536, 30)):
        for name, refused, err in call_both(lib, width=w, height=h):
            assert refused and err == name + ": need a picture of 1..65535 x 1..65535 pixels", err


def test_what_the_glyph_entry_points_refuse(lib):
    for bands in (0, 2, 5):
        for name, refused, err in call_both(lib, bands=bands):
            assert refused and err == name + ": bands must be 1 (L), 3 (RGB) or 4 (RGBA) bytes per pixel", err
    for stride in (W * 3 - 1, -5):
        for name, refused, err in call_both(lib, stride=stride):
            assert refused and err == name + ": row stride shorter than a row", err
    for kw in (dict(pixels=False), dict(use_opts=False), dict(boxes=False), dict(n_found=False)):
        for name, refused, err in call_both(lib, **kw):
            assert refused and err == name + ": bad arguments (null pointer)", err
    name, refused, err = call_both(lib, records=False, ncls=0)[0]  # (number_class 0: read_page, which has no records, is refused too)
    assert refused and err == "page_to_mnist: bad arguments (null pointer)", err
    for o, sentence in ((abi.GlyphOpts(-0.5, 4.0, -1, 3, 0), "contrast must be a finite factor of 0 or more"),
                        (abi.GlyphOpts(3.0, float("nan"), -1, 3, 0), "brightness must be a finite factor of 0 or more"),
                        (abi.GlyphOpts(3.0, 4.0, 256, 3, 0), "threshold must be -1 (none) or 0..255"),
                        (abi.GlyphOpts(3.0, 4.0, -1, 2, 0), "filter must be 0 (NEAREST) or 3 (BICUBIC)")):
        for name, refused, err in call_both(lib, o=o):
            assert refused and err == "%s: %s" % (name, sentence), err
    for ncls in (0, 65):
        name, refused, err = call_both(lib, ncls=ncls, only_read_page=True)[0]
        assert refused and err == "number_class must be in 1..64", err


def test_null_page_is_acceptable(lib):
    """page == NULL is the default {1, 1, 0}, no null-pointer refusal: read_page gets past the page options to the refusal
    behind them, where a bad page stops it earlier.  (That the default IS {1, 1, 0}: tests/test_gpu_read_page.py.)"""
    name, refused, err = call_both(lib, null_page=True, ncls=0, only_read_page=True)[0]
    assert refused and err == "number_class must be in 1..64", err
    name, refused, err = call_both(lib, page=abi.PageOpts(1, 0, 3), ncls=0, only_read_page=True)[0]
    assert refused and err == "read_page: word_gap needs line_order 1", err


def test_python_names_a_missing_symbol():
    """there is no second implementation in Python: a library without the entry points is an error"""
    import types

    import bnn
    fake = types.SimpleNamespace(bnn=types.SimpleNamespace(interface=object()), _find_entry=None)
    for symbol in ("bnn_mi355x_page_to_mnist", "bnn_mi355x_read_page"):
        with pytest.raises(RuntimeError, match="no %s: rebuild" % symbol):
            bnn.LfcClassifier._find_entry(fake, symbol)
    assert bnn.LfcClassifier.read_page.__defaults__[:3] == (True, True, 0)


def test_cnv_library_refuses():
    cnv = gl.load("cnvW1A1")
    for name, refused, err in call_both(cnv):
        assert refused and err == name + ": MNIST-format records are the input of the LFC networks only", err
