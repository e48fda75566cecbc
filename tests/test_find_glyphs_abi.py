"""CPU: bnn_mi355x_find_glyphs and bnn_mi355x_read_glyphs as bnn/abi.py declares them; what they refuse, they refuse before
anything touches a GPU, and last_error names the entry point and the reason; a CNV library has no MNIST-format records
and refuses both with the glyph entry points' sentence."""
import ctypes as C

import numpy as np
import pytest

import gpu_lib as gl
from bnn import abi

W, H = 40, 30


@pytest.fixture(scope="module")
def lib():
    return gl.load("lfcW1A1")


def test_signatures():
    L = gl.load("lfcW1A1")
    for name in ("bnn_mi355x_find_glyphs_host", "bnn_mi355x_find_glyphs", "bnn_mi355x_read_glyphs", "bnn_mi355x_last_find_usec"):
        assert name in abi.EXT and hasattr(L, name)
    assert [n for n, _ in abi.FindOpts._fields_] == ["ink_level", "reach_x", "reach_y", "min_pixels", "order"]
    assert C.sizeof(abi.FindOpts) == 20
    assert len(L.bnn_mi355x_find_glyphs_host.argtypes) == 9 and L.bnn_mi355x_find_glyphs_host.restype is C.c_int
    assert len(L.bnn_mi355x_find_glyphs.argtypes) == 11 and L.bnn_mi355x_find_glyphs.restype is C.c_int
    assert len(L.bnn_mi355x_read_glyphs.argtypes) == 14 and L.bnn_mi355x_read_glyphs.restype == C.POINTER(C.c_int)
    assert L.bnn_mi355x_last_find_usec.restype is C.c_float and L.bnn_mi355x_last_find_usec() >= 0.0


def call_both(lib, find=None, o=None, width=W, height=H, bands=3, stride=0, pixels=True, boxes=True, cap=50, use_opts=True, ncls=10,
              n_found=True):
    """the two device entry points on one set of arguments -> [(name, refused, last_error)]"""
    o = abi.GlyphOpts(3.0, 4.0, -1, 3, 0) if o is None else o
    f = abi.FindOpts(255, 1, 1, 1, 0) if find is None else find
    scene = np.zeros((H, W, 4), np.uint8)
    out = np.zeros((max(cap, 1), 4), np.int32)
    px = scene.ctypes.data if pixels else None
    op = C.byref(o) if use_opts else None
    bp = out.ctypes.data if boxes else None
    found = C.c_int(-5)
    res = []
    rc = lib.bnn_mi355x_find_glyphs(px, width, height, bands, stride, op, C.byref(f), bp, None, None, cap)
    res.append(("find_glyphs", rc == -1, lib.bnn_mi355x_last_error().decode()))
    p = lib.bnn_mi355x_read_glyphs(px, width, height, bands, stride, op, C.byref(f), ncls, cap, C.byref(found) if n_found else None, bp, None, None,
                                   None)
    res.append(("read_glyphs", not p, lib.bnn_mi355x_last_error().decode()))
    if p:
        lib.free_results(p)
    assert found.value == -5 and not out.any()  # a refused call writes nothing
    return res


@pytest.mark.parametrize("find,word", [
    (abi.FindOpts(0, 1, 1, 1, 0), "ink_level"), (abi.FindOpts(256, 1, 1, 1, 0), "ink_level"), (abi.FindOpts(255, 0, 1, 1, 0), "reach"),
    (abi.FindOpts(255, 1, 0, 1, 0), "reach"), (abi.FindOpts(255, 17, 1, 1, 0), "reach"), (abi.FindOpts(255, 1, 17, 1, 0), "reach"),
    (abi.FindOpts(255, 1, 1, 0, 0), "min_pixels"), (abi.FindOpts(255, 1, 1, 1, 2), "order"), (abi.FindOpts(255, 1, 1, 1, -1), "order"),
])
def test_bad_find_options(lib, find, word):
    for name, refused, err in call_both(lib, find=find):
        assert refused and name in err and word in err, err


def test_bad_cap_and_size(lib):
    for cap in (0, -1):
        for name, refused, err in call_both(lib, cap=cap):
            assert refused and name in err and "cap" in err, err
    for name, refused, err in call_both(lib, width=4097, height=4096):  # one row more than 2^24 pixels
        assert refused and name in err and "16777216 pixels" in err, err
    for w, h in ((0, 30), (40, 0), (65536, 30)):
        for name, refused, err in call_both(lib, width=w, height=h):
            assert refused and name in err and "picture" in err, err


def test_what_the_glyph_entry_points_refuse(lib):
    for bands in (0, 2, 5):
        for name, refused, err in call_both(lib, bands=bands):
            assert refused and name in err and "bands" in err, err
    for stride in (W * 3 - 1, -5):
        for name, refused, err in call_both(lib, stride=stride):
            assert refused and name in err and "row stride" in err, err
    for kw in (dict(pixels=False), dict(use_opts=False), dict(boxes=False)):
        for name, refused, err in call_both(lib, **kw):
            assert refused and name in err and "null" in err, err
    name, refused, err = call_both(lib, n_found=False)[1]
    assert refused and name in err and "null" in err, err
    for o, word in ((abi.GlyphOpts(-0.5, 4.0, -1, 3, 0), "contrast"), (abi.GlyphOpts(3.0, float("nan"), -1, 3, 0), "brightness"),
                    (abi.GlyphOpts(3.0, 4.0, 256, 3, 0), "threshold"), (abi.GlyphOpts(3.0, 4.0, -1, 2, 0), "filter")):
        for name, refused, err in call_both(lib, o=o):
            assert refused and name in err and word in err, err
    for ncls in (0, 65):
        name, refused, err = call_both(lib, ncls=ncls)[1]
        assert refused and "number_class" in err, err


def test_python_names_a_missing_symbol():
    """there is no second implementation in Python: a library without the entry points is an error"""
    import types

    import bnn
    fake = types.SimpleNamespace(bnn=types.SimpleNamespace(interface=object()))
    for symbol in ("bnn_mi355x_find_glyphs", "bnn_mi355x_read_glyphs"):
        with pytest.raises(RuntimeError, match=symbol):
            bnn.LfcClassifier._find_entry(fake, symbol)
    with pytest.raises(ValueError, match="order"):
        bnn.LfcClassifier._find_opts((1, 1), 1, 255, "up", 10)
    f, cap = bnn.LfcClassifier._find_opts((2, 5), 3, 200, "left", 10)
    assert (f.ink_level, f.reach_x, f.reach_y, f.min_pixels, f.order, cap) == (200, 2, 5, 3, 1, 10)


def test_cnv_library_refuses():
    cnv = gl.load("cnvW1A1")
    for name, refused, err in call_both(cnv):
        assert refused and name in err and "MNIST-format records are the input of the LFC networks only" in err, err
