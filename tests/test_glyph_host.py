"""CPU: the host half of the glyph entry points (csrc/glyphs.cpp, resample_coeffs in csrc/resample.cpp) through the two
host-only symbols bnn_mi355x_glyph_fit and bnn_mi355x_resample_coeffs.  The fit rule against the notebooks' Python
expressions for every ink box up to 1200 x 1200; the coefficient tables, applied in numpy exactly as the record kernel
applies them (clip8((2^21 + sum p k) >> 22)), against Image.resize itself."""
import ctypes as C

import numpy as np
import pytest

import gpu_lib as gl

PIL = pytest.importorskip("PIL")
from PIL import Image  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    return gl.load("lfcW1A1")


def test_glyph_fit_equals_the_notebook(lib):
    """cell 11: ratio = min(28./height, 28./width); (28, 28) / (int(width*ratio), 28) / (28, int(height*ratio)); the paste
    at int((28 - size) / 2); a dimension of 0 is status 2"""
    N = 1200
    w, h = np.meshgrid(np.arange(1, N + 1), np.arange(1, N + 1), indexing="ij")
    ratio = np.minimum(28. / h, 28. / w)
    ow = np.where(h == w, 28, np.where(h > w, (w * ratio).astype(np.int64), 28))
    oh = np.where(h == w, 28, np.where(h > w, 28, (h * ratio).astype(np.int64)))
    status = np.where((ow == 0) | (oh == 0), 2, 0)
    px = ((28 - ow) / 2).astype(np.int64)
    py = ((28 - oh) / 2).astype(np.int64)
    # the numpy form is the notebook's: spot-check it against plain Python floats
    for a, b in [(1, 28), (1, 29), (3, 7), (1200, 43), (1200, 42), (577, 1111), (28, 783), (28, 785)]:
        r = min((28. / b), (28. / a))
        want = (28, 28) if a == b else (int(a * r), 28) if b > a else (28, int(b * r))
        assert (ow[a - 1, b - 1], oh[a - 1, b - 1]) == want
    got = np.zeros((N, N, 5), np.int32)
    out = (C.c_int * 5)()
    fit = lib.bnn_mi355x_glyph_fit
    for a in range(1, N + 1):
        row = got[a - 1]
        for b in range(1, N + 1):
            fit(a, b, out)
            row[b - 1] = out
    ok = status == 0
    assert (got[:, :, 4] == status).all()
    assert (got[:, :, 0][ok] == ow[ok]).all() and (got[:, :, 1][ok] == oh[ok]).all()
    assert (got[:, :, 2][ok] == px[ok]).all() and (got[:, :, 3][ok] == py[ok]).all()
    assert status.sum() > 0 and lib.bnn_mi355x_glyph_fit(1, 29, None) == 2 and lib.bnn_mi355x_glyph_fit(1, 28, None) == 0
    assert lib.bnn_mi355x_glyph_fit(0, 5, None) == 2 and lib.bnn_mi355x_glyph_fit(5, -1, None) == 2


def tables(lib, filt, n_in, n_out):
    ksize = lib.bnn_mi355x_resample_coeffs(filt, n_in, n_out, None, None, 0)
    assert ksize > 0
    kk = np.zeros((n_out, ksize), np.int32)
    bounds = np.zeros((n_out, 2), np.int32)
    assert lib.bnn_mi355x_resample_coeffs(filt, n_in, n_out, kk.ctypes.data, bounds.ctypes.data, kk.size) == ksize
    return kk, bounds


def apply_tables(rows, kk, bounds):
    """step 6 on the rows of an [r, in] uint8 array -> [r, out]"""
    out = np.zeros((rows.shape[0], len(kk)), np.uint8)
    r64 = rows.astype(np.int64)
    for xx in range(len(kk)):
        xmin, taps = int(bounds[xx, 0]), int(bounds[xx, 1])
        assert 0 <= xmin and 0 <= taps <= kk.shape[1] and xmin + taps <= rows.shape[1]
        acc = (1 << 21) + r64[:, xmin:xmin + taps] @ kk[xx, :taps].astype(np.int64)
        out[:, xx] = np.clip(acc >> 22, 0, 255)
    return out


INS = list(range(1, 121)) + [333, 600, 1170]


@pytest.mark.parametrize("filt", [0, 3])
def test_resample_coeffs_equal_pillow(lib, filt):
    """one-row "L" images (two of them stacked: the height stays, so Pillow runs the horizontal pass alone): a random row
    and a row of 0 / 255 alone, where the bicubic lobes overshoot and clip8 works at both ends"""
    rng = np.random.default_rng(5 + filt)
    checked = 0
    for n_in in INS:
        rows = np.stack([rng.integers(0, 256, n_in, dtype=np.uint8), rng.integers(0, 2, n_in, dtype=np.uint8) * 255])
        img = Image.fromarray(rows)
        for n_out in range(1, 29):
            if n_out == n_in:
                continue  # a pass whose sizes agree is skipped (Image.resize returns a copy)
            kk, bounds = tables(lib, filt, n_in, n_out)
            want = np.asarray(img.resize((n_out, 2), filt))
            got = apply_tables(rows, kk, bounds)
            assert (got == want).all(), (filt, n_in, n_out)
            checked += 1
    assert checked == len(INS) * 28 - 28


def test_resample_coeffs_refuses(lib):
    for filt, n_in, n_out in ((1, 5, 5), (2, 5, 5), (-1, 5, 5), (3, 0, 5), (3, 5, 0), (0, -2, 5)):
        assert lib.bnn_mi355x_resample_coeffs(filt, n_in, n_out, None, None, 0) == -1
        assert b"resample_coeffs" in lib.bnn_mi355x_last_error()
    # a table is written only when the caller's room holds all of it
    ksize = lib.bnn_mi355x_resample_coeffs(3, 16, 4, None, None, 0)
    assert ksize == 17  # support 2 x scale 4 on either side of the centre, plus one
    kk = np.full(4 * ksize - 1, -7, np.int32)
    assert lib.bnn_mi355x_resample_coeffs(3, 16, 4, kk.ctypes.data, None, kk.size) == ksize and (kk == -7).all()
