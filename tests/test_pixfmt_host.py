"""CPU: bnn_mi355x_unpack_frames_host -- the pixel formats' model on the host (csrc/pixfmt.cpp, DESIGN.md 9 "Camera frames")
-- against Pillow on every (Y, Cb, Cr) triple, against tests/pixfmt_ref.py (the model restated in numpy) on small frames of
every format with padded strides, and what the entry points refuse before anything touches a GPU.  Every comparison is
exact.  Host only: any library (a CNV and an LFC one are used)."""
import ctypes as C

import numpy as np
import pytest

import pixfmt_cases as pc
import pixfmt_ref as ref

PIL = pytest.importorskip("PIL")
from PIL import Image  # noqa: E402

FORMATS = sorted(ref.FORMATS)


@pytest.fixture(scope="module", params=["cnvW1A1", "lfcW1A1"])
def lib(request):
    return pc.gl.load(request.param)


@pytest.fixture(scope="module")
def cnv():
    return pc.gl.load("cnvW1A1")


def test_the_integer_tables_are_the_floating_point_statement():
    """pixfmt.h computes T_c[i] as (c100k * (i - 128) + 50000) / 100000 with C's truncating division: all 1024 entries"""
    x = np.arange(256, dtype=np.int64) - 128
    for c, row in zip(ref.COEFFS, ref.tables()):
        c100k = round(c * 64 * 100000)
        assert c100k == c * 64 * 100000 or abs(c100k - c * 64 * 100000) < 1e-6
        num = c100k * x + 50000
        trunc = np.sign(num) * (np.abs(num) // 100000)
        assert np.array_equal(trunc, row), c
        assert np.abs(num).max() < 2 ** 31


@pytest.mark.parametrize("video_range", [0, 1])
def test_every_triple(cnv, video_range):
    """all 2^24 (Y, Cb, Cr) in one 4096 x 4096 NV12 frame: range 0 equals Pillow's convert("RGB") from YCbCr, range 1 the
    numpy model; in each channel at least 1 % of the outputs clip at each end"""
    buf, y, cb, cr = pc.exhaustive_nv12()
    got = pc.unpack(cnv, pc.HOST, buf, pc.struct("nv12", 4096, 4096, 1, video_range=video_range))[0]
    before = ref.yuv_to_rgb(y, cb, cr, video_range, clip=False)
    for ch in range(3):
        low, high = (before[..., ch] < 0).mean(), (before[..., ch] > 255).mean()
        print("range", video_range, "channel", ch, "clipped low %.4f high %.4f" % (low, high))
        assert low >= 0.01 and high >= 0.01
    if video_range == 0:
        want = np.asarray(Image.merge("YCbCr", [Image.fromarray(p) for p in (y, cb, cr)]).convert("RGB"))
    else:
        want = np.clip(before, 0, 255).astype(np.uint8)
    assert np.array_equal(got, want), int((got != want).any(axis=-1).sum())


def test_pinned_video_range_triples(cnv):
    for (y, cb, cr), rgb in (((16, 128, 128), (0, 0, 0)), ((235, 128, 128), (255, 255, 255)), ((81, 90, 240), (255, 0, 0))):
        assert tuple(ref.yuv_to_rgb(y, cb, cr, 1)) == rgb
        frame = np.array([y, y, y, y, cb, cr], np.uint8)  # NV12, 2 x 2
        got = pc.unpack(cnv, pc.HOST, frame, pc.struct("nv12", 2, 2, 1, video_range=1))
        assert (got.reshape(-1, 3) == rgb).all()


@pytest.mark.parametrize("h", [2, 6])
@pytest.mark.parametrize("w", [2, 4, 6, 34, 66])
@pytest.mark.parametrize("fmt", FORMATS)
def test_small_frames_equal_the_numpy_model(lib, fmt, w, h):
    """3 frames, a row stride wider than the row (odd where the format allows it), a frame stride with a gap, random padding:
    the numpy model on the same bytes, and the same frames without any padding"""
    s, fs = pc.padded_strides(fmt, w, h)
    buf = pc.random_frames(fmt, w, h, 3, s, fs)
    for video_range in (0, 1):
        got = pc.unpack(lib, pc.HOST, buf, pc.struct(fmt, w, h, 3, s, fs, video_range))
        assert np.array_equal(got, ref.unpack(buf, fmt, w, h, 3, s, fs, video_range)), (fmt, w, h, video_range)
        tight = ref.packed(buf, fmt, w, h, 3, s, fs)
        assert len(tight) == ref.geometry(fmt, w, h, 3)[3]
        assert np.array_equal(pc.unpack(lib, pc.HOST, tight, pc.struct(fmt, w, h, 3, video_range=video_range)), got)


def test_frame_equivalences(cnv):
    w, h = 34, 6
    rng = np.random.default_rng(5)
    y, cb, cr = rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h // 2, w // 2), dtype=np.uint8), rng.integers(
        0, 256, (h // 2, w // 2), dtype=np.uint8)
    i420 = np.concatenate([y.ravel(), cb.ravel(), cr.ravel()])
    nv12 = np.concatenate([y.ravel(), np.stack([cb, cr], axis=-1).ravel()])
    # YUYV carries a chroma sample per row: the rows of the 4:2:0 chroma doubled
    yuyv = np.stack([y[:, 0::2], np.repeat(cb, 2, axis=0), y[:, 1::2], np.repeat(cr, 2, axis=0)], axis=-1).ravel()
    for video_range in (0, 1):
        a = pc.unpack(cnv, pc.HOST, nv12, pc.struct("nv12", w, h, 1, video_range=video_range))
        assert np.array_equal(pc.unpack(cnv, pc.HOST, i420, pc.struct("i420", w, h, 1, video_range=video_range)), a)
        assert np.array_equal(pc.unpack(cnv, pc.HOST, yuyv, pc.struct("yuyv", w, h, 1, video_range=video_range)), a)
    rgb = rng.integers(0, 256, (2, h, w, 3), dtype=np.uint8)
    bgr = np.ascontiguousarray(rgb[..., ::-1])
    assert np.array_equal(pc.unpack(cnv, pc.HOST, bgr, pc.struct("bgr", w, h, 2)), rgb)
    assert np.array_equal(pc.unpack(cnv, pc.HOST, rgb, pc.struct("rgb", w, h, 2)), rgb)
    assert np.array_equal(pc.unpack(cnv, pc.HOST, rgb[..., 0].copy(), pc.struct("l", w, h, 2)), np.repeat(rgb[..., :1], 3, axis=-1))


REFUSED = [
    ("nv12", dict(w=5), "width"), ("i420", dict(w=5), "width"), ("yuyv", dict(w=5), "width"),
    ("nv12", dict(h=5), "height"), ("i420", dict(h=5), "height"),
    ("i420", dict(row_stride=9), "row_stride"),
    ("nv12", dict(fmt=6), "format"), ("nv12", dict(fmt=-1), "format"), ("nv12", dict(video_range=2), "range"),
    ("nv12", dict(row_stride=5), "row_stride"), ("yuyv", dict(row_stride=11), "row_stride"), ("bgr", dict(row_stride=17), "row_stride"),
    ("nv12", dict(row_stride=8, frame_stride=8 * 6 - 1), "frame_stride"),
    ("nv12", dict(frames=0), "n_frames"), ("nv12", dict(w=0), "width"), ("nv12", dict(h=0), "height"),
]


def frames_of(fmt, w=6, h=4, frames=2, row_stride=0, frame_stride=0, video_range=0):
    return pc.struct(fmt, w, h, frames, row_stride, frame_stride, video_range)


@pytest.mark.parametrize("fmt,change,word", REFUSED)
def test_refusals_name_the_argument(lib, fmt, change, word):
    change = dict(change)
    fr = frames_of(change.pop("fmt", fmt), **change)
    buf = np.zeros(4096, np.uint8)
    rc, msg = pc.unpack(lib, pc.HOST, buf, fr, raw=True)
    assert rc == -1 and msg.startswith("unpack_frames_host: ") and word in msg, msg


def test_null_pointers(lib):
    buf = np.zeros(4096, np.uint8)
    fr = frames_of("nv12")
    assert lib.bnn_mi355x_unpack_frames_host(None, buf.ctypes.data, buf.ctypes.data) == -1
    assert "frames is null" in lib.bnn_mi355x_last_error().decode()
    assert lib.bnn_mi355x_unpack_frames_host(C.byref(fr), None, buf.ctypes.data) == -1
    assert "pixels is null" in lib.bnn_mi355x_last_error().decode()
    assert lib.bnn_mi355x_unpack_frames_host(C.byref(fr), buf.ctypes.data, None) == -1
    assert "rgb_out is null" in lib.bnn_mi355x_last_error().decode()


CLIP_CALLS = ["bnn_mi355x_scan_clip_frames", "bnn_mi355x_detect_clip_frames", "bnn_mi355x_scan_clip_device", "bnn_mi355x_detect_clip_device"]


def clip_call(L, symbol, fr, buf):
    """one of the four clip entry points on 32 x 32 frames, size (32,) -> (refused, message)"""
    sz = np.asarray([32], np.int32)
    boxes, dets, counts, ncand = np.zeros((1, 4), np.int32), np.zeros((1, 1, 8), np.int32), np.zeros(8, np.int32), np.zeros(8, np.int32)
    o = pc.abi.DetectOpts(1, 0, -32769, 1, 2, 16, 1)
    pixels = buf.ctypes.data if buf is not None else None
    if "scan" in symbol:
        args = [C.byref(fr) if fr is not None else None, pixels, sz.ctypes.data, 1, 10, boxes.ctypes.data, None, None, 0]
    else:
        args = [C.byref(fr) if fr is not None else None, pixels, sz.ctypes.data, 1, 10, C.byref(o), dets.ctypes.data, counts.ctypes.data, ncand.ctypes.data,
                None, None, None]
    if symbol.endswith("_device"):
        args.append(None)
    rc = getattr(L, symbol)(*args)
    return (not rc) if "scan" in symbol else rc == -1, L.bnn_mi355x_last_error().decode()


@pytest.mark.parametrize("symbol", CLIP_CALLS)
@pytest.mark.parametrize("network", ["cnvW1A2", "cnvW2A2", "lfcW1A1", "lfcW1A2"])
def test_other_libraries_refuse_the_clip_entry_points(network, symbol):
    L = pc.gl.load(network)
    refused, msg = clip_call(L, symbol, pc.struct("nv12", 32, 32, 1), np.zeros(32 * 48, np.uint8))
    name = symbol[len("bnn_mi355x_"):]
    assert refused and msg.startswith(name + ": "), msg
    assert ("CNV networks only" in msg) if network.startswith("lfc") else ("built for cnvW1A1 only" in msg), msg


@pytest.mark.parametrize("symbol", CLIP_CALLS)
def test_the_clip_entry_points_refuse_bad_frames_without_a_gpu(cnv, symbol):
    name = symbol[len("bnn_mi355x_"):]
    buf = np.zeros(32 * 48 * 2, np.uint8)
    for fr, pixels, word in ((pc.struct("nv12", 33, 32, 1), buf, "width"), (pc.struct("i420", 32, 33, 1), buf, "height"),
                             (pc.struct("yuyv", 33, 32, 1), buf, "width"), (pc.struct("i420", 32, 32, 1, row_stride=33), buf, "row_stride"),
                             (pc.struct(7, 32, 32, 1), buf, "format"), (pc.struct("nv12", 32, 32, 1, video_range=3), buf, "range"),
                             (pc.struct("bgr", 32, 32, 1, row_stride=95), buf, "row_stride"), (pc.struct("nv12", 32, 32, 1), None, "pixels"),
                             (None, buf, "frames")):
        refused, msg = clip_call(cnv, symbol, fr, pixels)
        assert refused and msg.startswith(name + ": ") and word in msg, (word, msg)
