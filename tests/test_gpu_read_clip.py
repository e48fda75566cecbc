"""GPU: read a clip -- the glyphs of all frames in one set of launches (bnn_mi355x_find_glyphs_clip, bnn_mi355x_clip_to_mnist,
bnn_mi355x_read_clip, LfcClassifier.*_clip; csrc/clip_glyph_kernels.hip, csrc/clip_glyphs.h).

Everything has an exact answer: per frame, what the one-picture calls return for that frame alone.  The labelling is held
against tests/ccl_ref.py frame by frame; the whole calls against the oracle chain of test_gpu_read_page.py (ccl_ref labels ->
np.where(labels == i, plane, 255) -> Pillow through glyph_ref -> lines_ref).  lfcW1A1 with the mnist parameters."""
import ctypes as C
import functools

import numpy as np
import pytest

import ccl_ref
import gpu_lib as gl
from test_gpu_read_page import abi, classes_of_records, oracle, read_gpu, same_page

PIL = pytest.importorskip("PIL")
from PIL import Image, ImageDraw, ImageFont  # noqa: E402

pytestmark = pytest.mark.gpu

IDENTITY = (1.0, 1.0, -1)


@pytest.fixture(scope="module")
def clf():
    import bnn
    return bnn.LfcClassifier(bnn.NETWORK_LFCW1A1, "mnist", bnn.RUNTIME_SW)


def err(L):
    return L.bnn_mi355x_last_error().decode()


def clip_args(a, opts, find, filter=3):
    """the arguments every clip entry point starts with; the structs are kept alive by the returned tuple"""
    o, f = abi.GlyphOpts(opts[0], opts[1], opts[2], filter, 0), abi.FindOpts(*find)
    return (a.ctypes.data, a.shape[0], 0, a.shape[2], a.shape[1], 1 if a.ndim == 3 else a.shape[3], 0, C.byref(o), C.byref(f)), (o, f)


def out_arrays(n, cap, *shapes):
    return [np.full((n, cap) + s, -7, np.int32) for s in shapes], np.full(n, -1, np.int32), np.full(n, -1, np.int32)


# ---- 1  the labelling against ccl_ref, frame by frame -----------------------------------------------------------------------
def frames_of(kind, w, h, f):
    if kind in ("noise 0.3", "noise 0.6"):  # on both sides of the percolation point
        return np.stack([ccl_ref.noise(w, h, float(kind[6:]), seed) for seed in range(f)])
    if kind == "spiral":  # one square spiral cut to the frame: its arms cross every tile border
        return np.stack([ccl_ref.spiral(max(w, h))[:h, :w]] * f)
    a = np.full((f, h, w), 0 if kind == "all ink" else 255, np.uint8)
    if kind == "frame seam":  # the rows on both sides of every seam between two frames
        a[1:, :16] = 0
        a[:-1, -16:] = 0
    return a


@functools.lru_cache(maxsize=None)
def labelled(frame_bytes, w, h, reach):
    """ccl_ref's answer for one frame, computed once per (frame, reach) and shared; callers leave it unchanged"""
    return ccl_ref.label(np.frombuffer(frame_bytes, np.uint8).reshape(h, w), reach=reach, order=0)


@pytest.mark.parametrize("reach", [(1, 1), (16, 1), (4, 16), (16, 16)])
@pytest.mark.parametrize("f", [1, 3])
@pytest.mark.parametrize("h", [31, 32, 33, 65])
@pytest.mark.parametrize("w", [63, 64, 65, 130])
def test_labelling_equals_the_oracle_frame_by_frame(clf, w, h, f, reach):
    L = clf.bnn.interface
    cap = ((w + 1) // 2) * ((h + 1) // 2)
    for kind in ("noise 0.3", "noise 0.6", "spiral", "all ink", "frame seam"):
        a = frames_of(kind, w, h, f)
        (boxes, counts), found, kept = out_arrays(f, cap, (4,), ())
        labels = np.full((f, h, w), -7, np.int32)
        args, keep = clip_args(a, IDENTITY, (255, reach[0], reach[1], 1, 0))
        assert L.bnn_mi355x_find_glyphs_clip(*args, boxes.ctypes.data, counts.ctypes.data, labels.ctypes.data, cap, found.ctypes.data,
                                             kept.ctypes.data) == 0, err(L)
        for i in range(f):
            want = labelled(a[i].tobytes(), w, h, reach)
            k = int(kept[i])
            ccl_ref.same((boxes[i, :k], counts[i, :k], int(found[i]), labels[i]), want, (kind, w, h, f, reach, "frame", i))
            assert (boxes[i, k:] == -7).all() and (counts[i, k:] == -7).all()
        if kind == "frame seam" and f == 3 and h == 65:
            assert found.tolist() == [1, 2, 1]  # the ink on the two sides of a seam never joins, at any reach


# ---- 2  whole-call parity on a 3-frame 96 x 70 clip of drawn digits ------------------------------------------------------------
def digits(rows, background, w=96, h=70):
    img = Image.new("L", (w, h), background)
    draw, font = ImageDraw.Draw(img), ImageFont.load_default(size=26)
    for j, row in enumerate(rows):
        for i, ch in enumerate(row):
            if ch != " ":
                draw.text((4 + 18 * i, 2 + 34 * j), ch, font=font, fill=10)
    return np.asarray(img)


CONTRAST, INK = (1.5, 1.0, -1), 100  # the backgrounds come out grey: ink is what lies below 100
CLIP = np.stack([digits(("3141", "59 26"), 255), digits(("271", "8 28"), 200), digits(("16180", "339"), 140)])


def clip_gpu(clf, a, symbol, mask=1, lines=1, word_gap=0, ink_level=255, reach=(1, 1), min_pixels=1, order=1, cap=64, opts=IDENTITY):
    """clip_to_mnist or read_clip -> one dict per frame, as test_gpu_read_page's page_gpu / read_gpu make them"""
    L = clf.bnn.interface
    n = len(a)
    g = abi.PageOpts(mask, lines, word_gap)
    (boxes, status, line, gap), found, kept = out_arrays(n, cap, (4,), (), (), ())
    args, keep = clip_args(a, opts, (ink_level, reach[0], reach[1], min_pixels, order))
    if symbol == "clip_to_mnist":
        recs = np.full((n, cap, 784), 0xAB, np.uint8)
        assert L.bnn_mi355x_clip_to_mnist(*args, C.byref(g), cap, found.ctypes.data, kept.ctypes.data, boxes.ctypes.data, recs.ctypes.data,
                                          status.ctypes.data, line.ctypes.data, gap.ctypes.data) == 0, err(L)
    else:
        usec, pre = C.c_float(-1), C.c_float(-1)
        p = L.bnn_mi355x_read_clip(*args, C.byref(g), 10, cap, found.ctypes.data, kept.ctypes.data, boxes.ctypes.data, line.ctypes.data,
                                   gap.ctypes.data, C.byref(usec), C.byref(pre), status.ctypes.data)
        assert p, err(L)
        classes = np.ctypeslib.as_array(p, shape=(n, cap)).astype(np.int32, copy=True)
        L.free_results(p)
    out = []
    for i in range(n):
        k = min(int(found[i]), cap)
        assert kept[i] == k  # ... and the slots behind them stay as the caller left them
        assert (boxes[i, k:] == -7).all() and (status[i, k:] == -7).all() and (line[i, k:] == -7).all() and (gap[i, k:] == -7).all()
        d = dict(boxes=boxes[i, :k], status=status[i, :k], line=line[i, :k], gap=gap[i, :k], total=int(found[i]))
        if symbol == "clip_to_mnist":
            assert (recs[i, k:] == 0xAB).all()
            d["records"] = recs[i, :k]
        else:
            assert (classes[i, k:] == -1).all()
            d["classes"] = classes[i, :k]
        out.append(d)
    return out


@pytest.mark.parametrize("lines", [0, 1])
@pytest.mark.parametrize("mask", [0, 1])
def test_a_clip_of_digits_equals_the_oracle_per_frame(clf, tmp_path, mask, lines):
    """the frames' backgrounds are 255, 200 and 140 under contrast 1.5: a clip-wide mean would give other planes"""
    kw = dict(mask=mask, lines=lines, ink_level=INK, opts=CONTRAST)
    records, read = clip_gpu(clf, CLIP, "clip_to_mnist", **kw), clip_gpu(clf, CLIP, "read_clip", **kw)
    for i, frame in enumerate(CLIP):
        want = oracle(frame, **kw)
        assert want["total"] >= 5
        same_page(records[i], want, ("clip_to_mnist", mask, lines, "frame", i))
        same_page(read[i], want, ("read_clip", mask, lines, "frame", i))
        assert read[i]["classes"].tolist() == classes_of_records(clf, tmp_path, want["records"], want["status"]).tolist()
    assert clf.bnn.interface.bnn_mi355x_last_find_usec() > 0


# ---- 3  edges: per frame, read_clip is read_page on that frame -----------------------------------------------------------------
EDGES = [("a frame with no ink between two with ink", np.stack([CLIP[0], np.full((70, 96), 255, np.uint8), CLIP[0]]), dict(), False),
         ("cap below a frame's total", CLIP, dict(cap=2), False),
         ("one frame", CLIP[1:2], dict(), False),
         ("two identical calls around deinit", CLIP, dict(), True)]


@pytest.mark.parametrize("what,a,kw,around_deinit", EDGES, ids=[e[0] for e in EDGES])
def test_edges_equal_read_page_per_frame(clf, what, a, kw, around_deinit):
    kw = dict(dict(ink_level=INK, opts=CONTRAST, cap=64), **kw)
    got = clip_gpu(clf, a, "read_clip", **kw)
    if around_deinit:
        clf.bnn.interface.deinit()
        again = clip_gpu(clf, a, "read_clip", **kw)
        assert [{k: np.asarray(v).tolist() for k, v in d.items()} for d in got] == [{k: np.asarray(v).tolist() for k, v in d.items()} for d in again]
    for i, frame in enumerate(a):
        want = read_gpu(clf, frame, **kw)
        for key in ("classes", "boxes", "status", "line", "gap", "total"):
            assert np.asarray(got[i][key]).tolist() == np.asarray(want[key]).tolist(), (what, "frame", i, key)
    if "no ink" in what:
        assert got[1]["total"] == 0 and len(got[1]["boxes"]) == 0 and got[0]["total"] > 0
    if "cap" in what:
        assert all(d["total"] > 2 and len(d["boxes"]) == 2 for d in got)


# ---- 4  refusals before the GPU, and Python ------------------------------------------------------------------------------------
def refused(L, a, n_frames=None, frame_stride=0):
    (boxes,), found, kept = out_arrays(len(a), 4, (4,))
    args, keep = clip_args(a, IDENTITY, (255, 1, 1, 1, 0))
    args = args[:1] + (len(a) if n_frames is None else n_frames, frame_stride) + args[3:]
    rc = L.bnn_mi355x_find_glyphs_clip(*args, boxes.ctypes.data, None, None, 4, found.ctypes.data, kept.ctypes.data)
    return err(L) if rc == -1 else None


def test_refusals_come_before_the_gpu(clf):
    L, a = clf.bnn.interface, CLIP
    assert "n_frames must be 1..4096" in refused(L, a, n_frames=0)
    assert "frame stride shorter" in refused(L, a, frame_stride=96 * 70 - 1)
    big = np.zeros((1, 8, 4096), np.uint8)  # 513 such frames are 2^24 + 32768 pixels; refused before any is read
    assert "at most 16777216 pixels" in refused(L, big, n_frames=513)
    cnv = gl.Net("cnvW1A1", "cifar10").L
    assert "LFC networks only" in refused(cnv, a)


def test_python_methods_return_what_the_c_calls_return(clf):
    kw = dict(ink_level=INK, contrast=1.5, brightness=1.0)
    want = clip_gpu(clf, CLIP, "read_clip", ink_level=INK, opts=CONTRAST, cap=4096)
    got = clf.read_clip([Image.fromarray(f) for f in CLIP], **kw)
    records = clf.clip_to_mnist(CLIP, **kw)
    found = clf.find_glyphs_clip(CLIP, order="raster", details=True, **kw)
    for i, (classes, boxes, lines, gaps) in enumerate(got):
        assert (classes.tolist(), boxes.tolist(), lines.tolist(), gaps.tolist()) == tuple(want[i][k].tolist() for k in ("classes", "boxes", "line", "gap"))
        assert records[i][1].tolist() == boxes.tolist() and records[i][0].shape == (len(boxes), 784)
        assert found[i][2] == want[i]["total"] == clf.glyphs_found[i] and sorted(found[i][0].tolist()) == sorted(boxes.tolist())
    assert clf.read_clip_text(CLIP, **kw) == [clf._page_text(*(want[i][k] for k in ("classes", "line", "gap"))) for i in range(3)]
    with pytest.raises(ValueError):
        clf.read_clip([CLIP[0], CLIP[1][:, :90]], **kw)
    with pytest.raises(ValueError):
        clf.read_clip([Image.fromarray(CLIP[0]), Image.fromarray(CLIP[1]).convert("RGB")], **kw)
