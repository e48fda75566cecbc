"""GPU: the scans' own level resize (k_scan_resize_h / _v in csrc/scan_kernels.hip, k_clip_resize_h / _v in
csrc/scan_clip_kernels.hip) against Pillow's Image.resize(size, LANCZOS), byte for byte, on every route
launch_scan_resize and launch_clip_resize can take: both passes horizontal first, both passes vertical first
(h > 100 w and the height shrinks), one pass alone in either direction, the re-layout alone, RGB and L, packed rows and
a row stride, one frame and several.

Pictures are seeded noise and the saturated "blocks" checkerboard; tests/test_resize_ref.py shows on the CPU that the
blocks pictures make clip8 work at both ends of every pass and that the two pass orders give different bytes, so a
kernel wrong in either respect cannot pass here.  Where two passes run, a failure says whether the device produced the
opposite order's bytes (tests/resize_ref.py).  The network is not under test: cnvW1A1 with the shipped cifar10
parameters only; scores are compared with classify_windows on Pillow's level picture and with scan_scene."""
import ctypes as C

import numpy as np
import pytest

import gpu_lib as gl
import resize_ref as rr
import scan_clip_ref
import scan_ref
import test_gpu_scan as gs
import test_gpu_scan_clip as gc

pytest.importorskip("PIL")

pytestmark = pytest.mark.gpu

NCLS = 10
TALL = (40, 4001)  # the smallest scene whose level (32 x 3200, size 40) takes the vertical pass first


@pytest.fixture(scope="module")
def L():
    lib = gl.load("cnvW1A1")
    lib.load_parameters(gl.param_dir("cifar10", "cnvW1A1").encode())
    assert lib.bnn_mi355x_last_error() == b"", lib.bnn_mi355x_last_error()
    return lib


def pillow_planes(a, out_w, out_h):
    return gs.pillow_planes(np.ascontiguousarray(a), (out_w, out_h))


def device_resize(L, buf, w, h, bands, row_stride, out_w, out_h):
    got = np.zeros((3, out_h, out_w), np.uint8)
    assert L.bnn_mi355x_scan_resize(buf.ctypes.data, w, h, bands, row_stride, out_w, out_h, got.ctypes.data) == 0, gs.err(L)
    return got


def differs(what, a, out_w, out_h, got, want):
    """the failure message: the case, the number of differing bytes, and -- where two passes run -- whether the device
    gave what the opposite pass order gives"""
    msg = "%s: %d of %d bytes differ from Pillow's" % (what, int((got != want).sum()), want.size)
    h, w = a.shape[:2]
    if out_w != w and out_h != h:
        other = rr.planes_of(rr.resize(np.ascontiguousarray(a), out_w, out_h, vertical_first=not rr.vertical_pass_first(w, h, out_h)))
        msg += "; the device's bytes %s those of the OPPOSITE pass order" % ("EQUAL" if (got == other).all() else "do not equal")
    return msg


def strided(a, row_stride, seed):
    """-> (buffer with rows `row_stride` bytes apart and random padding, the view of it that is the picture)"""
    h, w = a.shape[:2]
    bands = 1 if a.ndim == 2 else 3
    buf = np.random.default_rng(seed).integers(0, 256, (h, row_stride), dtype=np.uint8)
    buf[:, :w * bands] = a.reshape(h, w * bands)
    view = buf[:, :w * bands].reshape(a.shape) if a.ndim == 2 else buf[:, :w * bands].reshape(h, w, 3)
    assert (view == a).all() and view.ctypes.data == buf.ctypes.data
    return buf, view


# ---- (a) bnn_mi355x_scan_resize: every route, RGB and L, noise and blocks ------------------------------------------------
@pytest.mark.parametrize("case", rr.CASES, ids=rr.case_id)
def test_every_route_equals_pillow(L, case):
    w, h, out_w, out_h, route = case[:5]
    for mode in rr.MODES:
        for kind in rr.KINDS:
            a = rr.picture(w, h, mode, kind)
            got = device_resize(L, a, w, h, 1 if mode == "L" else 3, 0, out_w, out_h)
            want = pillow_planes(a, out_w, out_h)
            assert (got == want).all(), differs("%d x %d -> %d x %d (%s) %s %s" % (w, h, out_w, out_h, route, mode, kind), a, out_w, out_h, got, want)


# ---- (b) row strides --------------------------------------------------------------------------------------------------------
def scan_scene(L, buf, w, h, bands, row_stride, sizes, ncls, detail):
    sz = np.asarray(sizes, np.int32)
    n = sum(len(scan_ref.boxes(w, h, s)) for s in sizes)
    boxes = np.full((n, 4), -1, np.int32)
    p = L.bnn_mi355x_scan_scene(buf.ctypes.data, w, h, bands, row_stride, sz.ctypes.data, len(sz), ncls, boxes.ctypes.data, None, None, 1 if detail else 0)
    assert p, gs.err(L)
    out = np.ctypeslib.as_array(p, shape=(n * (ncls if detail else 1),)).astype(np.int32, copy=True)
    L.free_results(p)
    assert boxes.tolist() == [list(b) for s in sizes for b in scan_ref.boxes(w, h, s)]
    return out.reshape(n, ncls) if detail else out


@pytest.mark.parametrize("mode", rr.MODES)
def test_row_stride(L, mode):
    """the 80 x 72 scene as a view into rows 100 * bands bytes apart, the vertical-first 16 x 1601 one into rows 20 * bands
    apart, the padding random: scan_resize and scan_scene give what they give for the packed copy, and Pillow's bytes"""
    bands = 1 if mode == "L" else 3
    for (w, h, out_w, out_h), apart in (((80, 72, 40, 36), 100), ((16, 1601, 12, 400), 20)):
        for kind in rr.KINDS:
            a = rr.picture(w, h, mode, kind)
            buf, view = strided(a, apart * bands, seed=w + len(kind))
            what = "%d x %d -> %d x %d %s %s, rows %d bytes apart" % (w, h, out_w, out_h, mode, kind, apart * bands)
            got = device_resize(L, buf, w, h, bands, apart * bands, out_w, out_h)
            want = pillow_planes(view, out_w, out_h)
            assert (got == want).all(), differs(what, a, out_w, out_h, got, want)
            assert (got == device_resize(L, a, w, h, bands, 0, out_w, out_h)).all(), what + ": differs from the packed call"
            # a stride of exactly a row behaves as 0 does
            exact = device_resize(L, a, w, h, bands, w * bands, out_w, out_h)
            assert (exact == want).all(), differs(what + " (stride = width * bands)", a, out_w, out_h, exact, want)
    a = rr.picture(80, 72, mode, "noise")
    buf, view = strided(a, 100 * bands, seed=3)
    packed = scan_scene(L, a, 80, 72, bands, 0, (64, 48), 64, True)
    got = scan_scene(L, buf, 80, 72, bands, 100 * bands, (64, 48), 64, True)
    assert (got == packed).all(), (mode, "scan_scene with a row stride: windows differing", int((got != packed).any(axis=1).sum()))
    assert (scan_scene(L, a, 80, 72, bands, 80 * bands, (64, 48), 64, True) == packed).all(), (mode, "stride = width * bands")
    assert (packed == gs.scene_by_windows(L, a, (64, 48), 64, True)).all(), mode


# ---- (c) scan_scene through the vertical-first resize -----------------------------------------------------------------------
def check_scene(L, a, sizes, what):
    """all 64 raw scores and the classes equal classify_windows on Pillow's level pictures"""
    h, w = a.shape[:2]
    bands = 1 if a.ndim == 2 else 3
    got = scan_scene(L, a, w, h, bands, 0, sizes, 64, True)
    want = gs.scene_by_windows(L, a, sizes, 64, True)
    bad = int((got != want).any(axis=1).sum())
    if bad:
        (lw, lh), = [scan_ref.level(w, h, s) for s in sizes[:1]]
        level = device_resize(L, a, w, h, bands, 0, lw, lh)
        pytest.fail("%s: %d of %d windows differ; the level picture: %s" % (what, bad, len(want), differs("level", a, lw, lh, level, pillow_planes(a, lw, lh))))
    assert (scan_scene(L, a, w, h, bands, 0, sizes, NCLS, False) == gs.scene_by_windows(L, a, sizes, NCLS, False)).all(), what
    return got


def test_scan_scene_takes_the_vertical_pass_first(L):
    """40 x 4001 blocks-plus-noise, RGB and L, size 40: level 32 x 3200, 793 windows, the vertical pass first; 40 x 4000, the
    horizontal-first side of the edge; size 48 (level 26 x 2667) is refused; then the 80 x 72 scene of test_gpu_scan.py
    gives what it gave before d_scan_tmp was sized by the other intermediate"""
    w, h = TALL
    small = np.random.default_rng(7).integers(0, 256, (72, 80, 3), dtype=np.uint8)
    first = scan_scene(L, small, 80, 72, 3, 0, (64, 48), 64, True)
    assert scan_ref.level(w, h, 40) == (32, 3200) and len(scan_ref.boxes(w, h, 40)) == 793
    assert rr.vertical_pass_first(w, h, 3200) and not rr.vertical_pass_first(w, h - 1, 3200)
    rgb = rr.blocks_plus_noise(w, h, "RGB", 11)
    check_scene(L, rgb, (40,), "40 x 4001 RGB")
    # two sizes in one call: 48 leaves a level 26 wide, which scan_ref.boxes refuses -- so must the library, whole call
    assert scan_ref.boxes(w, h, 48) is None
    sz = np.asarray((40, 48), np.int32)
    boxes = np.zeros((2 * 793, 4), np.int32)
    assert not L.bnn_mi355x_scan_scene(rgb.ctypes.data, w, h, 3, 0, sz.ctypes.data, 2, 64, boxes.ctypes.data, None, None, 1)
    assert "window size 48 leaves a level below 32 x 32 pixels" in gs.err(L), gs.err(L)
    check_scene(L, rr.blocks_plus_noise(w, h, "L", 13), (40,), "40 x 4001 L")
    check_scene(L, rr.blocks_plus_noise(w, h - 1, "RGB", 14), (40,), "40 x 4000 RGB (horizontal first)")
    again = scan_scene(L, small, 80, 72, 3, 0, (64, 48), 64, True)
    assert (again == first).all() and (again == gs.scene_by_windows(L, small, (64, 48), 64, True)).all()


# ---- (d) scan_clip through the same routes ------------------------------------------------------------------------------------
def clip_equals_scenes(L, clip, sizes, what):
    """every frame's 64 raw scores == scan_scene on that frame"""
    _, scores = gc.scan_clip(L, clip, sizes, 64, True)
    h, w = clip.shape[1:3]
    bands = 1 if clip.ndim == 3 else 3
    for f in range(len(clip)):
        want = scan_scene(L, np.ascontiguousarray(clip[f]), w, h, bands, 0, sizes, 64, True)
        bad = int((scores[f] != want).any(axis=1).sum())
        assert bad == 0, "%s: frame %d: %d of %d windows differ from scan_scene's" % (what, f, bad, len(want))
    return scores


def test_scan_clip_takes_the_vertical_pass_first(L):
    """two different 40 x 4001 RGB frames, size 40: every frame equals scan_scene (tied to Pillow above); the stage-0 map of
    frame 1 equals debug_scan_stage on Pillow's level planes of frame 1 -- the second frame's slice of the intermediate;
    two L frames likewise"""
    w, h = TALL
    clip = np.stack([rr.blocks_plus_noise(w, h, "RGB", 11), rr.blocks_plus_noise(w, h, "RGB", 12)])
    assert (clip[0] != clip[1]).any()
    clip_equals_scenes(L, clip, (40,), "2 x 40 x 4001 RGB")
    sz = np.asarray((40,), np.int32)
    off = np.zeros((2, 6), np.int64)
    assert L.bnn_mi355x_scan_clip_layout(w, h, sz.ctypes.data, 1, 2, None, None, off.ctypes.data, None, None, None) == 2, gs.err(L)
    total = scan_clip_ref.layout(w, h, (40,), 2)["stage_bytes"][0]
    out = np.zeros(total, np.uint8)
    assert L.bnn_mi355x_debug_scan_clip_stage(clip.ctypes.data, 2, 0, w, h, 3, 0, sz.ctypes.data, 1, 0, out.ctypes.data, out.nbytes) == total, gs.err(L)
    for f in (1, 0):
        want = gc.scan_stage(L, pillow_planes(clip[f], 32, 3200), 0)
        got = out[off[f, 0]:off[f, 0] + want.nbytes].view(np.uint32).reshape(want.shape)
        assert (got == want).all(), "stage 0 of frame %d: %d of %d words differ from the map of Pillow's level" % (f, int((got != want).sum()), want.size)
    grey = np.stack([rr.blocks_plus_noise(w, h, "L", 13), rr.blocks_plus_noise(w, h, "L", 15)])
    clip_equals_scenes(L, grey, (40,), "2 x 40 x 4001 L")


def test_scan_clip_rgb_strides(L):
    """three 80 x 72 RGB frames, rows 300 bytes apart, frames 300 * 72 + 24, random padding, sizes (64, 48): the packed
    clip's scores, which are scan_scene's per frame; then rows packed with frames apart, rows apart with frames packed"""
    sizes, w, h, frames = (64, 48), 80, 72, 3
    clip = gc.clip_of(frames, w, h, seed=21)
    want = clip_equals_scenes(L, clip, sizes, "3 x 80 x 72 RGB")
    assert (want[2] == gs.scene_by_windows(L, clip[2], sizes, 64, True)).all(), "frame 2 differs from classify_windows on Pillow's levels"
    row_stride, frame_stride = 300, 300 * h + 24
    buf = np.random.default_rng(5).integers(0, 256, frames * frame_stride, dtype=np.uint8)
    for f in range(frames):
        rows = buf[f * frame_stride:f * frame_stride + h * row_stride].reshape(h, row_stride)
        rows[:, :3 * w] = clip[f].reshape(h, 3 * w)
    shape = (frames, h, w, 3)
    got = gc.scan_clip(L, buf, sizes, 64, True, row_stride=row_stride, frame_stride=frame_stride, shape=shape)[1]
    assert (got == want).all(), ("rows and frames apart: windows differing", int((got != want).any(axis=2).sum()))
    apart = np.random.default_rng(6).integers(0, 256, (frames, 3 * w * h + 7), dtype=np.uint8)
    apart[:, :3 * w * h] = clip.reshape(frames, -1)
    got = gc.scan_clip(L, apart, sizes, 64, True, frame_stride=3 * w * h + 7, shape=shape)[1]
    assert (got == want).all(), ("rows packed, frames apart: windows differing", int((got != want).any(axis=2).sum()))
    rows = np.random.default_rng(7).integers(0, 256, (frames, h, row_stride), dtype=np.uint8)
    rows[:, :, :3 * w] = clip.reshape(frames, h, 3 * w)
    got = gc.scan_clip(L, rows, sizes, 64, True, row_stride=row_stride, shape=shape)[1]
    assert (got == want).all(), ("rows apart, frames packed: windows differing", int((got != want).any(axis=2).sum()))


def test_scan_clip_refuses_frames_too_narrow_to_scan(L):
    """two 16 x 1601 frames: refused by the plan, before anything is uploaded or launched -- the message is the plan's"""
    clip = np.zeros((2, 1601, 16, 3), np.uint8)
    sz = np.asarray((8,), np.int32)
    boxes = np.full((16, 4), -1, np.int32)
    assert not L.bnn_mi355x_scan_clip(clip.ctypes.data, 2, 0, 16, 1601, 3, 0, sz.ctypes.data, 1, NCLS, boxes.ctypes.data, None, None, 0)
    assert gs.err(L) == "scan_clip: need a picture of 32 x 32 pixels or more (got 16 x 1601)"
    assert (boxes == -1).all()
