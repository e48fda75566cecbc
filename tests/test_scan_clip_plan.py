"""CPU: the clip scan's host-only entry points (bnn_mi355x_scan_clip_layout, bnn_mi355x_scan_clip_capacity;
csrc/scan_clip.cpp) against the plain-Python restatement tests/scan_clip_ref.py, and every refusal of the four new entry
points that must come before anything touches a GPU.  No test here touches a GPU: dlopen of the product library needs
none, and the refused calls return before the first HIP call."""
import ctypes as C
import itertools
import re

import numpy as np
import pytest

import gpu_lib as gl
import scan_clip_ref as ref
import scan_ref

SIZES = (8, 32, 48, 64, 96)
SIZE_SETS = [(s,) for s in SIZES] + list(itertools.combinations(SIZES, 2))
FRAMES = (1, 2, 5)


@pytest.fixture(scope="module")
def L():
    return gl.load("cnvW1A1")


def err(L):
    return L.bnn_mi355x_last_error().decode()


def c_layout(L, w, h, sizes, frames):
    sz = np.asarray(sizes, np.int32)
    m = L.bnn_mi355x_scan_clip_layout(w, h, sz.ctypes.data, len(sz), frames, None, None, None, None, None, None)
    if m < 0:
        return None
    assert m == frames * len(sizes)
    mw, mh = np.full((m, 6), -1, np.int32), np.full((m, 6), -1, np.int32)
    off, first = np.full((m, 6), -1, np.int64), np.full(m, -1, np.int64)
    size, buf = np.full(m, -1, np.int32), np.full(2, -1, np.int64)
    assert L.bnn_mi355x_scan_clip_layout(w, h, sz.ctypes.data, len(sz), frames, mw.ctypes.data, mh.ctypes.data, off.ctypes.data, first.ctypes.data,
                                         size.ctypes.data, buf.ctypes.data) == m
    return {"w": mw, "h": mh, "off": off, "first": first, "size": size, "buf": tuple(int(b) for b in buf)}


def c_capacity(L, w, h, sizes):
    sz = np.asarray(sizes, np.int32)
    return L.bnn_mi355x_scan_clip_capacity(w, h, sz.ctypes.data, len(sz))


def check_layout(L, w, h, sizes, frames):
    want = ref.layout(w, h, sizes, frames) if ref.acceptable(w, h, sizes, frames) else None
    got = c_layout(L, w, h, sizes, frames)
    if want is None:
        assert got is None, (w, h, sizes, frames)
        return
    assert got is not None, (w, h, sizes, frames, err(L))
    assert got["buf"] == want["buf"], (w, h, sizes, frames)
    for m, (f, s, (nx, ny), first, off) in enumerate(want["maps"]):
        assert m == f * len(sizes) + sizes.index(s)
        assert got["size"][m] == s and got["first"][m] == first, (w, h, sizes, frames, m)
        assert [(int(a), int(b)) for a, b in zip(got["w"][m], got["h"][m])] == ref.stage_sizes(nx, ny), (w, h, sizes, frames, m)
        assert got["off"][m].tolist() == off, (w, h, sizes, frames, m)
    assert (got["off"][:, 5] == 32 * got["first"]).all()
    assert (got["off"] % 8 == 0).all()


def test_the_stated_limits_agree():
    with open(gl.ROOT + "/include/bnn_mi355x.h") as f:
        header = f.read()
    with open(gl.ROOT + "/bnn-pynq_amd/csrc/scan_clip.h") as f:
        model = f.read()
    stated = {k: int(re.search(r"#define BNN_MI355X_SCAN_CLIP_%s (\d+)" % k, header).group(1)) for k in ("MAX_FRAMES", "MAX_BYTES")}
    assert stated == {"MAX_FRAMES": ref.MAX_FRAMES, "MAX_BYTES": ref.MAX_CLIP_BYTES}
    assert int(re.search(r"constexpr int kScanClipMaxFrames = (\d+);", model).group(1)) == ref.MAX_FRAMES
    assert 1 << int(re.search(r"constexpr size_t kScanClipMaxBytes = \(size_t\)1 << (\d+);", model).group(1)) == ref.MAX_CLIP_BYTES
    assert int(re.search(r"constexpr int kScanClipBlock = (\d+);", model).group(1)) == ref.BLOCK


def test_layout_agrees_with_the_restatement(L):
    """every width and height in 32..80 with every size set (sizes singly and in pairs), the frame count going round
    (1, 2, 5); every frame count on a coarser grid"""
    for w in range(32, 81):
        for h in range(32, 81):
            for k, sizes in enumerate(SIZE_SETS):
                check_layout(L, w, h, sizes, FRAMES[(w + h + k) % 3])
    for w in range(32, 81, 7):
        for h in range(32, 81, 5):
            for sizes in SIZE_SETS:
                for frames in FRAMES:
                    check_layout(L, w, h, sizes, frames)


def test_layout_order_of_sizes_is_the_callers(L):
    """(96, 64) is not (64, 96): maps, first and offsets follow the order given"""
    a, b = c_layout(L, 200, 120, (64, 96), 2), c_layout(L, 200, 120, (96, 64), 2)
    assert a["size"].tolist() == [64, 96, 64, 96] and b["size"].tolist() == [96, 64, 96, 64]
    check_layout(L, 200, 120, (96, 64), 2)


def test_items_and_blocks_of_the_restatement():
    """100 x 52 with sizes (32, 40), the GPU tests' clip: levels 100 x 52 and 80 x 41, 108 and 39 windows; stage 0 has 4 900
    and 2 964 items; every stage has a map boundary that is no block boundary, and stage 5's maps are smaller than a block"""
    lv = ref.levels(100, 52, (32, 40))
    assert [(l, g) for _, l, g in lv] == [((100, 52), (18, 6)), ((80, 41), (13, 3))]
    assert ref.items(18, 6)[0] == 4900 and ref.items(13, 3)[0] == 2964
    for g in ((18, 6), (13, 3)):
        assert all(n % ref.BLOCK for n in ref.items(*g)), g
    assert ref.items(18, 6)[5] == 108 and ref.items(13, 3)[5] == 39
    lay = ref.layout(100, 52, (32, 40), 3)
    assert lay["windows"] == 3 * 147 and lay["blocks"][0] == 3 * (20 + 12) and lay["blocks"][5] == 6


def test_capacity_is_the_largest_accepted_clip(L):
    """F is accepted, F + 1 is refused; the restatement finds the same F by search"""
    for w, h, sizes in [(640, 480, (64, 96)), (64, 64, (32,)), (32, 32, (32,)), (1920, 1080, (64, 96)), (2048, 2048, (32,)), (8192, 8192, (8192,)),
                        (320, 240, (32, 64, 96)), (80, 72, (64, 48))]:
        cap = c_capacity(L, w, h, sizes)
        assert cap == ref.capacity(w, h, sizes) >= 1, (w, h, sizes, cap, err(L))
        assert c_layout(L, w, h, sizes, cap) is not None, (w, h, sizes, cap, err(L))
        assert c_layout(L, w, h, sizes, cap + 1) is None, (w, h, sizes, cap)
    assert c_capacity(L, 32, 32, (32,)) == 4096
    # 640 x 480 with (64, 96): 73 x 53 + 46 x 33 = 5 387 windows a frame; the map bytes bind (layer 0's maps: 870 912 bytes a frame)
    lay = ref.layout(640, 480, (64, 96), 1)
    assert lay["windows"] == 5387 and lay["buf"][0] == 870912
    assert c_capacity(L, 640, 480, (64, 96)) == scan_ref.MAX_MAP_BYTES // 870912 == 154
    got = c_layout(L, 640, 480, (64, 96), 154)
    assert got["first"][-1] + 46 * 33 == 154 * 5387


def test_capacity_refusals(L):
    assert c_capacity(L, 31, 40, (32,)) == 0 and "32 x 32 pixels or more" in err(L) and err(L).startswith("scan_clip_capacity: ")
    assert c_capacity(L, 64, 64, (72,)) == 0 and "level below 32 x 32" in err(L)
    assert c_capacity(L, 64, 64, (20,)) == 0 and "not a multiple of 8" in err(L)
    assert c_capacity(L, 4096, 4096, (32,)) == 0 and "bytes, more than the limit" in err(L)
    assert L.bnn_mi355x_scan_clip_capacity(64, 64, None, 1) == 0 and "null pointer" in err(L)
    one = np.array([32], np.int32)
    assert L.bnn_mi355x_scan_clip_capacity(64, 64, one.ctypes.data, 0) == 0 and "one window size or more" in err(L)
    assert ref.capacity(31, 40, (32,)) == ref.capacity(64, 64, (72,)) == ref.capacity(4096, 4096, (32,)) == 0


def test_refusals_come_before_the_gpu(L):
    """scan_clip / debug_scan_clip_stage / scan_clip_layout: bad frame counts, strides, bands, pointers, sizes, number_class
    and the three clip limits come back as NULL / -1 + last_error without a single HIP call (none could succeed on a machine
    without a GPU)"""
    px = np.zeros(2 * 3 * 80 * 72, np.uint8)
    one, bad = np.array([64], np.int32), np.array([64, 20], np.int32)
    boxes = np.zeros((64, 4), np.int32)

    def clip(pixels=px.ctypes.data, frames=2, fstride=0, w=80, h=72, bands=3, rstride=0, sizes=one.ctypes.data, n_sizes=1, ncls=10,
             out=boxes.ctypes.data):
        return L.bnn_mi355x_scan_clip(pixels, frames, fstride, w, h, bands, rstride, sizes, n_sizes, ncls, out, None, None, 0)

    for frames in (0, -1, 4097):
        assert not clip(frames=frames) and "need 1 to 4096 frames" in err(L) and err(L).startswith("scan_clip: "), err(L)
    assert not clip(fstride=3 * 80 * 72 - 1) and "frame stride shorter than a frame" in err(L)
    assert not clip(fstride=-5) and "frame stride shorter than a frame" in err(L)
    assert not clip(rstride=256, fstride=3 * 80 * 72) and "frame stride shorter than a frame" in err(L)  # a frame: 72 rows of 256 bytes
    assert not clip(rstride=239) and "row stride shorter than a row" in err(L)
    assert not clip(bands=4) and "bands must be 1 (L) or 3 (RGB)" in err(L)
    assert not clip(pixels=None) and "null pointer" in err(L)
    assert not clip(sizes=None) and "null pointer" in err(L)
    assert not clip(out=None) and "null pointer" in err(L)
    assert not clip(n_sizes=0) and "one window size or more" in err(L)
    assert not clip(sizes=bad.ctypes.data, n_sizes=2) and "window size 20 is not a multiple of 8" in err(L)
    assert not clip(w=40, h=40) and "level below 32 x 32" in err(L)
    assert not clip(w=31) and "32 x 32 pixels or more" in err(L)
    assert not clip(w=8193) and "limit of 8192 pixels a side" in err(L)
    for ncls in (0, 65):
        assert not clip(ncls=ncls) and "number_class" in err(L)
    # the clip's own limits (the refused calls read nothing: the small buffer stands in for the clip)
    s32, s8192 = np.array([32], np.int32), np.array([8192], np.int32)
    assert not clip(frames=5, w=2048, h=2048, sizes=s32.ctypes.data) and "1275125 windows, more than the limit of 1048576" in err(L)
    sz = np.array([64, 96], np.int32)
    assert not clip(frames=155, w=640, h=480, sizes=sz.ctypes.data, n_sizes=2) and "bytes in one buffer, more than the limit of 134217728" in err(L)
    assert not clip(frames=6, w=8192, h=8192, sizes=s8192.ctypes.data) and "bytes, more than the limit of 1073741824" in err(L)
    assert ref.acceptable(8192, 8192, (8192,), 5) and not ref.acceptable(8192, 8192, (8192,), 6) and ref.acceptable(8192, 8192, (8192,), 6, bands=1)
    assert not ref.acceptable(2048, 2048, (32,), 5) and not ref.acceptable(640, 480, (64, 96), 155)

    out = np.zeros(16, np.uint8)

    def dbg(stage=0, cap=out.size, frames=2, o=out.ctypes.data, pixels=px.ctypes.data):
        return L.bnn_mi355x_debug_scan_clip_stage(pixels, frames, 0, 80, 72, 3, 0, one.ctypes.data, 1, stage, o, cap)

    assert dbg(stage=6) == -1 and "bad arguments" in err(L)
    assert dbg(stage=-1) == -1 and "bad arguments" in err(L)
    assert dbg(o=None) == -1 and "bad arguments" in err(L)
    assert dbg(pixels=None) == -1 and "null pointer" in err(L)
    assert dbg(frames=0) == -1 and "need 1 to 4096 frames" in err(L) and err(L).startswith("debug_scan_clip_stage: ")
    # 80 x 72 at size 64: the level is 40 x 36 (3 x 2 windows), its layer-0 map 38 x 34 pixels of 8 bytes, two frames
    assert dbg() == -1 and "take %d bytes" % (2 * 38 * 34 * 8) in err(L), err(L)
    assert L.bnn_mi355x_scan_clip_layout(80, 72, one.ctypes.data, 1, 0, None, None, None, None, None, None) == -1 and "need 1 to 4096 frames" in err(L)
    assert L.bnn_mi355x_scan_clip_layout(80, 72, None, 1, 1, None, None, None, None, None, None) == -1 and "null pointer" in err(L)


@pytest.mark.parametrize("network, what", [("cnvW1A2", "built for cnvW1A1 only"), ("cnvW2A2", "built for cnvW1A1 only"),
                                           ("lfcW1A1", "CNV networks only"), ("lfcW1A2", "CNV networks only")])
def test_other_networks_refuse(network, what):
    lib = gl.load(network)
    px = np.zeros(3 * 40 * 40, np.uint8)
    one = np.array([32], np.int32)
    boxes = np.zeros((64, 4), np.int32)
    calls = [lambda: -1 if not lib.bnn_mi355x_scan_clip(px.ctypes.data, 1, 0, 40, 40, 3, 0, one.ctypes.data, 1, 10, boxes.ctypes.data, None, None, 0) else 0,
             lambda: lib.bnn_mi355x_scan_clip_capacity(40, 40, one.ctypes.data, 1),
             lambda: lib.bnn_mi355x_scan_clip_layout(40, 40, one.ctypes.data, 1, 1, None, None, None, None, None, None),
             lambda: lib.bnn_mi355x_debug_scan_clip_stage(px.ctypes.data, 1, 0, 40, 40, 3, 0, one.ctypes.data, 1, 0, boxes.ctypes.data, boxes.nbytes)]
    for call in calls:
        assert call() == -1
        assert what in lib.bnn_mi355x_last_error().decode()
