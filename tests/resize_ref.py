"""Pillow's 8-bit Image.resize(size, LANCZOS) in plain numpy, from its documented arithmetic (Resample.c of Pillow 12),
independently of csrc/resample.cpp and of the kernels.  It gives more than Pillow does: the pass order is an argument,
and every pass also returns the unclipped value (2^21 + sum) >> 22 of each of its samples, so that a test can say how
often clip8 worked and what the other order would have given.  Pinned to Pillow itself by tests/test_resize_ref.py.
Also here: the pictures and the table of cases that test_resize_ref.py and test_gpu_scan_resize.py share."""
import math

import numpy as np

PRECISION_BITS = 22


def _lanczos(x):
    if -3.0 <= x < 3.0:
        if x == 0.0:
            return 1.0
        a, b = x * math.pi, x / 3.0 * math.pi
        return math.sin(a) / a * (math.sin(b) / b)
    return 0.0


def coeffs(in_size, out_size):
    """[(xmin, [k ...])] per output sample: precompute_coeffs + normalize_coeffs_8bpc, the box being the whole axis"""
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 3.0 * filterscale
    ss = 1.0 / filterscale
    out = []
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [_lanczos((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        out.append((xmin, [int(v * (1 << PRECISION_BITS) + (0.5 if v >= 0 else -0.5)) for v in w]))
    return out


def _pass(a, axis, out_size):
    """one pass along `axis` of a [h, w, bands] uint8 array -> (uint8 result, int64 unclipped values)"""
    a = np.moveaxis(a, axis, 0).astype(np.int64)
    raw = np.empty((out_size,) + a.shape[1:], np.int64)
    for xx, (xmin, k) in enumerate(coeffs(a.shape[0], out_size)):
        ss = np.tensordot(np.asarray(k, np.int64), a[xmin:xmin + len(k)], axes=1) + (1 << (PRECISION_BITS - 1))
        assert np.abs(ss).max() < 2 ** 31  # Pillow sums in an int: no wrap happens, so none is restated
        raw[xx] = ss >> PRECISION_BITS
    raw = np.moveaxis(raw, 0, axis)
    return np.clip(raw, 0, 255).astype(np.uint8), raw


def vertical_pass_first(w, h, out_h):
    return h > 100 * w and out_h < h


def passes(a, out_w, out_h, vertical_first=None):
    """-> (result, [(axis name, unclipped values) of every pass that ran, in the order they ran]); a: uint8 [h, w] (L) or
    [h, w, 3] (RGB); vertical_first None: Pillow's own rule"""
    grey = a.ndim == 2
    cur = a[:, :, None] if grey else a
    h, w = cur.shape[:2]
    if vertical_first is None:
        vertical_first = vertical_pass_first(w, h, out_h)
    todo = [("v", 0, out_h, h), ("h", 1, out_w, w)] if vertical_first else [("h", 1, out_w, w), ("v", 0, out_h, h)]
    ran = []
    for name, axis, out_size, in_size in todo:
        if out_size == in_size:
            continue
        cur, raw = _pass(cur, axis, out_size)
        ran.append((name, raw[:, :, 0] if grey else raw))
    cur = np.ascontiguousarray(cur[:, :, 0] if grey else cur)
    return (cur.copy() if cur is a else cur), ran


def resize(a, out_w, out_h, vertical_first=None):
    return passes(a, out_w, out_h, vertical_first)[0]


def planes_of(r):
    """a resized picture as the scan's level planes [3, h, w] (L: the grey plane three times)"""
    return np.ascontiguousarray(np.broadcast_to(r[None], (3,) + r.shape) if r.ndim == 2 else r.transpose(2, 0, 1))


# ---- the pictures and the cases -------------------------------------------------------------------------------------------
def picture(w, h, mode, kind):
    """"noise": seeded uniform bytes; "blocks": the saturated checkerboard of test_image_to_cifar.py / test_gpu_windows.py
    (the Lanczos lobes overshoot at its edges, clip8 works at both ends)"""
    if kind == "noise":
        return np.random.default_rng(7000 * w + h + (1 if mode == "L" else 3)).integers(0, 256, (h, w) if mode == "L" else (h, w, 3), dtype=np.uint8)
    assert kind == "blocks"
    by, bx = max(h // 7, 1), max(w // 5, 1)
    yy, xx = np.mgrid[0:h, 0:w]
    base = (((yy // by) + (xx // bx)) % 2 * 255).astype(np.uint8)
    return np.ascontiguousarray(base if mode == "L" else np.stack([base, 255 - base, np.roll(base, bx // 2 + 1, axis=1)], axis=2))


def blocks_plus_noise(w, h, mode, seed):
    """the blocks picture with seeded noise of amplitude up to 40 added and clipped: windows differ, clip8 still works"""
    a = picture(w, h, mode, "blocks").astype(np.int32)
    n = np.random.default_rng(seed).integers(-40, 41, a.shape)
    return np.clip(a + n, 0, 255).astype(np.uint8)


# (w, h, out_w, out_h, route, marks): the routes of launch_scan_resize / launch_clip_resize; "order": the other pass order
# must differ (blocks, or noise where the mark says so), "clips": both ends of clip8 work in every pass (blocks)
CASES = [
    (80, 72, 40, 36, "both, horizontal first", ("order", "clips")),
    (80, 72, 40, 72, "horizontal only, shrink", ("clips",)),
    (80, 72, 100, 72, "horizontal only, enlarge", ("clips",)),
    (80, 72, 80, 36, "vertical only, shrink", ("clips",)),
    (80, 72, 80, 90, "vertical only, enlarge", ("clips",)),
    (40, 40, 97, 101, "both enlarge, odd sizes", ("order", "clips")),
    (3, 301, 2, 150, "vertical first, a few hundred bytes", ("order", "clips")),
    (16, 1601, 12, 400, "vertical first, factor 4", ("order", "clips")),
    (8, 800, 6, 600, "the edge h == 100 w, horizontal first", ("order-noise",)),
    (8, 801, 6, 600, "the edge, one row more, vertical first", ("order-noise",)),
    (640, 480, 80, 60, "49 taps, many blocks per launch", ("order", "clips")),
    (2, 300, 1, 7, "vertical first, one output column", ()),
    (300, 2, 7, 1, "one output row", ()),
    (1, 1, 3, 3, "one input sample", ()),
]
MODES = ("RGB", "L")
KINDS = ("noise", "blocks")
ORDER_MIN_BYTES = 100   # the opposite pass order changes at least this many bytes of an "order" case
CLIPS_MIN = 50          # samples below 0, and above 255, in every pass of a "clips" case


# 3 x 301 -> 2 x 150 carries its marks on the RGB picture alone: its L picture has 903 samples and 300 output bytes, of
# which the other order changes 40, and its first pass clips 18 samples at each end, its second none -- the thresholds
# above cannot be met there.  The L picture still goes to the device and must equal Pillow's.
MARKS_ON_RGB_ONLY = {(3, 301, 2, 150)}


def marked_modes(case):
    return ("RGB",) if case[:4] in MARKS_ON_RGB_ONLY else MODES


def case_id(case):
    return "%dx%d-%dx%d" % case[:4]


def order_kind(case):
    """the content on which the case's "order" mark holds, or None"""
    return "blocks" if "order" in case[5] else "noise" if "order-noise" in case[5] else None
