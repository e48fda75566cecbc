"""The oracle of the find_glyphs tests: connected components of the ink of an L plane in plain Python and numpy, apart
from csrc/components.cpp (the model: csrc/components.h).  The pixel pairs of the forward half-neighbourhood that are both
ink are collected with array slicing; a union-find runs over the pairs; filter, order and cap as the model states them.

Also the pictures both test files use (CASES): the smallest shapes where a labelling kernel goes wrong."""
import ctypes
import functools

import numpy as np

DEFAULTS = dict(ink_level=255, reach=(1, 1), min_pixels=1, order=0, cap=1 << 20)


def forward_offsets(rx, ry):
    """(dx, dy) of the forward half: the same row to the right, then the rows below from -rx to rx"""
    return [(dx, 0) for dx in range(1, rx + 1)] + [(dx, dy) for dy in range(1, ry + 1) for dx in range(-rx, rx + 1)]


def label(plane, ink_level=255, reach=(1, 1), min_pixels=1, order=0, cap=1 << 20):
    """-> (boxes int32 [n, 4], pixel counts int32 [n], total, labels int32 [H, W]) with n = min(cap, total)"""
    plane = np.asarray(plane)
    h, w = plane.shape
    ink = plane < ink_level
    idx = np.arange(h * w, dtype=np.int64).reshape(h, w)
    parent = list(range(h * w))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    for dx, dy in forward_offsets(*reach):
        if dy >= h or abs(dx) >= w:
            continue
        ys, yd = slice(0, h - dy), slice(dy, h)
        xs, xd = (slice(0, w - dx), slice(dx, w)) if dx >= 0 else (slice(-dx, w), slice(0, w + dx))
        both = ink[ys, xs] & ink[yd, xd]
        for a, b in zip(idx[ys, xs][both].tolist(), idx[yd, xd][both].tolist()):
            a, b = find(a), find(b)
            if a < b:
                parent[b] = a
            elif b < a:
                parent[a] = b
    flat_ink = ink.reshape(-1)
    root = np.full(h * w, -1, np.int64)
    for p in np.flatnonzero(flat_ink).tolist():
        root[p] = find(p)
    comps = []  # (first, left, upper, right, lower, pixels)
    firsts, inverse, counts = np.unique(root[flat_ink], return_inverse=True, return_counts=True)
    py, px = np.nonzero(ink)
    for k, first in enumerate(firsts.tolist()):
        m = inverse == k
        comps.append((first, int(px[m].min()), int(py[m].min()), int(px[m].max()) + 1, int(py[m].max()) + 1, int(counts[k])))
    comps = [c for c in comps if c[5] >= min_pixels]
    comps.sort(key=(lambda c: (c[1], c[2], c[0])) if order == 1 else (lambda c: c[0]))
    total = len(comps)
    comps = comps[:cap]
    index = {c[0]: k for k, c in enumerate(comps)}
    labels = np.array([index.get(r, -1) for r in root.tolist()], np.int32).reshape(h, w)
    boxes = np.array([c[1:5] for c in comps], np.int32).reshape(-1, 4)
    pixels = np.array([c[5] for c in comps], np.int32)
    return boxes, pixels, total, labels


# ---- the pictures: 0 is ink, 255 is background --------------------------------------------------------------------
def blank(w, h):
    return np.full((h, w), 255, np.uint8)


def with_ink(w, h, points):
    a = blank(w, h)
    for x, y in points:
        a[y, x] = 0
    return a


def edge_columns(w, h=5):
    """ink in column 0 and in the last column: the 16-byte lane, the 64-bit ink word, the padding"""
    a = blank(w, h)
    a[::2, 0] = 0
    a[1::2, w - 1] = 0
    a[h - 1, w - 1] = 0
    return a


def dashes(w, h):
    a = blank(w, h).reshape(-1)
    a[np.arange(w * h) % 7 < 4] = 0
    return a.reshape(h, w)


def diagonal(n, anti):
    a = blank(n, n)
    i = np.arange(n)
    a[i, (n - 1 - i) if anti else i] = 0
    return a


def cross(w, h):
    a = blank(w, h)
    a[h // 2, :] = 0
    a[:, w // 2] = 0
    return a


def spiral(n):
    """a one-pixel-wide rectangular spiral with one-pixel gaps: one component, a chain of thousands of joins"""
    a = blank(n, n)
    x0, y0, x1, y1 = 0, 0, n - 1, n - 1
    a[y0, x0:x1 + 1] = 0
    while True:
        a[y0:y1 + 1, x1] = 0                      # down the right side
        if x1 - x0 < 2: break
        a[y1, x0:x1 + 1] = 0                      # along the bottom, leftwards
        y0 += 2
        if y1 - y0 < 0: break
        a[y0:y1 + 1, x0] = 0                      # up the left side
        x1 -= 2
        if x1 - x0 < 2: break
        a[y0, x0:x1 + 1] = 0                      # along the top, rightwards
        y1 -= 2
        x0 += 2
        if y1 - y0 < 0 or x1 - x0 < 0: break
    return a


def serpentine(w, h):
    a = blank(w, h)
    a[::2, :] = 0
    for k, y in enumerate(range(1, h, 2)):
        a[y, (w - 1) if k % 2 == 0 else 0] = 0
    return a


def comb(w, h, joined_at_top):
    a = blank(w, h)
    a[:, ::2] = 0
    a[:, 1::2] = 255
    if joined_at_top:
        a[0, :] = 0
    else:
        a[h - 1, :] = 0
    return a


def two_combs(w, h):
    """teeth of one comb hang from the top row, those of the other stand on the bottom row, between them: never touching"""
    a = blank(w, h)
    a[0, :] = 0
    a[:h - 2, 0::4] = 0
    a[h - 1, :] = 0
    a[2:, 2::4] = 0
    return a


def rings(n, step=3):
    """concentric one-pixel square rings, two background pixels apart"""
    a = blank(n, n)
    k = 0
    while 2 * k < n:
        lo, hi = k, n - 1 - k
        a[lo, lo:hi + 1] = 0; a[hi, lo:hi + 1] = 0; a[lo:hi + 1, lo] = 0; a[lo:hi + 1, hi] = 0
        k += step
    return a


def noise(w, h, density, seed):
    return np.where(np.random.default_rng(seed).random((h, w)) < density, 0, 255).astype(np.uint8)


def blobs():
    """blobs of 1 .. 5 pixels"""
    a = blank(40, 12)
    for k in range(5):
        a[3, 4 + 7 * k:4 + 7 * k + k + 1] = 0
    a[8, 30] = 0
    return a


def same_left():
    """two components with the same left edge, the lower one first in raster order of neither: ties go by upper; and one
    further left that comes later in raster order"""
    a = blank(30, 20)
    a[2, 10:14] = 0
    a[9, 10:12] = 0
    a[5, 20:25] = 0
    a[15, 3:6] = 0
    return a


def grid(n):
    """isolated pixels on every second row and column: n * n / 4 components"""
    a = blank(n, n)
    a[::2, ::2] = 0
    return a


def ramp(w=64, h=8):
    return (np.arange(w * h) * 255 // (w * h - 1)).astype(np.uint8).reshape(h, w)[:, ::-1].copy()


def pair_pictures(reach):
    """two single pixels at dx = reach_x, reach_x + 1 and dy = reach_y, reach_y + 1 (and on the axes, and to the lower
    left), in the interior and against each border: joined exactly when within reach -> [(name, picture, joined)]"""
    rx, ry = reach
    w, h = 3 * rx + 40, 3 * ry + 30
    out = []
    for dx, dy in [(rx, ry), (rx + 1, ry), (rx, ry + 1), (rx + 1, ry + 1), (rx, 0), (rx + 1, 0), (0, ry), (0, ry + 1), (-rx, ry), (-rx - 1, ry)]:
        ax, bx = (0, dx) if dx >= 0 else (-dx, 0)
        spots = {"interior": (w // 2 - 3, h // 2 - 2), "upper left": (0, 0), "lower right": (w - 1 - max(ax, bx), h - 1 - dy),
                 "upper right": (w - 1 - max(ax, bx), 0), "lower left": (0, h - 1 - dy)}
        for where, (ox, oy) in spots.items():
            pic = with_ink(w, h, [(ox + ax, oy), (ox + bx, oy + dy)])
            out.append(("%s dx %d dy %d" % (where, dx, dy), pic, abs(dx) <= rx and abs(dy) <= ry))
    return out


def _cases():
    c = []

    def add(name, picture, **kw):
        c.append((name, picture, kw))

    add("1x1 ink", with_ink(1, 1, [(0, 0)]))
    add("1x1 blank", blank(1, 1))
    add("200x1", dashes(200, 1))
    add("1x200", dashes(1, 200))
    for w in (15, 16, 17, 63, 64, 65, 129):
        add("edge columns %d" % w, edge_columns(w))
    add("blank", blank(200, 160))
    add("all ink", np.zeros((160, 200), np.uint8))
    add("diagonal", diagonal(200, False))
    add("anti-diagonal", diagonal(200, True))
    add("cross", cross(200, 160))
    add("spiral", spiral(96))
    add("serpentine", serpentine(131, 67))
    add("comb joined at the bottom", comb(200, 160, False))
    add("comb joined at the top", comb(200, 160, True))
    add("two combs", two_combs(201, 70))
    add("rings", rings(200))
    for density in (0.05, 0.2, 0.4, 0.45, 0.6):
        for seed in (1, 2):
            add("noise %.2f seed %d" % (density, seed), noise(160, 200, density, seed))
    add("noise reach (3, 2)", noise(160, 200, 0.05, 3), reach=(3, 2))
    add("noise reach (16, 16)", noise(64, 48, 0.01, 4), reach=(16, 16))
    add("dense noise reach (16, 16)", noise(64, 48, 0.3, 5), reach=(16, 16))
    for m in (1, 3, 6):
        add("blobs min_pixels %d" % m, blobs(), min_pixels=m)
    for order in (0, 1):
        add("same left order %d" % order, same_left(), order=order)
        add("noise order %d cap 7" % order, noise(90, 70, 0.1, 6), order=order, cap=7, min_pixels=2)
    add("grid 64 cap 10", grid(64), cap=10)
    add("grid 64 cap 10 left", grid(64), cap=10, order=1)
    add("grid 128 cap 4096", grid(128), cap=4096)
    add("grid 130: more components than come back in the first copy", grid(130), order=1)
    add("cap 1", noise(50, 40, 0.2, 7), cap=1)
    for level in (1, 128, 254, 255):
        add("ramp ink_level %d" % level, ramp(), ink_level=level)
    return c


CASES = _cases()
CASE_IDS = [name for name, _, _ in CASES]


@functools.lru_cache(maxsize=None)
def expected(i):
    """the oracle's answer for CASES[i], computed once and shared; callers leave it unchanged"""
    _, picture, kw = CASES[i]
    return label(picture, **dict(DEFAULTS, **kw))


# ---- what both test files do with an answer -----------------------------------------------------------------------------
def find_host(lib, plane, ink_level=255, reach=(1, 1), min_pixels=1, order=0, cap=1 << 20, stride=0, width=None, null_find=False,
              want_labels=True, want_counts=True):
    h = plane.shape[0]
    w = plane.shape[1] if width is None else width
    n = min(cap, (w + 1) // 2 * ((h + 1) // 2))
    boxes = np.full((max(n, 1), 4), -7, np.int32)
    counts = np.full(max(n, 1), -7, np.int32)
    labels = np.full((h, w), -7, np.int32)
    from bnn import abi
    f = abi.FindOpts(ink_level, reach[0], reach[1], min_pixels, order)
    total = lib.bnn_mi355x_find_glyphs_host(plane.ctypes.data, w, h, stride, None if null_find else ctypes.byref(f), boxes.ctypes.data,
                                            counts.ctypes.data if want_counts else None, labels.ctypes.data if want_labels else None, cap)
    assert total >= 0, lib.bnn_mi355x_last_error().decode()
    k = min(total, cap)
    assert (boxes[k:] == -7).all() and (counts[k:] == -7).all()  # nothing is written past what is returned
    return boxes[:k], counts[:k], total, labels


def same(got, want, what):
    assert got[2] == want[2], (what, "total", got[2], want[2])
    assert np.array_equal(got[0], want[0]), (what, "boxes")
    assert np.array_equal(got[1], want[1]), (what, "pixel counts")
    assert np.array_equal(got[3], want[3]), (what, "labels: first differing pixel", int(np.argmax(got[3].reshape(-1) != want[3].reshape(-1))))
