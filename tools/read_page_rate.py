#!/usr/bin/env python3
"""What the mask costs or saves on the way from a frame to what it says: tools/find_glyphs_rate.py's 640 x 480 RGB frames
of drawn digits, lfcW1A1 mnist, with ONE glyph and with 64 glyphs.  Two routes alternate in one process:
  A  read_glyphs(order="raster"): the yardstick, code this tool's change did not touch -- upload, enhance, the labelling
     launches, the component list's round trip, k_glyph_bbox, the ink boxes' round trip, k_glyph_record, the pass
  B  read_page(mask=True): the same up to the component list's round trip, then the line order on the host, one upload of
     descriptors, keys and tables, k_page_record (4 more bytes read per tap: the pixel's label), the pass -- one launch and
     one host round trip fewer
Every call's wall time is written out, then the medians and the ranges; likewise the device time between the call's
events (everything before the pass, and the pass) and the labelling launches alone (bnn_mi355x_last_find_usec).  The
classes of the two routes are asserted equal in every call for every glyph whose box overlaps no other box (inside an
overlap the two routes are MEANT to differ).  No figure is fixed in advance.  The record goes to
profiles/r26_read_page_rate.txt.
usage: read_page_rate.py [rounds [record.txt]]"""
import contextlib
import io
import os
import statistics
import sys
import time

import numpy as np
import torch  # noqa: F401  (HIP runtime order)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bnn-pynq_amd"))
from PIL import Image, ImageDraw, ImageFont  # noqa: E402
import bnn  # noqa: E402


@contextlib.contextmanager
def quiet():
    """the entry points of the reference's API report their rate on stdout, from Python and from C: not in the record"""
    sys.stdout.flush()
    keep = os.dup(1)
    null = os.open(os.devnull, os.O_WRONLY)
    os.dup2(null, 1)
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            yield
    finally:
        os.dup2(keep, 1)
        os.close(null)
        os.close(keep)


rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
record = sys.argv[2] if len(sys.argv) > 2 else None
with quiet():
    clf = bnn.LfcClassifier(bnn.NETWORK_LFCW1A1, "mnist", bnn.RUNTIME_SW)


def frame(cols, rows):
    """cols x rows digits on an off-white 640 x 480 sheet (tools/find_glyphs_rate.py's frame)"""
    img = Image.new("RGB", (640, 480), (240, 238, 232))
    d = ImageDraw.Draw(img)
    cw, ch = 640 // cols, 480 // rows
    font = ImageFont.load_default(size=int(0.7 * min(cw, ch)))
    for j in range(rows):
        for i in range(cols):
            d.text((cw * i + cw // 4, ch * j + ch // 10), "0123456789"[(3 * i + 7 * j) % 10], font=font, fill=(20, 20, 35))
    img.load()
    return img


def device_times(n):
    n = max(n, 1)
    return clf.usecPreprocess * n / 1e3, clf.usecPerImage * n / 1e3, clf.bnn.interface.bnn_mi355x_last_find_usec() / 1e3


def route_a(img):
    t0 = time.perf_counter()
    classes, boxes = clf.read_glyphs(img, order="raster")
    wall = 1e3 * (time.perf_counter() - t0)
    return (classes, boxes, wall) + device_times(len(boxes))


def route_b(img):
    t0 = time.perf_counter()
    classes, boxes, lines, _ = clf.read_page(img, mask=True)
    wall = 1e3 * (time.perf_counter() - t0)
    return (classes, boxes, wall) + device_times(len(boxes)) + (lines,)


def apart(boxes):
    """the boxes that overlap no other box"""
    b = np.asarray(boxes)
    keep = []
    for i, (l, u, r, lo) in enumerate(b):
        others = np.delete(b, i, axis=0)
        if not ((others[:, 0] < r) & (others[:, 2] > l) & (others[:, 1] < lo) & (others[:, 3] > u)).any():
            keep.append(tuple(int(v) for v in b[i]))
    return keep


def by_box(classes, boxes):
    return {tuple(int(v) for v in b): int(c) for c, b in zip(classes, boxes)}


def line(name, v):
    return "%-58s median %8.3f  min %8.3f  max %8.3f  (x%.3f)  calls: %s" % (name, statistics.median(v), min(v), max(v), max(v) / min(v),
                                                                             " ".join("%.3f" % x for x in v))


out = ["lfcW1A1 mnist, a 640 x 480 RGB frame of drawn digits whose boxes are not given; ms per call, %d alternations in one process after "
       "one untimed call of each route" % rounds]
for cols, rows in ((1, 1), (8, 8)):
    img = frame(cols, rows)
    ref = route_a(img)  # once each, untimed: buffers, tables, the pass's workspaces
    got = route_b(img)
    want, mine = by_box(ref[0], ref[1]), by_box(got[0], got[1])
    assert sorted(want) == sorted(mine), (ref[1], got[1])  # the same glyphs, whatever the order
    free = apart(ref[1])
    a, b = [[] for _ in range(4)], [[] for _ in range(4)]
    for _ in range(rounds):
        r = route_a(img)
        assert by_box(r[0], r[1]) == want
        for k in range(4):
            a[k].append(r[2 + k])
        r = route_b(img)
        assert by_box(r[0], r[1]) == mine and all(mine[box] == want[box] for box in free)
        for k in range(4):
            b[k].append(r[2 + k])
    n = len(ref[0])
    out.append("-- %d glyph%s found by both routes in %d line%s, %d of them overlap no other box: their classes are equal in every call; "
               "%d glyph%s of different class under the mask"
               % (n, "" if n == 1 else "s", len(set(got[6].tolist())), "" if len(set(got[6].tolist())) == 1 else "s", len(free),
                  sum(mine[k] != want[k] for k in want), "" if sum(mine[k] != want[k] for k in want) == 1 else "s"))
    for name, v in (("A: read_glyphs", a), ("B: read_page, mask = 1", b)):
        out.append(line(name + ", wall", v[0]))
        out.append(line("  device time up to the pass (upload .. records, trips)", v[1]))
        out.append(line("  device time, the pass", v[2]))
        out.append(line("  device time, the labelling launches alone", v[3]))
    spread = max(a[0]) - min(a[0])
    diff = statistics.median(b[0]) - statistics.median(a[0])
    out.append("  median B - median A = %+.3f ms wall; the yardstick's own spread (max - min of A) = %.3f ms: %s"
               % (diff, spread, "B is slower than A by more than A's spread" if diff > spread else
                  "B is faster than A by more than A's spread" if -diff > spread else "the difference is within A's spread"))
    spread = max(a[1]) - min(a[1])
    diff = statistics.median(b[1]) - statistics.median(a[1])
    out.append("  the same for the device time up to the pass: %+.3f ms, spread of A %.3f ms" % (diff, spread))
text = "\n".join(out) + "\n"
sys.stdout.write(text)
if record:
    with open(record, "w") as f:
        f.write(text)
