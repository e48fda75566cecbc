#!/usr/bin/env python3
"""What reading a clip in one call costs or saves against the route a user has today: tools/find_glyphs_rate.py's 640 x 480
RGB frames of drawn digits, lfcW1A1 mnist, with ONE glyph and with 64 glyphs a frame, clips of F = 1 / 4 / 16 / 54 frames (54
is the pixel limit at this size).  Two routes alternate in one process:
  A  a loop of F read_page(mask=True) calls: the yardstick, code this tool's change did not touch -- per frame an upload,
     about ten launches, the component list's round trip, the record kernel, an LFC pass on that frame's glyphs
  B  ONE read_clip(mask=True) call: one upload of the clip as a tall plane, luma and enhance with a mean per frame, the tile
     labelling in LDS, its seams, flatten, collect, ONE round trip, ONE record launch, ONE LFC pass for all frames' glyphs
Every round's wall time is written out, then the medians and the ranges; likewise the sum of the labelling launches' device
time (bnn_mi355x_last_find_usec: per frame in A, once in B).  The classes, boxes and lines of the two routes are asserted equal
in every call.  A gain is claimed only where it lies outside A's own spread; no figure is fixed in advance.  The record goes to
profiles/r37_read_clip_rate.txt.
usage: read_clip_rate.py [rounds [record.txt]]"""
import os
import statistics
import sys
import time

import numpy as np
import torch  # noqa: F401  (HIP runtime order)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bnn-pynq_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from PIL import Image, ImageDraw, ImageFont  # noqa: E402
import bnn  # noqa: E402

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
record = sys.argv[2] if len(sys.argv) > 2 else None
clf = bnn.LfcClassifier(bnn.NETWORK_LFCW1A1, "mnist", bnn.RUNTIME_SW)
find_usec = clf.bnn.interface.bnn_mi355x_last_find_usec


def frame(cols, rows, shift):
    """cols x rows digits on an off-white 640 x 480 sheet (tools/find_glyphs_rate.py's frame; `shift` turns the digits)"""
    img = Image.new("RGB", (640, 480), (240, 238, 232))
    d = ImageDraw.Draw(img)
    cw, ch = 640 // cols, 480 // rows
    font = ImageFont.load_default(size=int(0.7 * min(cw, ch)))
    for j in range(rows):
        for i in range(cols):
            d.text((cw * i + cw // 4, ch * j + ch // 10), "0123456789"[(3 * i + 7 * j + shift) % 10], font=font, fill=(20, 20, 35))
    return np.asarray(img)


def route_a(clip):
    t0 = time.perf_counter()
    out, labelling = [], 0.0
    for a in clip:
        out.append(clf.read_page(a, mask=True))
        labelling += find_usec()
    return out, 1e3 * (time.perf_counter() - t0), labelling / 1e3


def route_b(clip):
    t0 = time.perf_counter()
    out = clf.read_clip(clip, mask=True)
    return out, 1e3 * (time.perf_counter() - t0), find_usec() / 1e3


def same(a, b):
    return len(a) == len(b) and all(x.tolist() == y.tolist() for fa, fb in zip(a, b) for x, y in zip(fa, fb))


def line(name, v):
    return "%-46s median %8.3f  min %8.3f  max %8.3f  (x%.3f)  rounds: %s" % (name, statistics.median(v), min(v), max(v), max(v) / min(v),
                                                                              " ".join("%.3f" % x for x in v))


def verdict(a, b):
    spread, diff = max(a) - min(a), statistics.median(b) - statistics.median(a)
    return "median B - median A = %+.3f ms (A / B = x%.2f); the yardstick's own spread (max - min of A) = %.3f ms: %s" % (
        diff, statistics.median(a) / statistics.median(b), spread,
        "B is faster than A by more than A's spread" if -diff > spread else
        "B is slower than A by more than A's spread" if diff > spread else "within A's spread: not established")


out = ["lfcW1A1 mnist, clips of F 640 x 480 RGB frames of drawn digits; ms per clip, %d alternations in one process after one untimed "
       "round of each route; A: a loop of F read_page(mask=True) calls, B: one read_clip(mask=True) call" % rounds]
devnull = open(os.devnull, "w")
for cols, rows in ((1, 1), (8, 8)):
    for n_frames in (1, 4, 16, 54):
        clip = np.stack([frame(cols, rows, f) for f in range(n_frames)])
        stdout, sys.stdout = sys.stdout, devnull  # (the reference's API reports its rate on stdout: not in the record)
        try:
            want = route_a(clip)[0]  # once each, untimed: buffers, tables, the pass's workspaces
            assert same(route_b(clip)[0], want)
            a, b = ([], []), ([], [])
            for _ in range(rounds):
                for route, v in ((route_a, a), (route_b, b)):
                    got, wall, labelling = route(clip)
                    assert same(got, want)
                    v[0].append(wall)
                    v[1].append(labelling)
        finally:
            sys.stdout = stdout
        out.append("-- F = %d, %d glyph%s a frame (%d in all): classes, boxes, lines and gaps equal in every call" % (
            n_frames, len(want[0][0]), "" if len(want[0][0]) == 1 else "s", sum(len(f[0]) for f in want)))
        out.append(line("A: F x read_page, wall", a[0]))
        out.append(line("B: read_clip, wall", b[0]))
        out.append("  " + verdict(a[0], b[0]))
        out.append(line("A: sum of the labelling launches, device", a[1]))
        out.append(line("B: the labelling launches, device", b[1]))
        out.append("  " + verdict(a[1], b[1]))
out.append("Not measured: other frame sizes, dense noise, the chars net, mask = 0, the tile labelling against the per-pixel merge at equal "
           "launch counts.")
text = "\n".join(out) + "\n"
sys.stdout.write(text)
if record:
    with open(record, "w") as f:
        f.write(text)
