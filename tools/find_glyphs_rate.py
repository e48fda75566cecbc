#!/usr/bin/env python3
"""From a frame to what it says on the LFC networks: a 640 x 480 RGB frame of drawn digits, lfcW1A1 mnist, with ONE glyph
and with 64 glyphs, whose boxes nobody hands over.  Two routes alternate in one process:
  A  what a caller had before find_glyphs: enhance() (upload, the plane comes back), scipy.ndimage.label + find_objects
     on the host (the numpy column split where scipy is absent: the record says which), then classify_glyphs() (the same
     frame uploaded and enhanced again)
  B  read_glyphs(): one upload, the labelling launches, the component list's round trip, the records and the pass
Every call's wall time is written out, then the medians and the spread; the classes (and boxes) of the two routes are
asserted equal in every call.  Then the device time of the labelling launches alone (ink words .. compacted list,
bnn_mi355x_last_find_usec) at reach (1, 1) and (4, 16).  No ratio is fixed in advance.  The record goes to
profiles/r25_find_glyphs_rate.txt.
usage: find_glyphs_rate.py [rounds [record.txt]]"""
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

try:
    from scipy import ndimage
    HOST_LABELLING = "scipy.ndimage.label + find_objects (3 x 3 structure)"
except ImportError:
    ndimage = None
    HOST_LABELLING = "the numpy column split (scipy is absent): one line of glyphs only"


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
    """cols x rows digits on an off-white 640 x 480 sheet (tools/glyph_front_rate.py's frame, without its boxes)"""
    img = Image.new("RGB", (640, 480), (240, 238, 232))
    d = ImageDraw.Draw(img)
    cw, ch = 640 // cols, 480 // rows
    font = ImageFont.load_default(size=int(0.7 * min(cw, ch)))
    for j in range(rows):
        for i in range(cols):
            d.text((cw * i + cw // 4, ch * j + ch // 10), "0123456789"[(3 * i + 7 * j) % 10], font=font, fill=(20, 20, 35))
    img.load()
    return img


def host_boxes(plane):
    """raster order of the first pixel, as read_glyphs(order="raster") returns them"""
    if ndimage is not None:
        lab, _ = ndimage.label(plane != 255, structure=np.ones((3, 3)))
        return [(s[1].start, s[0].start, s[1].stop, s[0].stop) for s in ndimage.find_objects(lab)]
    ink_columns = (plane != 255).any(axis=0)
    edges = np.flatnonzero(np.diff(np.concatenate([[0], ink_columns.astype(np.int8), [0]])))
    boxes = []
    for a, b in zip(edges[::2], edges[1::2]):
        rows = np.flatnonzero((plane[:, a:b] != 255).any(axis=1))
        boxes.append((int(a), int(rows[0]), int(b), int(rows[-1]) + 1))
    return boxes


def route_a(img):
    t0 = time.perf_counter()
    plane = np.asarray(clf.enhance(img))
    boxes = host_boxes(plane)
    classes = np.asarray(clf.classify_glyphs(img, boxes)) if boxes else np.zeros(0, np.int32)
    return classes, np.asarray(boxes, np.int32).reshape(-1, 4), 1e3 * (time.perf_counter() - t0)


def route_b(img):
    t0 = time.perf_counter()
    classes, boxes = clf.read_glyphs(img, order="raster")
    wall = 1e3 * (time.perf_counter() - t0)
    n = max(len(boxes), 1)
    return classes, boxes, wall, clf.usecPreprocess * n / 1e3, clf.usecPerImage * n / 1e3, clf.bnn.interface.bnn_mi355x_last_find_usec() / 1e3


def line(name, v):
    return "%-58s median %8.3f  min %8.3f  max %8.3f  (x%.3f)  calls: %s" % (name, statistics.median(v), min(v), max(v), max(v) / min(v),
                                                                             " ".join("%.3f" % x for x in v))


out = ["lfcW1A1 mnist, a 640 x 480 RGB frame of drawn digits whose boxes are not given; ms per call, %d alternations in one process after "
       "one untimed call of each route; host labelling of route A: %s" % (rounds, HOST_LABELLING)]
for cols, rows in ((1, 1), (8, 8)):
    img = frame(cols, rows)
    ref, ref_boxes, _ = route_a(img)  # once each, untimed: buffers, tables, the pass's workspaces
    got = route_b(img)
    if ndimage is not None:
        assert np.array_equal(ref_boxes, got[1]), (ref_boxes, got[1])
    assert np.array_equal(ref, got[0]), (ref, got[0])
    a_wall, b_wall, b_pre, b_pass, b_label = [], [], [], [], []
    for _ in range(rounds):
        c, _, wall = route_a(img)
        assert np.array_equal(c, ref)
        a_wall.append(wall)
        c, _, wall, pre, dev, lab = route_b(img)
        assert np.array_equal(c, ref)
        b_wall.append(wall); b_pre.append(pre); b_pass.append(dev); b_label.append(lab)
    n = len(ref)
    out.append("-- %d glyph%s found by both routes, classes equal in every call (%s)" % (n, "" if n == 1 else "s", " ".join(str(int(c)) for c in ref)))
    out.append(line("A: enhance + host labelling + classify_glyphs, wall", a_wall))
    out.append(line("B: read_glyphs, wall", b_wall))
    out.append(line("  B device time, upload + labelling + glyph kernels + trips", b_pre))
    out.append(line("  B device time, the labelling launches alone, reach (1, 1)", b_label))
    out.append(line("  B device time, the pass", b_pass))
    spread = max(max(a_wall) - min(a_wall), max(b_wall) - min(b_wall))
    gain = statistics.median(a_wall) - statistics.median(b_wall)
    out.append("  median A - median B = %.3f ms; largest spread between repeats of either route = %.3f ms: %s"
               % (gain, spread, "B is faster by more than the spread" if gain > spread else "the difference is within the spread"))
    far = []
    for _ in range(rounds):
        clf.find_glyphs(img, reach=(4, 16), order="raster")
        far.append(clf.bnn.interface.bnn_mi355x_last_find_usec() / 1e3)
    out.append(line("  find_glyphs, the labelling launches alone, reach (4, 16)", far) + "  (%d glyphs at that reach)" % clf.glyphs_found)
text = "\n".join(out) + "\n"
sys.stdout.write(text)
if record:
    with open(record, "w") as f:
        f.write(text)
