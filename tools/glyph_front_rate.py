#!/usr/bin/env python3
"""From a picture to classes on the LFC networks (LFC-BNN_MNIST_Webcam.ipynb cells 9-15): a 640 x 480 RGB frame of drawn
digits, lfcW1A1 mnist, with ONE box (the notebook's case: the whole frame holds one digit) and with 64 boxes.  Two
routes alternate in one process:
  host:    the notebook's cells in Pillow per box (tests/glyph_ref.py), an idx file, classify_mnists
  device:  classify_glyphs (one upload of the frame, four kernels, one host round trip for the ink boxes, the pass on
           records that stay in HBM)
Every call's wall time is written out, then the medians and the spread; the classes of the two routes are asserted equal
in every call.  No ratio is fixed in advance.  The record goes to profiles/r24_glyph_front_rate.txt.
usage: glyph_front_rate.py [rounds [record.txt]]"""
import contextlib
import io
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch  # noqa: F401  (HIP runtime order)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bnn-pynq_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from PIL import Image, ImageDraw, ImageFont  # noqa: E402
import bnn  # noqa: E402
import glyph_ref  # noqa: E402


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
    """cols x rows digits on an off-white 640 x 480 sheet and the grid's boxes"""
    img = Image.new("RGB", (640, 480), (240, 238, 232))
    d = ImageDraw.Draw(img)
    cw, ch = 640 // cols, 480 // rows
    font = ImageFont.load_default(size=int(0.7 * min(cw, ch)))
    boxes = []
    for j in range(rows):
        for i in range(cols):
            d.text((cw * i + cw // 4, ch * j + ch // 10), "0123456789"[(3 * i + 7 * j) % 10], font=font, fill=(20, 20, 35))
            boxes.append((cw * i, ch * j, cw * (i + 1), ch * (j + 1)))
    img.load()
    return img, boxes


def host_route(img, boxes):
    t0 = time.perf_counter()
    recs, _, status = glyph_ref.glyphs(img, boxes)
    with tempfile.NamedTemporaryFile() as tmp:
        tmp.write(glyph_ref.idx_file(recs))
        tmp.flush()
        with quiet():
            classes = np.asarray(clf.classify_mnists(tmp.name))
    classes[status == 2] = -1
    return classes, 1e3 * (time.perf_counter() - t0)


def device_route(img, boxes):
    t0 = time.perf_counter()
    classes = np.asarray(clf.classify_glyphs(img, boxes))
    wall = 1e3 * (time.perf_counter() - t0)
    return classes, wall, clf.usecPreprocess * len(boxes) / 1e3, clf.usecPerImage * len(boxes) / 1e3


def line(name, v):
    return "%-44s median %8.3f  min %8.3f  max %8.3f  (x%.3f)  calls: %s" % (name, statistics.median(v), min(v), max(v), max(v) / min(v),
                                                                             " ".join("%.3f" % x for x in v))


out = ["lfcW1A1 mnist, a 640 x 480 RGB frame of drawn digits; ms per call, %d alternations in one process after one untimed call of each "
       "route; classes of the two routes equal in every call" % rounds]
for cols, rows in ((1, 1), (8, 8)):
    img, boxes = frame(cols, rows)
    n = len(boxes)
    ref, _ = host_route(img, boxes)  # once each, untimed: buffers, tables, the pass's workspaces
    got = device_route(img, boxes)[0]
    assert (ref == got).all(), (ref, got)
    h_wall, d_wall, d_pre, d_pass = [], [], [], []
    for _ in range(rounds):
        c, wall = host_route(img, boxes)
        assert (c == ref).all()
        h_wall.append(wall)
        c, wall, pre, dev = device_route(img, boxes)
        assert (c == ref).all()
        d_wall.append(wall); d_pre.append(pre); d_pass.append(dev)
    out.append("-- %d box%s (classes %s)" % (n, "" if n == 1 else "es", " ".join(str(int(c)) for c in ref)))
    out.append(line("host: glyph_ref + idx file + classify_mnists, wall", h_wall))
    out.append(line("device: classify_glyphs, wall", d_wall))
    out.append(line("  device time, upload + glyph kernels + round trip", d_pre))
    out.append(line("  device time, the pass", d_pass))
text = "\n".join(out) + "\n"
sys.stdout.write(text)
if record:
    with open(record, "w") as f:
        f.write(text)
