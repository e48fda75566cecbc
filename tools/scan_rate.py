#!/usr/bin/env python3
"""Scan a scene densely: the 640 x 480 street picture, window sizes (64, 96), cnvW1A1 road-signs.  The yardstick is the
route a user has without the scan, given the SAME windows: Pillow resizes the picture to each level (320 x 240, 213 x 160)
and classify_windows classifies every 32 x 32 window of the level at stride 4 (one record per window, the nine-layer pass
on each).  It alternates in one process with scan_scene (one upload, per level the device resize and ONE pass of layers
0-5 over the whole level, layers 6-8 on its cells).  Each call reports wall time and the device times the entry points
return; medians and ranges of seven alternations after one untimed call each, classes asserted equal in every call.  The
record goes to profiles/r27_scan_rate.txt.  usage: scan_rate.py [rounds]"""
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
from PIL import Image  # noqa: E402
import bnn  # noqa: E402

SIZES = (64, 96)


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
with quiet():
    clf = bnn.CnvClassifier(bnn.NETWORK_CNVW1A1, "road-signs", bnn.RUNTIME_SW)
im = Image.open(os.path.join(ROOT, "tests", "golden", "street_with_stop.jpg")).convert("RGB")
im.load()
assert im.size == (640, 480)
levels = [clf.scan_boxes(im.size, s) for s in SIZES]
counts = [len(b) for _, b in levels]
n = sum(counts)
# a level's windows in the level's own coordinates: 32 x 32 boxes at stride 4
level_boxes = [np.array([(4 * i, 4 * j, 4 * i + 32, 4 * j + 32) for j in range((lh - 32) // 4 + 1) for i in range((lw - 32) // 4 + 1)], np.int32)
               for (lw, lh), _ in levels]


def windows_route():
    """Pillow's level pictures, classify_windows on each"""
    t0 = time.perf_counter()
    pics = [im.resize(lv, Image.LANCZOS) for lv, _ in levels]
    t1 = time.perf_counter()
    classes, pre, dev = [], 0.0, 0.0
    for pic, b in zip(pics, level_boxes):
        classes.append(np.asarray(clf.classify_windows(pic, b)))
        pre += clf.usecPreprocess * len(b) / 1e3
        dev += clf.usecPerImage * len(b) / 1e3
    t2 = time.perf_counter()
    return np.concatenate(classes), 1e3 * (t2 - t0), 1e3 * (t1 - t0), pre, dev


def scan_route():
    t0 = time.perf_counter()
    _, classes = clf.scan_scene(im, SIZES)
    t1 = time.perf_counter()
    return np.asarray(classes), 1e3 * (t1 - t0), clf.usecPreprocess * n / 1e3, clf.usecPerImage * n / 1e3


def spread(v):
    return "median %8.3f  range %8.3f .. %8.3f  (%s)" % (statistics.median(v), min(v), max(v), " ".join("%.3f" % x for x in v))


# once each, untimed: buffers, coefficient tables, the workspaces
ref = windows_route()[0]
got = scan_route()[0]
assert ref.shape == got.shape == (n,) and (ref == got).all()
a_wall, a_pil, a_pre, a_pass, b_wall, b_pre, b_pass = [], [], [], [], [], [], []
for _ in range(rounds):
    c, wall, pil, pre, dev = windows_route()
    assert (c == ref).all()
    a_wall.append(wall); a_pil.append(pil); a_pre.append(pre); a_pass.append(dev)
    c, wall, pre, dev = scan_route()
    assert (c == ref).all()
    b_wall.append(wall); b_pre.append(pre); b_pass.append(dev)
print("cnvW1A1 road-signs, street_with_stop.jpg 640 x 480 RGB, sizes %s: levels %s, %d windows (%s); ms per call, %d alternations in one "
      "process after one untimed call each; classes equal in every call"
      % (SIZES, " ".join("%d x %d" % lv for lv, _ in levels), n, " + ".join(str(c) for c in counts), rounds))
print("Pillow levels + classify_windows:  wall                              %s" % spread(a_wall))
print("                                   of which Image.resize (host)      %s" % spread(a_pil))
print("                                   device, upload + window kernels   %s" % spread(a_pre))
print("                                   device, the per-window pass       %s" % spread(a_pass))
print("scan_scene:                        wall                              %s" % spread(b_wall))
print("                                   device, upload + resizes          %s" % spread(b_pre))
print("                                   device, the scans                 %s" % spread(b_pass))
ya, yb = statistics.median(a_wall), statistics.median(b_wall)
print("wall, medians: scan_scene x%.3f of the yardstick; the yardstick's own spread x%.3f (max / min of its %d calls)"
      % (yb / ya, max(a_wall) / min(a_wall), rounds))
da, db = statistics.median(a_pass), statistics.median(b_pass)
print("device, medians: the scans x%.3f of the per-window pass on the same windows; its own spread x%.3f"
      % (db / da, max(a_pass) / min(a_pass)))
print("class 14 (%s): %d windows" % (clf.classes[14], int((ref == 14).sum())))
