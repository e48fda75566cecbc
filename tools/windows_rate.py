#!/usr/bin/env python3
"""Locate objects in a scene (CNV-BNN_Road-Signs.ipynb cells 13-16): the 640 x 480 street picture, the notebook's 1 330
windows, cnvW1A1 road-signs.  The crops' route -- classify_images([im.crop(b) for b in boxes]): one upload and two or
three launches per window, the records back to the host, a temporary file, the file path -- alternates in one process
with classify_windows (one upload of the picture, one launch per window size, the pass on records that stay in HBM).
Each run reports wall time and the two device times (preprocess per window: classify_windows only; the classification
pass: both), best of three plus the spread, and asserts that the classes are equal.  The record goes to
profiles/r23_windows_rate.txt.  usage: windows_rate.py [rounds]"""
import contextlib
import io
import os
import sys
import time

import numpy as np
import torch  # noqa: F401  (HIP runtime order)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bnn-pynq_amd"))
from PIL import Image  # noqa: E402
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


rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 3
with quiet():
    clf = bnn.CnvClassifier(bnn.NETWORK_CNVW1A1, "road-signs", bnn.RUNTIME_SW)
im = Image.open(os.path.join(ROOT, "tests", "golden", "street_with_stop.jpg")).convert("RGB")
im.load()
boxes = clf.tile_boxes(im.size)
n = len(boxes)
assert im.size == (640, 480) and n == 1330


def crops_route():
    """cells 13-14 as this project serves them without classify_windows; the crops are part of the route"""
    t0 = time.perf_counter()
    crops = [im.crop(b) for b in boxes]
    t1 = time.perf_counter()
    with quiet():
        classes = clf.classify_images(crops)
    t2 = time.perf_counter()
    return np.asarray(classes), 1e3 * (t2 - t0), 1e3 * (t1 - t0), clf.usecPerImage * n / 1e3


def windows_route():
    t0 = time.perf_counter()
    classes = clf.classify_windows(im, boxes)
    t1 = time.perf_counter()
    return np.asarray(classes), 1e3 * (t1 - t0), clf.usecPreprocess * n / 1e3, clf.usecPerImage * n / 1e3


def spread(v):
    return "best %8.3f (x%.3f: %s)" % (min(v), max(v) / min(v), " ".join("%.3f" % x for x in v))


# once each, untimed: buffers, coefficient tables, the pass's workspaces
ref, _, _, _ = crops_route()
got, _, _, _ = windows_route()
assert (ref == got).all()
a_wall, a_crop, a_pass, b_wall, b_pre, b_pass = [], [], [], [], [], []
for _ in range(rounds):
    c, wall, crop, dev = crops_route()
    assert (c == ref).all()
    a_wall.append(wall); a_crop.append(crop); a_pass.append(dev)
    c, wall, pre, dev = windows_route()
    assert (c == ref).all()
    b_wall.append(wall); b_pre.append(pre); b_pass.append(dev)
print("cnvW1A1 road-signs, street_with_stop.jpg 640 x 480 RGB, %d windows (962 of 64, 368 of 96); ms per call, %d alternations in one "
      "process after one untimed call each; classes equal in every call" % (n, rounds))
print("classify_images(crops):  wall             %s" % spread(a_wall))
print("                         of which im.crop %s" % spread(a_crop))
print("                         device, the pass %s   (uploads and resample kernels are not timed on this route)" % spread(a_pass))
print("classify_windows:        wall             %s" % spread(b_wall))
print("                         device, upload + window kernels %s" % spread(b_pre))
print("                         device, the pass %s" % spread(b_pass))
print("wall: classify_windows x%.3f of classify_images(crops) (best of %d each); the yardstick's own spread x%.3f"
      % (min(b_wall) / min(a_wall), rounds, max(a_wall) / min(a_wall)))
hits = [b for b, c in zip(boxes, ref) if c == 14]
print("class 14 (%s): %d windows" % (clf.classes[14], len(hits)))
