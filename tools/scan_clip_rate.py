#!/usr/bin/env python3
"""Scan a clip: F frames of the 640 x 480 street picture (frame f is the picture rolled by 4 f columns), window sizes
(64, 96), cnvW1A1 road-signs, F = 1, 4, 16 and 64.  The yardstick is the route a user has without the clip entry point:
F calls of scan_scene (per call one upload, per level the device resize, six stage launches, layers 6-8 and the decode).
It alternates in one process with ONE scan_clip call on the same frames (one upload, per level one pair of resize launches
for all frames, six stage launches over all maps, layers 6-8 and the decode once).  Each route reports wall time and the
device times the entry points return (usecPreprocess and usecPerImage times the windows); medians and ranges of seven
alternations after one untimed call each, classes asserted equal in every call.  The record goes to
profiles/r29_scan_clip_rate.txt.  usage: scan_clip_rate.py [rounds]"""
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
CLIPS = (1, 4, 16, 64)


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
picture = np.asarray(im)
n = sum(len(clf.scan_boxes(im.size, s)[1]) for s in SIZES)


def scenes_route(clip):
    """F calls of scan_scene"""
    classes, pre, dev = [], 0.0, 0.0
    t0 = time.perf_counter()
    for frame in clip:
        classes.append(clf.scan_scene(frame, SIZES)[1])
        pre += clf.usecPreprocess * n / 1e3
        dev += clf.usecPerImage * n / 1e3
    t1 = time.perf_counter()
    return np.stack(classes), 1e3 * (t1 - t0), pre, dev


def clip_route(clip):
    t0 = time.perf_counter()
    _, classes = clf.scan_clip(clip, SIZES)
    t1 = time.perf_counter()
    return np.asarray(classes), 1e3 * (t1 - t0), clf.usecPreprocess * n * len(clip) / 1e3, clf.usecPerImage * n * len(clip) / 1e3


def spread(v):
    return "median %9.3f  range %9.3f .. %9.3f  (%s)" % (statistics.median(v), min(v), max(v), " ".join("%.3f" % x for x in v))


print("cnvW1A1 road-signs, street_with_stop.jpg 640 x 480 RGB rolled by 4 f columns, sizes %s: %d windows a frame; ms per clip, %d alternations "
      "in one process after one untimed call each; classes equal in every call" % (SIZES, n, rounds))
for frames in CLIPS:
    clip = np.ascontiguousarray(np.stack([np.roll(picture, 4 * f, axis=1) for f in range(frames)]))
    # once each, untimed: buffers, coefficient tables, the workspaces
    ref = scenes_route(clip)[0]
    got = clip_route(clip)[0]
    assert ref.shape == got.shape == (frames, n) and (ref == got).all()
    a_wall, a_pre, a_pass, b_wall, b_pre, b_pass = [], [], [], [], [], []
    for _ in range(rounds):
        c, wall, pre, dev = scenes_route(clip)
        assert (c == ref).all()
        a_wall.append(wall); a_pre.append(pre); a_pass.append(dev)
        c, wall, pre, dev = clip_route(clip)
        assert (c == ref).all()
        b_wall.append(wall); b_pre.append(pre); b_pass.append(dev)
    print("F = %d (%d windows)" % (frames, frames * n))
    print("  %2d x scan_scene:  wall                      %s" % (frames, spread(a_wall)))
    print("                    device, upload + resizes  %s" % spread(a_pre))
    print("                    device, the scans         %s" % spread(a_pass))
    print("  1 x scan_clip:    wall                      %s" % spread(b_wall))
    print("                    device, upload + resizes  %s" % spread(b_pre))
    print("                    device, the stages        %s" % spread(b_pass))
    ya, yb = statistics.median(a_wall), statistics.median(b_wall)
    da, db = statistics.median(a_pass), statistics.median(b_pass)
    print("  wall, medians: scan_clip x%.3f of the yardstick; the yardstick's own spread x%.3f (max / min of its %d repeats)"
          % (yb / ya, max(a_wall) / min(a_wall), rounds))
    print("  device (scans / stages), medians: scan_clip x%.3f of the yardstick; the yardstick's own spread x%.3f"
          % (db / da, max(a_pass) / min(a_pass)))
    print("  class 14 (%s): %s windows per frame" % (clf.classes[14], " ".join(str(int((r == 14).sum())) for r in ref[:8]) + (" ..." if frames > 8 else "")))
