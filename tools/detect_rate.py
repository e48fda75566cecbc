#!/usr/bin/env python3
"""Detect objects in a clip: the 640 x 480 street picture rolled by 4 f columns per frame, window sizes (64, 96), cnvW1A1
road-signs, class 14 above a score of 455 (CNV-BNN_Road-Signs.ipynb cell 16), IoU 0.5, at most 64 detections a frame.
The yardstick is what a user has without the detection kernels: scan_clip(details=True) -- every window's scores come
down and are widened on the host -- followed by the numpy model of tests/detect_ref.py; its two parts are timed
separately, and the scan_clip(details=True) call alone is a lower bound for ANY host route.  It alternates in one process
with one detect_clip call (the same launches, then the detection kernels; only the lists come down).  Each call reports
wall time; medians and ranges of seven alternations after one untimed call each, detections asserted equal in every call.
The record goes to profiles/r31_detect_rate.txt.  usage: detect_rate.py [rounds [F ...]]"""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
from PIL import Image  # noqa: E402
import bnn  # noqa: E402
import detect_ref  # noqa: E402

SIZES = (64, 96)
STOP, MIN_SCORE, IOU, MAX_DET, MAX_CANDIDATES = 14, 455, (32768, 65536), 64, 4096


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
frame_counts = [int(a) for a in sys.argv[2:]] or [1, 16, 64]
with quiet():
    clf = bnn.CnvClassifier(bnn.NETWORK_CNVW1A1, "road-signs", bnn.RUNTIME_SW)
im = np.asarray(Image.open(os.path.join(ROOT, "tests", "golden", "street_with_stop.jpg")).convert("RGB"))
assert im.shape == (480, 640, 3)
n = sum(len(clf.scan_boxes((640, 480), s)[1]) for s in SIZES)
ncls = len(clf.classes)


def host_route(clip):
    """scan_clip(details=True), then the numpy model -> (detections, wall ms, ms of the scan_clip call, ms of the model)"""
    t0 = time.perf_counter()
    boxes, scores = clf.scan_clip(clip, SIZES, details=True)
    t1 = time.perf_counter()
    dets, counts, ncand = detect_ref.detect(boxes, scores, 1 << STOP, 1, MIN_SCORE, IOU, MAX_CANDIDATES, MAX_DET)
    t2 = time.perf_counter()
    found = [[(tuple(int(v) for v in d[:4]), int(d[4]), int(d[5])) for d in dets[f, :counts[f]]] for f in range(len(counts))]
    return found, ncand.tolist(), 1e3 * (t2 - t0), 1e3 * (t1 - t0), 1e3 * (t2 - t1)


def device_route(clip):
    t0 = time.perf_counter()
    found = clf.detect_clip(clip, STOP, SIZES, min_score=MIN_SCORE, by_score=True, iou=IOU, max_det=MAX_DET, max_candidates=MAX_CANDIDATES)
    t1 = time.perf_counter()
    windows = n * len(clip)
    return found, list(clf.n_candidates), 1e3 * (t1 - t0), clf.usecPreprocess * windows / 1e3, clf.usecPerImage * windows / 1e3, clf.usecDetect * len(clip) / 1e3


def spread(v):
    return "median %8.3f  range %8.3f .. %8.3f  (%s)" % (statistics.median(v), min(v), max(v), " ".join("%.3f" % x for x in v))


print("cnvW1A1 road-signs, street_with_stop.jpg 640 x 480 RGB rolled by 4 f columns, sizes %s: %d windows a frame; class %d (%s) by score above %d, "
      "IoU %d / %d, max_det %d, max_candidates %d; ms per clip, %d alternations in one process after one untimed call each; detections equal in "
      "every call" % (SIZES, n, STOP, clf.classes[STOP], MIN_SCORE, IOU[0], IOU[1], MAX_DET, MAX_CANDIDATES, rounds))
for frames in frame_counts:
    clip = np.stack([np.roll(im, -4 * f, axis=1) for f in range(frames)])
    with quiet():  # once each, untimed: the workspaces
        ref, ref_cand = host_route(clip)[:2]
        got, got_cand = device_route(clip)[:2]
    assert ref == got and ref_cand == got_cand
    a_wall, a_scan, a_model, b_wall, b_pre, b_pass, b_det = [], [], [], [], [], [], []
    for _ in range(rounds):
        with quiet():
            found, cand, wall, scan, model = host_route(clip)
        assert found == ref and cand == ref_cand
        a_wall.append(wall); a_scan.append(scan); a_model.append(model)
        with quiet():
            found, cand, wall, pre, dev, det = device_route(clip)
        assert found == ref and cand == ref_cand
        b_wall.append(wall); b_pre.append(pre); b_pass.append(dev); b_det.append(det)
    print("F = %d (%d windows)" % (frames, n * frames))
    print("  scan_clip(details) + numpy model:  wall                       %s" % spread(a_wall))
    print("                                     of which scan_clip(details) %s" % spread(a_scan))
    print("                                     of which the numpy model    %s" % spread(a_model))
    print("  detect_clip:                       wall                       %s" % spread(b_wall))
    print("                                     device, upload + resizes   %s" % spread(b_pre))
    print("                                     device, the stages         %s" % spread(b_pass))
    print("                                     device, detection kernels  %s" % spread(b_det))
    print("  bytes downloaded: %d (scores, int16 x 64 a window) against %d (dets, counts, n_candidates)"
          % (frames * n * 64 * 2, frames * (MAX_DET * 8 + 2) * 4))
    ya, ys, yb = statistics.median(a_wall), statistics.median(a_scan), statistics.median(b_wall)
    print("  wall, medians: detect_clip x%.3f of the yardstick and x%.3f of its scan_clip(details) call alone; that call's own spread x%.3f, the "
          "yardstick's x%.3f (max / min of %d calls)" % (yb / ya, yb / ys, max(a_scan) / min(a_scan), max(a_wall) / min(a_wall), rounds))
    print("  candidates per frame: %s%s; detections per frame: %s%s" % (" ".join(str(c) for c in ref_cand[:8]), " ..." if frames > 8 else "",
                                                                        " ".join(str(len(d)) for d in ref[:8]), " ..." if frames > 8 else ""))
    print("  frame 0: %s" % ", ".join("%s score %d" % (b, s) for b, _, s in ref[0]))
