#!/usr/bin/env python3
"""The two forms of the clip scan's stages 1-3: F frames of the 640 x 480 street picture (frame f is the picture rolled by
4 f columns), window sizes (64, 96), cnvW1A1 road-signs, F = 1, 4, 16 and 64.  The yardstick is form 0, the integer
kernels (k_clip_quad); it alternates in one process with form 1, the matrix cores (k_clip_conv_mfma), ONE scan_clip call
each on the same frames.  Each form reports the wall time of the call and the device time the entry point returns
(usecPerImage times the windows: the six stage launches with layers 6-8 and the decode behind them, between two events);
medians and ranges of seven alternations after one untimed call each, scores asserted equal in every call.  The record
goes to profiles/r33_scan_form_rate.txt.  usage: scan_form_rate.py [rounds]"""
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


def route(clip, form):
    clf.scan_form(form)
    assert clf.scan_matrix_stages(n * len(clip)) == (0b1110 if form else 0)
    t0 = time.perf_counter()
    _, scores = clf.scan_clip(clip, SIZES, details=True)
    t1 = time.perf_counter()
    return np.asarray(scores), 1e3 * (t1 - t0), clf.usecPerImage * n * len(clip) / 1e3


def spread(v):
    return "median %9.3f  range %9.3f .. %9.3f  (%s)" % (statistics.median(v), min(v), max(v), " ".join("%.3f" % x for x in v))


print("cnvW1A1 road-signs, street_with_stop.jpg 640 x 480 RGB rolled by 4 f columns, sizes %s: %d windows a frame; ms per scan_clip call, %d "
      "alternations in one process after one untimed call each; scores equal in every call" % (SIZES, n, rounds))
was = clf.scan_form()
for frames in CLIPS:
    clip = np.ascontiguousarray(np.stack([np.roll(picture, 4 * f, axis=1) for f in range(frames)]))
    ref = route(clip, 0)[0]  # once each, untimed
    assert (route(clip, 1)[0] == ref).all()
    wall, dev = {0: [], 1: []}, {0: [], 1: []}
    for r in range(rounds):
        for form in ((0, 1) if r % 2 == 0 else (1, 0)):  # the order swaps every round: neither form always runs behind the other
            s, w, d = route(clip, form)
            assert (s == ref).all()
            wall[form].append(w); dev[form].append(d)
    print("F = %d (%d windows)" % (frames, frames * n))
    for form, name in ((0, "form 0, integer pipe:"), (1, "form 1, matrix cores:")):
        print("  %-22s wall                %s" % (name, spread(wall[form])))
        print("  %-22s device, the stages  %s" % ("", spread(dev[form])))
    for what, v in (("wall", wall), ("device (stages)", dev)):
        print("  %s, medians: form 1 x%.3f of form 0; form 0's own spread x%.3f (max / min of its %d repeats)"
              % (what, statistics.median(v[1]) / statistics.median(v[0]), max(v[0]) / min(v[0]), rounds))
clf.scan_form(was)
