#!/usr/bin/env python3
"""The fine clip scan against the route it replaces: F frames of the 640 x 480 street picture (frame f is the picture rolled
by 4 f columns), window size 32, cnvW1A1 road-signs, F = 1, 4, 16 and 64, automatic forms.  ONE scan_clip(stride=2) of the
clip alternates in one process with the yardstick, four scan_clip calls on the clip cropped by (0, 0), (2, 0), (0, 2) and
(2, 2), the order swapping every round.  Each route reports the wall time and the device time the entry points return
(usecPerImage times the windows: the stage launches with layers 6-8 and the decode behind them, between two events); medians
and ranges of seven rounds after one untimed call each, scores asserted equal in every call.  A clip longer than one call
accepts goes in several calls on either route (CnvClassifier.scan_clip cuts it), which the record states.  First the share
of layer-3 conv outputs the bands of k_clip_conv_phase evaluate twice, counted from its band constants.  The record is
profiles/r36_scan_fine_rate.txt.  usage: scan_fine_rate.py [rounds]
With `trace` behind the rounds nothing is timed: ROUNDS bnn_mi355x_scan_clip_fine calls on 15 frames (the most one call
takes: 16 pass the window limit) and ROUNDS x 4 scan_clip calls on the cropped frames, for a kernel trace of its own
(rocprofv3 --kernel-trace --stats -- python tools/scan_fine_rate.py 6 trace), whose per-launch times of the stage-2 and
stage-3 kernels of either route stand behind the rate table."""
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

SIZES = (32,)
CLIPS = (1, 4, 16, 64)
CROPS = ((0, 0), (1, 0), (0, 1), (1, 1))  # (px, py) in result order


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
lib = clf.bnn.interface
im = Image.open(os.path.join(ROOT, "tests", "golden", "street_with_stop.jpg")).convert("RGB")
im.load()
assert im.size == (640, 480)
picture = np.asarray(im)
n_fine = len(clf.scan_fine_boxes(im.size, 32)[1])


def fine(clip):
    t0 = time.perf_counter()
    _, scores = clf.scan_clip(clip, SIZES, details=True, stride=2)
    t1 = time.perf_counter()
    return np.asarray(scores), 1e3 * (t1 - t0), clf.usecPerImage * scores.shape[0] * scores.shape[1] / 1e3


def four_calls(crops):
    parts, dev = [], 0.0
    t0 = time.perf_counter()
    for c in crops:
        _, s = clf.scan_clip(c, SIZES, details=True)
        parts.append(np.asarray(s))
        dev += clf.usecPerImage * s.shape[0] * s.shape[1] / 1e3
    t1 = time.perf_counter()
    return np.concatenate(parts, axis=1), 1e3 * (t1 - t0), dev


def spread(v):
    return "median %9.3f  range %9.3f .. %9.3f  (%s)" % (statistics.median(v), min(v), max(v), " ".join("%.3f" % x for x in v))


sz = np.asarray(SIZES, np.int32)
if sys.argv[2:] == ["trace"]:
    clip = np.ascontiguousarray(np.stack([np.roll(picture, 4 * f, axis=1) for f in range(15)]))
    crops = [np.ascontiguousarray(clip[:, 2 * py:, 2 * px:]) for px, py in CROPS]
    boxes = np.zeros((n_fine, 4), np.int32)
    for r in range(rounds):
        p = lib.bnn_mi355x_scan_clip_fine(clip.ctypes.data, 15, 0, 640, 480, 3, 0, sz.ctypes.data, 1, 64, boxes.ctypes.data, None, None, 1)
        assert p, lib.bnn_mi355x_last_error()
        got = np.ctypeslib.as_array(p, shape=(15, n_fine, 64)).copy()
        lib.free_results(p)
        with quiet():
            assert (got[:, :, :len(clf.classes)] == four_calls(crops)[0]).all()
    sys.exit(0)
cap = lib.bnn_mi355x_scan_clip_capacity(640, 480, sz.ctypes.data, 1)
# the halo of stage 3, from the band constants of csrc/scan_fine.h: bands of 16 rows x 63 columns, 15 rows and 62 columns apart
cw, ch = (640 - 32) // 2 + 1 + 9, (480 - 32) // 2 + 1 + 9
computed = sum(min(16, ch - y) * min(63, cw - x) for y in range(0, ch - 1, 15) for x in range(0, cw - 1, 62))
print("layer-3 convolution of a 640 x 480 level: %d x %d = %d outputs; the bands of k_clip_conv_phase<4, 4, true> evaluate %d (+%.1f %%)"
      % (cw, ch, cw * ch, computed, 100.0 * computed / (cw * ch) - 100))
print("cnvW1A1 road-signs, street_with_stop.jpg 640 x 480 RGB rolled by 4 f columns, size 32, automatic forms: %d windows a frame at "
      "stride 2; ms, %d rounds of the two routes in one process after one untimed call each; scores equal in every call.  One scan_clip "
      "call takes %d frames and one fine call %d: longer clips go in several calls" % (n_fine, rounds, cap, max(1, cap // 4)))
for frames in CLIPS:
    clip = np.ascontiguousarray(np.stack([np.roll(picture, 4 * f, axis=1) for f in range(frames)]))
    crops = [np.ascontiguousarray(clip[:, 2 * py:, 2 * px:]) for px, py in CROPS]
    ref = four_calls(crops)[0]  # once each, untimed
    assert ref.shape[1] == n_fine and (fine(clip)[0] == ref).all()
    wall, dev = {0: [], 1: []}, {0: [], 1: []}
    for r in range(rounds):
        for route in ((0, 1), (1, 0))[r % 2]:
            s, w, d = fine(clip) if route else four_calls(crops)
            assert (s == ref).all()
            wall[route].append(w); dev[route].append(d)
    print("F = %d (%d windows)" % (frames, frames * n_fine))
    for route, name in ((0, "four scan_clip calls:"), (1, "scan_clip(stride=2):")):
        print("  %-22s wall                %s" % (name, spread(wall[route])))
        print("  %-22s device, the stages  %s" % ("", spread(dev[route])))
    for what, v in (("wall", wall), ("device (stages)", dev)):
        ratio, own = statistics.median(v[1]) / statistics.median(v[0]), max(v[0]) / min(v[0])
        print("  %s, medians: fine x%.3f of the four calls; the four calls' own spread x%.3f (max / min of its %d repeats)%s"
              % (what, ratio, own, rounds, ": not established" if 1 / own <= ratio <= own else ""))

