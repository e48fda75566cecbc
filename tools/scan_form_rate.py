#!/usr/bin/env python3
"""The three forms of the clip scan's stages 1-5: F frames of the 640 x 480 street picture (frame f is the picture rolled by
4 f columns), window sizes (64, 96), cnvW1A1 road-signs, F = 1, 4, 16 and 64.  Form 0, the integer kernels (k_clip_quad,
k_clip_vec), form 1, stages 1-3 on the matrix cores (k_clip_conv_mfma), and form 2, stages 4 and 5 there as well
(k_clip_tail_mfma), alternate in one process, ONE scan_clip call each on the same frames, the order rotating every
round.  Form 0 is form 1's yardstick and form 1, the fastest route before form 2, is form 2's.  Each form reports the wall
time of the call and the device time the entry point returns (usecPerImage times the windows: the six stage launches
with layers 6-8 and the decode behind them, between two events); medians and ranges of seven rounds after one untimed
call each, scores asserted equal in every call.  The records are profiles/r33_scan_form_rate.txt (forms 0 and 1) and
profiles/r34_scan_tail_rate.txt (all three).  usage: scan_form_rate.py [rounds]
With `l0` behind the rounds the forms of STAGE 0 alternate instead (scan_stage0_form 0, the integer kernel k_clip_conv0, which
is the yardstick, and 1, k_clip_conv0_mfma), stages 1-5 under form 2 throughout, the order swapping every round; the rest of
the protocol is the same.  Its record is profiles/r35_scan_l0_rate.txt.  usage: scan_form_rate.py ROUNDS l0"""
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
MASKS = {0: 0, 1: 0b1110, 2: 0b111110}
NAMES = ((0, "form 0, integer pipe:"), (1, "form 1, layers 1-3:"), (2, "form 2, layers 1-5:"))


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


def route(clip, form, l0=0):
    clf.scan_form(form)
    clf.scan_stage0_form(l0)
    assert clf.scan_matrix_stages(n * len(clip)) == MASKS[form] | l0
    t0 = time.perf_counter()
    _, scores = clf.scan_clip(clip, SIZES, details=True)
    t1 = time.perf_counter()
    return np.asarray(scores), 1e3 * (t1 - t0), clf.usecPerImage * n * len(clip) / 1e3


def spread(v):
    return "median %9.3f  range %9.3f .. %9.3f  (%s)" % (statistics.median(v), min(v), max(v), " ".join("%.3f" % x for x in v))


print("cnvW1A1 road-signs, street_with_stop.jpg 640 x 480 RGB rolled by 4 f columns, sizes %s: %d windows a frame; ms per scan_clip call, %d "
      "rounds of the %s in one process after one untimed call each; scores equal in every call"
      % (SIZES, n, rounds, "two forms of stage 0" if sys.argv[2:] == ["l0"] else "three forms"))
was, was0 = clf.scan_form(), clf.scan_stage0_form()
for frames in CLIPS if sys.argv[2:] == ["l0"] else ():
    clip = np.ascontiguousarray(np.stack([np.roll(picture, 4 * f, axis=1) for f in range(frames)]))
    ref = route(clip, 2, 0)[0]  # once each, untimed
    assert (route(clip, 2, 1)[0] == ref).all()
    wall, dev = {0: [], 1: []}, {0: [], 1: []}
    for r in range(rounds):
        for l0 in ((0, 1), (1, 0))[r % 2]:
            s, w, d = route(clip, 2, l0)
            assert (s == ref).all()
            wall[l0].append(w); dev[l0].append(d)
    print("F = %d (%d windows), stages 1-5 under form 2" % (frames, frames * n))
    for l0, name in ((0, "stage 0 integer pipe:"), (1, "stage 0 matrix cores:")):
        print("  %-22s wall                %s" % (name, spread(wall[l0])))
        print("  %-22s device, the stages  %s" % ("", spread(dev[l0])))
    for what, v in (("wall", wall), ("device (stages)", dev)):
        print("  %s: stage-0 form 1 median x%.3f, best x%.3f of form 0's; form 0's own spread x%.3f (max / min of its %d repeats)"
              % (what, statistics.median(v[1]) / statistics.median(v[0]), min(v[1]) / min(v[0]), max(v[0]) / min(v[0]), rounds))
for frames in CLIPS if sys.argv[2:] != ["l0"] else ():
    clip = np.ascontiguousarray(np.stack([np.roll(picture, 4 * f, axis=1) for f in range(frames)]))
    ref = route(clip, 0)[0]  # once each, untimed
    assert (route(clip, 1)[0] == ref).all() and (route(clip, 2)[0] == ref).all()
    wall, dev = {0: [], 1: [], 2: []}, {0: [], 1: [], 2: []}
    for r in range(rounds):
        for form in ((0, 1, 2), (1, 2, 0), (2, 0, 1))[r % 3]:  # the order rotates every round: no form always runs behind the same one
            s, w, d = route(clip, form)
            assert (s == ref).all()
            wall[form].append(w); dev[form].append(d)
    print("F = %d (%d windows)" % (frames, frames * n))
    for form, name in NAMES:
        print("  %-22s wall                %s" % (name, spread(wall[form])))
        print("  %-22s device, the stages  %s" % ("", spread(dev[form])))
    for what, v in (("wall", wall), ("device (stages)", dev)):
        for form, base in ((1, 0), (2, 1)):
            print("  %s, medians: form %d x%.3f of form %d; form %d's own spread x%.3f (max / min of its %d repeats)"
                  % (what, form, statistics.median(v[form]) / statistics.median(v[base]), base, base, max(v[base]) / min(v[base]), rounds))
clf.scan_form(was)
clf.scan_stage0_form(was0)
