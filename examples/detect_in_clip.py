#!/usr/bin/env python3
"""Detect objects in every frame of a clip on an MI355X: the clip of examples/locate_in_clip.py -- a few shifted copies of
the street picture stand in for a camera's frames -- ending in ONE box per sign instead of every window that fires.  The
clip goes to the GPU once; the scan's launches run, then the detection kernels (threshold, order, non-maximum suppression)
work on the scores where the scan left them, and only the short lists come back.

    python examples/detect_in_clip.py [picture [frames [shift]]]
"""
import os
import sys

import torch  # noqa: F401  first: one HIP runtime per process

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bnn-pynq_amd"))
import numpy as np  # noqa: E402
from PIL import Image  # noqa: E402
import bnn  # noqa: E402

STOP = 14  # the class index the road-signs notebook looks for
MIN_SCORE = 455  # cell 16: result[i][14] > 455
SIZES = (64, 96)

picture = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "street_with_stop.jpg")
frames = int(sys.argv[2]) if len(sys.argv) > 2 else 4
shift = int(sys.argv[3]) if len(sys.argv) > 3 else 16
classifier = bnn.CnvClassifier(bnn.NETWORK_CNVW1A1, "road-signs", bnn.RUNTIME_HW)
im = np.asarray(Image.open(picture).convert("RGB"))

# the "camera": frame f is the picture moved f * shift columns to the left (the columns that leave come back on the right)
clip = np.stack([np.roll(im, -f * shift, axis=1) for f in range(frames)])

# every window that fires, as the notebook draws them ...
hits = classifier.locate_clip(clip, STOP, sizes=SIZES, min_score=MIN_SCORE)
# ... and the detections: the best window of every group of overlapping ones (IoU above 0.3 with a better one: dropped)
found = classifier.detect_clip(clip, STOP, sizes=SIZES, min_score=MIN_SCORE, by_score=True, iou=0.3)
print("%d frames of %d x %d: %.1f us detection kernels a frame (device time)" % (frames, im.shape[1], im.shape[0], classifier.usecDetect))
for f, (windows, dets) in enumerate(zip(hits, found)):
    assert classifier.n_candidates[f] == len(windows) and all(box in windows for box, _, _ in dets)
    print("frame %d: %d windows fire for class %d (%s) -> %d detection%s%s" % (
        f, len(windows), STOP, classifier.class_name(STOP), len(dets), "" if len(dets) == 1 else "s",
        ": " + ", ".join("%s score %d" % (box, score) for box, _, score in dets) if dets else ""))
# one picture by itself gives the same answer
assert found[-1] == classifier.detect(clip[-1], STOP, sizes=SIZES, min_score=MIN_SCORE, by_score=True, iou=0.3)
