#!/usr/bin/env python3
"""Locate objects in every frame of a clip (what the reference's *_Webcam notebooks do frame by frame) on an MI355X: a
few shifted copies of the street picture stand in for a camera's frames.  The whole clip goes to the GPU once; every frame
and every pyramid level (window sizes 64 and 96, stride size // 8) runs through ONE launch per layer, and the windows the
network calls a STOP sign are printed per frame.

    python examples/locate_in_clip.py [picture [frames [shift]]]
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
SIZES = (64, 96)

picture = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "street_with_stop.jpg")
frames = int(sys.argv[2]) if len(sys.argv) > 2 else 4
shift = int(sys.argv[3]) if len(sys.argv) > 3 else 16
classifier = bnn.CnvClassifier(bnn.NETWORK_CNVW1A1, "road-signs", bnn.RUNTIME_HW)
im = np.asarray(Image.open(picture).convert("RGB"))

# the "camera": frame f is the picture moved f * shift columns to the left (the columns that leave come back on the right)
clip = np.stack([np.roll(im, -f * shift, axis=1) for f in range(frames)])

boxes, classes = classifier.scan_clip(clip, sizes=SIZES)
windows = classes.size
print("%d frames of %d x %d, %d windows a frame: %.1f us upload + resizes, %.1f us stages (device time, whole clip)"
      % (frames, im.shape[1], im.shape[0], len(boxes), classifier.usecPreprocess * windows, classifier.usecPerImage * windows))
hits = classifier.locate_clip(clip, STOP, sizes=SIZES)
for f, found in enumerate(hits):
    assert found == [tuple(int(v) for v in b) for b, c in zip(boxes, classes[f]) if c == STOP]
    print("frame %d: class %d (%s) in %d windows%s" % (f, STOP, classifier.class_name(STOP), len(found), ": " + str(found[:4]) + (" ..." if len(found) > 4 else "") if found else ""))
# one frame by itself gives the same answer (locate with dense=True is scan_scene: the clip's frame, bit for bit)
assert hits[-1] == classifier.locate(clip[-1], STOP, sizes=SIZES, dense=True)
