#!/usr/bin/env python3
""""Locate objects within a scene" (the reference's notebooks/CNV-BNN_Road-Signs.ipynb, cells 13-16) on an MI355X: the
street picture is tiled into the notebook's 1 330 overlapping windows (sizes 64 and 96, stride size // 4), every window
is classified, and the windows the network calls a STOP sign are outlined -- first by class (cell 14), then by score
(cell 16).  The picture goes to the GPU once; the windows never come back as pictures or records.

    python examples/locate_stop_sign.py [picture [outlined.png]]
"""
import os
import sys

import torch  # noqa: F401  first: one HIP runtime per process

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bnn-pynq_amd"))
from PIL import Image, ImageDraw  # noqa: E402
import bnn  # noqa: E402

STOP = 14  # the class index the notebook looks for

picture = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "street_with_stop.jpg")
classifier = bnn.CnvClassifier(bnn.NETWORK_CNVW1A1, "road-signs", bnn.RUNTIME_HW)
im = Image.open(picture).convert("RGB")

# cell 13: the tiles
bounds = classifier.tile_boxes(im.size, sizes=(64, 96))
print(len(bounds))

# cell 14: every tile's class, the STOP tiles outlined
results = classifier.classify_windows(im, bounds)
print("%d windows: %.1f us upload + window kernels, %.1f us classification pass (device time)"
      % (len(bounds), classifier.usecPreprocess * len(bounds), classifier.usecPerImage * len(bounds)))
stop = [b for b, c in zip(bounds, results) if c == STOP]
assert stop == classifier.locate(im, STOP)  # the same thing in one call
print("class %d (%s): %d tiles" % (STOP, classifier.class_name(STOP), len(stop)))

# cell 16: only the tiles whose STOP score exceeds a threshold
sure = classifier.locate(im, STOP, min_score=455)
print("score > 455:", sure)

# the dense scan: the same window sizes at a stride twice as fine in each direction (size // 8), every level of the
# picture classified from one pass over the whole level instead of one pass per window
dense = classifier.locate(im, STOP, sizes=(64, 96), dense=True)
boxes, _ = classifier.scan_scene(im, sizes=(64, 96))
print("dense: %d windows: %.1f us upload + resizes, %.1f us scans (device time); class %d: %d windows"
      % (len(boxes), classifier.usecPreprocess * len(boxes), classifier.usecPerImage * len(boxes), STOP, len(dense)))

if len(sys.argv) > 2:
    out = im.copy()
    draw = ImageDraw.Draw(out)
    for b in dense:
        draw.rectangle(b, outline="orange")
    for b in stop:
        draw.rectangle(b, outline="red")
    for b in sure:
        draw.rectangle(b, outline="yellow")
    out.save(sys.argv[2])
    print("outlined:", sys.argv[2])
