#!/usr/bin/env python3
"""Read handwriting from a picture (the reference's notebooks/LFC-BNN_MNIST_Webcam.ipynb, cells 9-15) on an MI355X -- for
a whole line of digits at once.  A few digits are drawn with Pillow's own font on an off-white sheet, the sheet is split
into boxes where columns hold no ink, and every box goes through the notebook's procedure (contrast, brightness, bounding
box of the ink, 28 x 28, invert) and the LFC network in ONE call: the picture goes to the GPU once, the records never
come back.  The mnist parameters were trained on handwriting; Pillow's font is print, so expect misread digits (the
host route through Pillow and classify_mnists reads the same ones): the example shows the path, not the accuracy.

    python examples/read_glyphs.py [digits [enhanced.png]]
"""
import os
import sys

import torch  # noqa: F401  first: one HIP runtime per process

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bnn-pynq_amd"))
import numpy as np  # noqa: E402
from PIL import Image, ImageDraw, ImageFont  # noqa: E402
import bnn  # noqa: E402

digits = sys.argv[1] if len(sys.argv) > 1 else "3141592"
classifier = bnn.LfcClassifier(bnn.NETWORK_LFCW1A1, "mnist", bnn.RUNTIME_HW)

# the "camera frame": dark digits on a sheet that is not quite white
sheet = Image.new("RGB", (40 + 50 * len(digits), 100), (238, 236, 230))
draw = ImageDraw.Draw(sheet)
font = ImageFont.load_default(size=64)
for i, ch in enumerate(digits):
    draw.text((30 + 50 * i, 12), ch, font=font, fill=(25, 25, 40))

# cell 9: what the notebook displays
enhanced = classifier.enhance(sheet)
if len(sys.argv) > 2:
    enhanced.save(sys.argv[2])
    print("enhanced:", sys.argv[2])

# one box per run of columns that hold ink (finding the boxes is the caller's business: any segmentation will do)
ink_columns = (np.asarray(enhanced) != 255).any(axis=0)
edges = np.flatnonzero(np.diff(np.concatenate([[0], ink_columns.astype(np.int8), [0]])))
boxes = [(int(a), 0, int(b), sheet.size[1]) for a, b in zip(edges[::2], edges[1::2])]
print("%d boxes" % len(boxes))

# cells 11-15 for all of them
classes = classifier.classify_glyphs(sheet, boxes)
print("%d glyphs: %.1f us upload + glyph kernels, %.1f us classification pass (device time)"
      % (len(boxes), classifier.usecPreprocess * len(boxes), classifier.usecPerImage * len(boxes)))
print("drawn:", digits)
print("read: ", "".join(classifier.class_name(c) if c >= 0 else "?" for c in classes))
