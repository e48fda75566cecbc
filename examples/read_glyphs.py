#!/usr/bin/env python3
"""Read handwriting from a picture (the reference's notebooks/LFC-BNN_MNIST_Webcam.ipynb, cells 9-15) on an MI355X -- for
a whole line of digits at once: "here is a frame, what does it say".  A few digits are drawn with Pillow's own font on an
off-white sheet and read_glyphs does the rest in ONE call: the picture goes to the GPU once, the glyphs are found there
(the connected components of the ink of the enhanced plane, left to right), every glyph goes through the notebook's
procedure (contrast, brightness, bounding box of the ink, 28 x 28, invert) and the LFC network, and neither the plane nor
the records come back.  The column split this example used to find its boxes with stays as a cross-check: on one line of
separate glyphs the found boxes have exactly its x-ranges.  The mnist parameters were trained on handwriting; Pillow's
font is print, so expect misread digits (the host route through Pillow and classify_mnists reads the same ones): the
example shows the path, not the accuracy.

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

# cells 9-15 for the whole sheet: find the glyphs, make their records, classify them
classes, boxes = classifier.read_glyphs(sheet, order="left")
n = len(boxes)
print("%d glyphs found" % classifier.glyphs_found)
if n:
    print("%d glyphs: %.1f us upload + labelling + glyph kernels, %.1f us classification pass (device time)"
          % (n, classifier.usecPreprocess * n, classifier.usecPerImage * n))
print("drawn:", digits)
print("read: ", "".join(classifier.class_name(c) if c >= 0 else "?" for c in classes))

# the cross-check: cell 9's picture, split where columns hold no ink (what a caller without find_glyphs would do; it
# fails for two lines, for glyphs whose columns overlap and for a speck of noise anywhere in a column)
enhanced = classifier.enhance(sheet)
if len(sys.argv) > 2:
    enhanced.save(sys.argv[2])
    print("enhanced:", sys.argv[2])
ink_columns = (np.asarray(enhanced) != 255).any(axis=0)
edges = np.flatnonzero(np.diff(np.concatenate([[0], ink_columns.astype(np.int8), [0]])))
split = [(int(a), int(b)) for a, b in zip(edges[::2], edges[1::2])]
found = [(int(b[0]), int(b[2])) for b in boxes]
print("x-ranges of the found boxes %s the column split's: %s" % ("equal" if found == split else "DIFFER from", found))

# A page: two lines, and two strokes whose boxes overlap.  read_glyphs would interleave the lines by x and hand the net
# each stroke with a piece of the other in its record; read_page puts the glyphs into lines (a glyph joins the line whose
# band it overlaps by half), marks the word gaps, and masks every glyph to its own ink.
page = Image.new("RGB", (40 + 50 * len(digits) + 130, 200), (238, 236, 230))
draw = ImageDraw.Draw(page)
for j, row in enumerate((digits, digits[::-1])):
    for i, ch in enumerate(row):
        draw.text((30 + 50 * i + (40 if i >= 3 else 0), 12 + 100 * j), ch, font=font, fill=(25, 25, 40))
x = 40 + 50 * len(digits) + 45
draw.line((x, 80, x + 40, 20), fill=(25, 25, 40), width=5)        # a "/" ...
draw.line((x + 34, 45, x + 62, 95), fill=(25, 25, 40), width=5)   # ... and a "\\" under its arm: they do not touch, their boxes overlap
classes, boxes, lines, gaps = classifier.read_page(page, word_gap=40)
print("a page of %d glyphs in %d lines, read line by line with the glyphs masked to their own ink:" % (len(boxes), len(set(lines.tolist()))))
print(classifier.read_text(page, mask=True, lines=True, word_gap=40))
cropped, _, _, _ = classifier.read_page(page, mask=False, word_gap=40)
changed = [i for i in range(len(boxes)) if classes[i] != cropped[i]]
print("glyphs whose class differs when a neighbour's ink stays in the record (mask=False): %s"
      % (", ".join("%d at x %d..%d" % (i, boxes[i][0], boxes[i][2]) for i in changed) or "none"))
print("read_glyphs' order on the same page, by left edge alone:", classifier.read_text(page))
