#!/usr/bin/env python3
"""Detect objects in camera frames on an MI355X: the clip of examples/detect_in_clip.py as a decoder delivers it -- NV12, a
Y plane and interleaved CbCr at a quarter of the resolution, 1.5 bytes a pixel -- without a conversion on the host.  From
host memory the frames go up as they are and become RGB on the GPU; from a torch tensor (a decoder's surface) they are read
where they lie in HBM, on the current stream.  Both give the same lists as the RGB frames the conversion makes.

    python examples/detect_in_camera_clip.py [picture [frames [shift]]]
"""
import os
import sys

import torch  # first: one HIP runtime per process

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
im = Image.open(picture).convert("RGB")
im = np.asarray(im.crop((0, 0, im.size[0] & ~1, im.size[1] & ~1)))  # NV12 needs an even width and height
h, w = im.shape[:2]


def nv12_of(rgb):
    """the "decoder": Pillow's YCbCr, the chroma of the upper left pixel of every 2 x 2 block"""
    ycc = np.asarray(Image.fromarray(rgb).convert("YCbCr"))
    return np.concatenate([ycc[:, :, 0], ycc[0::2, 0::2, 1:].reshape(h // 2, w)])


# the "camera": frame f is the picture moved f * shift columns to the left, as NV12 [frames, h * 3 / 2, w]
clip = np.stack([nv12_of(np.roll(im, -f * shift, axis=1)) for f in range(frames)])
kwargs = dict(sizes=SIZES, min_score=MIN_SCORE, by_score=True, iou=0.3)

from_host = classifier.detect_clip(clip, STOP, pixel_format="nv12", **kwargs)
print("%d NV12 frames of %d x %d, %d bytes uploaded (RGB: %d): %.1f us a window for the frames' way to the device, their conversion and the resizes"
      % (frames, w, h, clip.nbytes, frames * w * h * 3, classifier.usecPreprocess))
from_tensor = classifier.detect_clip(torch.from_numpy(clip).cuda(), STOP, pixel_format="nv12", **kwargs)
assert from_tensor == from_host
# what a user did before: convert on the host, hand RGB frames over
assert classifier.detect_clip(classifier.unpack_frames(clip, "nv12"), STOP, **kwargs) == from_host
for f, dets in enumerate(from_host):
    print("frame %d: %d detection%s%s" % (f, len(dets), "" if len(dets) == 1 else "s",
                                          ": " + ", ".join("%s score %d" % (box, score) for box, _, score in dets) if dets else ""))
