#!/usr/bin/env python3
"""Detect in a clip of NV12 camera frames: the clip of scan_clip_rate.py and detect_rate.py -- the 640 x 480 street picture
rolled by 4 f columns per frame, window sizes (64, 96), cnvW1A1 road-signs, class 14 above a score of 455 -- handed over as
NV12.  The NV12 frames are made once from the RGB frames (Pillow's YCbCr, chroma of the upper left pixel of each 2 x 2
block); the RGB the yardstick gets is the model on them (tests/pixfmt_ref.py), so every route sees the same pixels and the
detections are asserted equal in every call.
  yardstick (a)  detect_clip on the ready RGB clip
  yardstick (b)  the numpy restatement of the conversion on the host, then (a): what a user with NV12 frames does today
  route (c)      detect_clip(pixel_format="nv12") from host memory
  route (d)      the same from a CUDA tensor
The four alternate in one process; medians and ranges of seven wall times after one untimed call each.  Also: the device
time of k_unpack_frames alone (bnn_mi355x_unpack_frames), the bytes uploaded, and the kernel's traffic rate (bytes read +
bytes written) against a hipMemcpyDtoD that moves the same traffic in the same run.  A difference is called established
only where the ranges are disjoint and the medians differ by more than yardstick (a)'s own max / min spread.
The record goes to profiles/r32_clip_frames_rate.txt.  usage: clip_frames_rate.py [rounds [F ...]]"""
import contextlib
import ctypes
import io
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bnn-pynq_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from PIL import Image  # noqa: E402
import bnn  # noqa: E402
from bnn import abi  # noqa: E402
import pixfmt_ref  # noqa: E402

SIZES = (64, 96)
W, H = 640, 480
STOP, MIN_SCORE, IOU, MAX_DET = 14, 455, (32768, 65536), 64


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


def to_nv12(rgb):
    """[F, H, W, 3] -> [F, H * 3 / 2, W]: any forward transform will do, the routes are compared on what the model makes of it"""
    out = np.empty((len(rgb), H * 3 // 2, W), np.uint8)
    for f, frame in enumerate(rgb):
        ycc = np.asarray(Image.fromarray(frame).convert("YCbCr"))
        out[f, :H] = ycc[:, :, 0]
        out[f, H:] = ycc[0::2, 0::2, 1:].reshape(H // 2, W)
    return out


rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
frame_counts = [int(a) for a in sys.argv[2:]] or [1, 16, 64]
with quiet():
    clf = bnn.CnvClassifier(bnn.NETWORK_CNVW1A1, "road-signs", bnn.RUNTIME_SW)
lib = clf.bnn.interface
im = np.asarray(Image.open(os.path.join(ROOT, "tests", "golden", "street_with_stop.jpg")).convert("RGB"))
assert im.shape == (H, W, 3)
n = sum(len(clf.scan_boxes((W, H), s)[1]) for s in SIZES)
KW = dict(sizes=SIZES, min_score=MIN_SCORE, by_score=True, iou=IOU, max_det=MAX_DET)


def timed(fn):
    t0 = time.perf_counter()
    found = fn()
    return found, 1e3 * (time.perf_counter() - t0)


def spread(v):
    return "median %8.3f  range %8.3f .. %8.3f  (%s)" % (statistics.median(v), min(v), max(v), " ".join("%.3f" % x for x in v))


def verdict(name, v, against, v0, own):
    ratio = statistics.median(v) / statistics.median(v0)
    disjoint = max(v) < min(v0) or min(v) > max(v0)
    said = "established" if disjoint and abs(ratio - 1) > own - 1 else "not established"
    return "%s x%.3f of %s: %s" % (name, ratio, against, said)


def unpack_alone(nv12):
    """device ms of k_unpack_frames on the uploaded clip (bnn_mi355x_unpack_frames), median of `rounds`"""
    fr = abi.Frames(abi.PIXEL_FORMATS["nv12"], 0, W, H, len(nv12), 0, 0)
    out = np.empty((len(nv12), H, W, 3), np.uint8)
    usec, ms = ctypes.c_float(0), []
    for _ in range(rounds + 1):
        assert lib.bnn_mi355x_unpack_frames(ctypes.byref(fr), nv12.ctypes.data, out.ctypes.data, ctypes.byref(usec)) == 0
        ms.append(usec.value * len(nv12) / 1e3)
    return ms[1:], out


def dtod(nbytes):
    """device ms of one hipMemcpyDtoD of nbytes between two tensors, median of `rounds`"""
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpyDtoDAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    src, dst = torch.zeros(nbytes, dtype=torch.uint8, device="cuda"), torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    ms = []
    for _ in range(rounds + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        assert hip.hipMemcpyDtoDAsync(dst.data_ptr(), src.data_ptr(), nbytes, stream) == 0
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return ms[1:]


print("cnvW1A1 road-signs, street_with_stop.jpg %d x %d rolled by 4 f columns as NV12, sizes %s: %d windows a frame; class %d (%s) by score above %d, "
      "IoU %d / %d, max_det %d; wall ms per clip, %d alternations of the four routes in one process after one untimed call each; detections equal in "
      "every call" % (W, H, SIZES, n, STOP, clf.classes[STOP], MIN_SCORE, IOU[0], IOU[1], MAX_DET, rounds))
for frames in frame_counts:
    nv12 = to_nv12(np.stack([np.roll(im, -4 * f, axis=1) for f in range(frames)]))
    rgb = pixfmt_ref.unpack(nv12, "nv12", W, H, frames)
    tensor = torch.from_numpy(nv12).cuda()
    routes = [
        ("(a) detect_clip on the ready RGB clip", lambda: clf.detect_clip(rgb, STOP, **KW)),
        ("(b) numpy conversion, then (a)", lambda: clf.detect_clip(pixfmt_ref.unpack(nv12, "nv12", W, H, frames), STOP, **KW)),
        ("(c) detect_clip(nv12), host memory", lambda: clf.detect_clip(nv12, STOP, pixel_format="nv12", **KW)),
        ("(d) detect_clip(nv12), CUDA tensor", lambda: clf.detect_clip(tensor, STOP, pixel_format="nv12", **KW)),
    ]
    with quiet():  # once each, untimed: the workspaces
        ref = routes[0][1]()
        for _, fn in routes[1:]:
            assert fn() == ref
    walls, pre = [[] for _ in routes], [[] for _ in routes]
    for _ in range(rounds):
        for k, (_, fn) in enumerate(routes):
            with quiet():
                found, ms = timed(fn)
            assert found == ref
            walls[k].append(ms)
            pre[k].append(clf.usecPreprocess * n * frames / 1e3)
    print("F = %d (%d windows)" % (frames, n * frames))
    for k, (name, _) in enumerate(routes):
        print("  %-38s wall                        %s" % (name, spread(walls[k])))
        print("  %-38s device, frames' way + resizes %s" % ("", spread(pre[k])))
    own = max(walls[0]) / min(walls[0])
    print("  yardstick (a)'s own spread x%.3f (max / min of %d calls)" % (own, rounds))
    for k, other in ((2, 1), (2, 0), (3, 1), (3, 0), (3, 2)):
        print("  " + verdict(routes[k][0][:3], walls[k], routes[other][0][:3], walls[other], own))
    with quiet():
        unpack_ms, out = unpack_alone(nv12)
    assert np.array_equal(out, rgb)
    raw_bytes, rgb_bytes = nv12.nbytes, rgb.nbytes
    copy_ms = dtod((raw_bytes + rgb_bytes) // 2)
    u, c = statistics.median(unpack_ms), statistics.median(copy_ms)
    print("  bytes uploaded: %d as NV12 against %d as RGB" % (raw_bytes, rgb_bytes))
    print("  k_unpack_frames alone, device ms:   %s" % spread(unpack_ms))
    print("  hipMemcpyDtoD of %d bytes, device ms: %s" % ((raw_bytes + rgb_bytes) // 2, spread(copy_ms)))
    print("  traffic (bytes read + written = %d in both): k_unpack_frames %.1f GB/s, hipMemcpyDtoD %.1f GB/s (x%.3f)"
          % (raw_bytes + rgb_bytes, (raw_bytes + rgb_bytes) / u / 1e6, (raw_bytes + rgb_bytes) / c / 1e6, c / u))
    print("  detections per frame: %s%s" % (" ".join(str(len(d)) for d in ref[:8]), " ..." if frames > 8 else ""))
