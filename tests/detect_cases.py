"""Inputs of the detections' tests (tests/test_detect_host.py on the CPU, tests/test_gpu_detect.py on the GPU) and the one
way both call the C ABI.  A case is (name, boxes [n, 4], scores [F, n, ncls], options); the options are the keyword
arguments of detect_ref.detect."""
import ctypes as C

import numpy as np

import gpu_lib as gl
import scan_ref
from bnn import abi

FIELDS = 8


def options(class_mask, by_score=0, min_score=-32769, iou=(1, 2), max_candidates=4096, max_det=64):
    return dict(class_mask=class_mask, by_score=by_score, min_score=min_score, iou=iou, max_candidates=max_candidates, max_det=max_det)


def c_opts(o):
    return abi.DetectOpts(o["class_mask"], o["by_score"], o["min_score"], o["iou"][0], o["iou"][1], o["max_candidates"], o["max_det"])


def call(lib, symbol, boxes, scores, o, raw=False):
    """(dets [F, max_det, 8], counts [F], n_candidates [F]) of ``symbol`` (detect_windows_host or detect_windows); with ``raw``
    the return code and the message instead of an assertion"""
    b = np.ascontiguousarray(np.asarray(boxes, np.int32).reshape(-1, 4))
    s = np.ascontiguousarray(np.asarray(scores, np.int32))
    frames, n, ncls = s.shape
    assert n == len(b)
    md = max(int(o["max_det"]), 1)
    dets = np.full((frames, md, FIELDS), -7, np.int32)
    counts, ncand = np.full(frames, -7, np.int32), np.full(frames, -7, np.int32)
    co = c_opts(o)
    args = [b.ctypes.data, n, s.ctypes.data, frames, ncls, C.byref(co), dets.ctypes.data, counts.ctypes.data, ncand.ctypes.data]
    if symbol == "bnn_mi355x_detect_windows":
        args.append(None)
    rc = getattr(lib, symbol)(*args)
    if raw:
        return rc, lib.bnn_mi355x_last_error().decode()
    assert rc == 0, lib.bnn_mi355x_last_error().decode()
    return dets, counts, ncand


def one_hot(cls, score, ncls=4, rest=0):
    """[n, ncls] scores: window i has ``score[i]`` at ``cls[i]`` and ``rest`` elsewhere"""
    s = np.full((len(cls), ncls), rest, np.int32)
    s[np.arange(len(cls)), cls] = score
    return s


def named_cases():
    A, B = (0, 0, 32, 32), (4, 0, 36, 32)  # inter 28 * 32 = 896, union 2 * 1024 - 896 = 1152: IoU 7/9
    far = [(100 * i, 0, 100 * i + 32, 32) for i in range(8)]
    cases = []
    two = one_hot([1, 1], [300, 200])[None]
    cases.append(("iou_boundary_kept_at_7_9", [A, B], two, options(0b10, iou=(7, 9))))
    cases.append(("iou_boundary_suppressed_below", [A, B], two, options(0b10, iou=(50971, 65536))))
    cases.append(("num_equals_den_never_suppresses", [A, A], two, options(0b10, iou=(5, 5))))
    cases.append(("ties_go_by_index", far, one_hot([2] * 8, [50, 70, 50, 70, 70, 50, 70, 50])[None], options(0b100)))
    cases.append(("cap_cuts_inside_a_tie_group", far, one_hot([2] * 8, [50, 70, 50, 70, 50, 50, 50, 50])[None], options(0b100, max_candidates=5, max_det=5)))
    cases.append(("max_det_stops_a_frame", far, one_hot([2] * 8, [8, 7, 6, 5, 4, 3, 2, 1])[None], options(0b100, max_det=3)))
    cases.append(("identical_boxes_of_two_classes", [A, A], one_hot([1, 3], [300, 200])[None], options(0b1010, iou=(0, 1))))
    cases.append(("identical_boxes_of_one_class", [A, A], one_hot([1, 1], [300, 200])[None], options(0b1010, iou=(0, 1))))
    by = np.array([[[500, 10, 460, 0], [100, 456, 900, 0], [100, 455, 900, 0]]], np.int32)  # class 1 above 455: windows 0 (no), 1 (yes), 2 (no)
    cases.append(("by_score_ignores_the_argmax", far[:3], by, options(0b10, by_score=1, min_score=455)))
    cases.append(("by_score_against_the_decode", far[:3], by, options(0b10, by_score=0, min_score=455)))
    neg = np.array([[[-5, -1, 0, -7], [0, 0, 0, 0]]], np.int32)  # no score above 0: the class is 0
    cases.append(("all_scores_at_or_below_zero", far[:2], neg, options(0b1111, min_score=-100)))
    cases.append(("all_scores_at_or_below_zero_masked_out", far[:2], neg, options(0b1110, min_score=-100)))
    cases.append(("no_candidates", far[:2], neg, options(0b1111, min_score=0)))
    rng = np.random.default_rng(11)
    three = rng.choice([0, 100, 200, 300], size=(3, 8, 4)).astype(np.int32)
    cases.append(("three_frames", far, three, options(0b1111, min_score=250, max_det=4)))
    ext = [(0, 0, 65535, 65535), (1, 1, 65535, 65535), (65534, 65534, 65535, 65535)]
    cases.append(("extreme_coordinates", ext, one_hot([0, 0, 0], [32767, 32767, -32768])[None], options(0b1, iou=(65533, 65536))))
    cases.append(("one_window", [A], one_hot([3], [1])[None], options(0b1000, max_candidates=1, max_det=1)))
    return cases


def fuzz_cases(count=200, seed=2024):
    """seeded: n <= 200, scores drawn from four values so that ties are everywhere, boxes from scan_ref.boxes (a 96 x 64
    frame at sizes 32 and 48) or random ones, random options"""
    rng = np.random.default_rng(seed)
    pyramid = np.array(scan_ref.boxes(96, 64, 32) + scan_ref.boxes(96, 64, 48), np.int32)
    cases = []
    for k in range(count):
        n = int(rng.integers(1, 201))
        if rng.integers(2):
            boxes = pyramid[rng.choice(len(pyramid), size=min(n, len(pyramid)), replace=False)]
            n = len(boxes)
        else:
            lu = rng.integers(0, 60, size=(n, 2))
            wh = rng.integers(1, 40, size=(n, 2))
            boxes = np.concatenate([lu, lu + wh], axis=1).astype(np.int32)
        frames, ncls = int(rng.integers(1, 4)), int(rng.integers(1, 9))
        values = np.sort(rng.integers(-40, 600, size=4))
        scores = rng.choice(values, size=(frames, n, ncls)).astype(np.int32)
        by_score = int(rng.integers(2))
        mask = 1 << int(rng.integers(ncls)) if by_score else int(rng.integers(1, 1 << ncls))
        den = int(rng.integers(1, 65537))
        mc = int(rng.choice([1, 2, 7, 64, 4096]))
        o = options(mask, by_score, int(rng.choice(list(values) + [-32769])) - int(rng.integers(2)), (int(rng.integers(0, den + 1)), den), mc,
                    int(rng.integers(1, min(mc, 80) + 1)))
        cases.append(("fuzz%03d" % k, boxes, scores, o))
    return cases


def edge_cases():
    """the wave, block and cap edges of the kernels: n in {1, 63, 64, 65, 257, 4097}, F in {1, 3}, max_candidates in {1, 16,
    4096}; at 4097 one case has every candidate on ONE score, so that the cut is by index alone"""
    rng = np.random.default_rng(7)
    cases = []
    for n in (1, 63, 64, 65, 257, 4097):
        lu = rng.integers(0, 300, size=(n, 2))
        wh = rng.integers(8, 64, size=(n, 2))
        boxes = np.concatenate([lu, lu + wh], axis=1).astype(np.int32)
        for frames in (1, 3):
            scores = rng.choice([-3, 90, 91, 300, 301, 4000], size=(frames, n, 3)).astype(np.int32)
            for mc in (1, 16, 4096):
                cases.append(("edge_n%d_f%d_c%d" % (n, frames, mc), boxes, scores, options(0b111, min_score=0, iou=(1, 3), max_candidates=mc, max_det=min(mc, 128))))
        if n == 4097:
            flat = np.full((2, n, 3), 77, np.int32)
            for mc in (1, 16, 4096):
                cases.append(("edge_one_score_c%d" % mc, boxes, flat, options(0b010, by_score=1, iou=(9, 10), max_candidates=mc, max_det=mc)))
            spread = rng.integers(-32768, 32768, size=(1, n, 3)).astype(np.int32)  # every byte of the score takes part in the cut
            cases.append(("edge_spread_scores", boxes, spread, options(0b111, iou=(1, 2), max_candidates=4096, max_det=200)))
            cases.append(("edge_spread_scores_c16", boxes, spread, options(0b100, by_score=1, iou=(1, 2), max_candidates=16, max_det=16)))
    return cases


def load(network):
    return gl.load(network)
