"""CPU: bnn_mi355x_detect_windows_host -- the detections' model on the host (csrc/detect.cpp) -- against hand-worked
cases whose answer is written out here, against tests/detect_ref.py (the model restated in plain numpy) on every case of
tests/detect_cases.py, and what it refuses.  Host only: any library (a CNV and an LFC one are used), no GPU."""
import ctypes as C

import numpy as np
import pytest

import detect_cases as dc
import detect_ref

HOST = "bnn_mi355x_detect_windows_host"


@pytest.fixture(scope="module", params=["cnvW1A1", "lfcW1A1"])
def lib(request):
    return dc.load(request.param)


def check(lib, boxes, scores, o):
    got = dc.call(lib, HOST, boxes, scores, o)
    want = detect_ref.detect(boxes, scores, **o)
    for g, w, what in zip(got, want, ("dets", "counts", "n_candidates")):
        assert np.array_equal(g, w), what
    return got


NAMED = {c[0]: c for c in dc.named_cases()}


@pytest.mark.parametrize("name", sorted(NAMED))
def test_named_case_equals_the_numpy_model(lib, name):
    _, boxes, scores, o = NAMED[name]
    check(lib, boxes, scores, o)


def kept(lib, name):
    _, boxes, scores, o = NAMED[name]
    dets, counts, ncand = check(lib, boxes, scores, o)
    return [dets[f, :counts[f], 6].tolist() for f in range(len(counts))], ncand.tolist()


def test_iou_boundary(lib):
    """IoU 7/9 exactly: kept at (7, 9) -- the compare is strict --, suppressed at (50971, 65536) < 7/9"""
    assert 50971 * 9 < 7 * 65536
    assert kept(lib, "iou_boundary_kept_at_7_9") == ([[0, 1]], [2])
    assert kept(lib, "iou_boundary_suppressed_below") == ([[0]], [2])
    assert kept(lib, "num_equals_den_never_suppresses") == ([[0, 1]], [2])


def test_order_cap_and_max_det(lib):
    assert kept(lib, "ties_go_by_index") == ([[1, 3, 4, 6, 0, 2, 5, 7]], [8])
    assert kept(lib, "cap_cuts_inside_a_tie_group") == ([[1, 3, 0, 2, 4]], [8])  # 70, 70, then the first three of six at 50
    assert kept(lib, "max_det_stops_a_frame") == ([[0, 1, 2]], [8])


def test_classes(lib):
    assert kept(lib, "identical_boxes_of_two_classes") == ([[0, 1]], [2])
    assert kept(lib, "identical_boxes_of_one_class") == ([[0]], [2])
    assert kept(lib, "by_score_ignores_the_argmax") == ([[1]], [1])  # window 1's argmax is class 2
    assert kept(lib, "by_score_against_the_decode") == ([[]], [0])
    assert kept(lib, "all_scores_at_or_below_zero") == ([[1, 0]], [2])  # class 0 with scores 0 and -5
    assert kept(lib, "all_scores_at_or_below_zero_masked_out") == ([[]], [0])
    _, boxes, scores, o = NAMED["all_scores_at_or_below_zero"]
    assert dc.call(lib, HOST, boxes, scores, o)[0][0, :2, 4:6].tolist() == [[0, 0], [0, -5]]


def test_detection_fields(lib):
    _, boxes, scores, o = NAMED["iou_boundary_kept_at_7_9"]
    dets, counts, _ = dc.call(lib, HOST, boxes, scores, o)
    assert dets[0, :2].tolist() == [[0, 0, 32, 32, 1, 300, 0, 32], [4, 0, 36, 32, 1, 200, 1, 32]]
    assert not dets[0, 2:].any()  # the rows past the count are zero


def test_frames_are_independent(lib):
    _, boxes, scores, o = NAMED["three_frames"]
    dets, counts, ncand = check(lib, boxes, scores, o)
    for f in range(3):
        d1, c1, n1 = dc.call(lib, HOST, boxes, scores[f:f + 1], o)
        assert c1[0] == counts[f] and n1[0] == ncand[f] and np.array_equal(d1[0], dets[f])
    assert len(set(ncand.tolist())) > 1  # the frames differ


def test_fuzz(lib):
    cut = 0
    for _, boxes, scores, o in dc.fuzz_cases():
        _, _, ncand = check(lib, boxes, scores, o)
        cut += int((ncand > o["max_candidates"]).sum())
    assert cut > 50  # the cap did cut


def test_edge_inputs_equal_the_numpy_model(lib):
    """a few of the GPU test's larger inputs, so that its reference -- this entry point -- is itself pinned there"""
    for name, boxes, scores, o in dc.edge_cases():
        if name in ("edge_n4097_f3_c16", "edge_one_score_c16", "edge_spread_scores", "edge_n257_f1_c4096"):
            check(lib, boxes, scores, o)


REFUSALS = [
    (dict(class_mask=0), "class_mask"),
    (dict(class_mask=0b10000), "class_mask"),
    (dict(class_mask=0b0011, by_score=1), "by_score"),
    (dict(by_score=2), "by_score"),
    (dict(iou=(3, 2)), "iou_num"),
    (dict(iou=(-1, 2)), "iou_num"),
    (dict(iou=(0, 0)), "iou_den"),
    (dict(iou=(1, 65537)), "iou_den"),
    (dict(max_candidates=0), "max_candidates"),
    (dict(max_candidates=4097), "max_candidates"),
    (dict(max_det=0), "max_det"),
    (dict(max_candidates=8, max_det=9), "max_det"),
]


@pytest.mark.parametrize("change,word", REFUSALS)
def test_refused_options(lib, change, word):
    _, boxes, scores, o = NAMED["three_frames"]
    rc, msg = dc.call(lib, HOST, boxes, scores, dict(o, **change), raw=True)
    assert rc == -1 and msg.startswith("detect_windows_host: ") and word in msg, msg


@pytest.mark.parametrize("box", [(5, 0, 5, 9), (6, 0, 5, 9), (0, 9, 5, 9), (-1, 0, 5, 9), (0, 0, 65536, 9), (0, 0, 5, 65536)])
def test_refused_boxes(lib, box):
    _, boxes, scores, o = NAMED["three_frames"]
    bad = list(boxes)
    bad[5] = box
    rc, msg = dc.call(lib, HOST, bad, scores, o, raw=True)
    assert rc == -1 and "boxes[5]" in msg, msg


def test_refused_scores_counts_and_pointers(lib):
    _, boxes, scores, o = NAMED["three_frames"]
    for v in (32768, -32769):
        s = scores.copy()
        s[1, 2, 3] = v
        rc, msg = dc.call(lib, HOST, boxes, s, o, raw=True)
        assert rc == -1 and "scores[%d]" % ((1 * 8 + 2) * 4 + 3) in msg and "int16" in msg, msg
    b = np.ascontiguousarray(np.asarray(boxes, np.int32))
    s = np.ascontiguousarray(scores)
    co = dc.c_opts(o)
    out = np.zeros(3 * o["max_det"] * 8, np.int32)
    cnt, nc = np.zeros(3, np.int32), np.zeros(3, np.int32)
    good = [b.ctypes.data, 8, s.ctypes.data, 3, 4, C.byref(co), out.ctypes.data, cnt.ctypes.data, nc.ctypes.data]
    assert lib.bnn_mi355x_detect_windows_host(*good) == 0
    for at, word in ((0, "boxes"), (2, "scores"), (5, "opts"), (6, "dets"), (7, "counts"), (8, "n_candidates")):
        args = list(good)
        args[at] = None
        assert lib.bnn_mi355x_detect_windows_host(*args) == -1
        assert word in lib.bnn_mi355x_last_error().decode()
    for at, v, word in ((1, 0, "n must"), (1, -1, "n must"), (3, 0, "frames"), (3, 4097, "frames"), (4, 0, "number_class"), (4, 65, "number_class")):
        args = list(good)
        args[at] = v
        assert lib.bnn_mi355x_detect_windows_host(*args) == -1
        assert word in lib.bnn_mi355x_last_error().decode()
