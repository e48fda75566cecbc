"""GPU: the detections (bnn_mi355x_detect_windows / bnn_mi355x_detect_clip, CnvClassifier.suppress / detect_clip / detect;
csrc/detect_kernels.hip).

Everything is exact.  The kernels on chosen inputs must equal the host model (bnn_mi355x_detect_windows_host, which
tests/test_detect_host.py pins to tests/detect_ref.py) byte for byte on dets, counts and n_candidates; a clip's detections
must equal tests/detect_ref.py on the scores and boxes bnn_mi355x_scan_clip returns for it."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import detect_cases as dc
import detect_ref
import gpu_lib as gl
import scan_ref

sys.path.insert(0, os.path.join(gl.ROOT, "bnn-pynq_amd"))

pytestmark = pytest.mark.gpu

HOST, DEVICE = "bnn_mi355x_detect_windows_host", "bnn_mi355x_detect_windows"
W, H, SIZES, FRAMES, WINDOWS = 96, 64, (32, 48), 3, 180


def err(L):
    return L.bnn_mi355x_last_error().decode()


# ---- 1. the kernels on chosen inputs ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["cnvW1A1", "cnvW2A2"])
def lib(request):
    return gl.load(request.param)  # (no parameters are needed: the scores are the caller's)


def same_as_host(lib, cases):
    for name, boxes, scores, o in cases:
        want = dc.call(lib, HOST, boxes, scores, o)
        got = dc.call(lib, DEVICE, boxes, scores, o)
        for g, w, what in zip(got, want, ("dets", "counts", "n_candidates")):
            assert g.tobytes() == w.tobytes(), (name, what, o)


def test_named_cases_equal_the_host_model(lib):
    same_as_host(lib, dc.named_cases())


def test_fuzz_cases_equal_the_host_model(lib):
    same_as_host(lib, dc.fuzz_cases())


def test_wave_block_and_cap_edges_equal_the_host_model(lib):
    cases = dc.edge_cases()
    assert {c[1].shape[0] for c in cases} == {1, 63, 64, 65, 257, 4097}
    same_as_host(lib, cases)
    # at 4097 windows on one score the cut is by index alone: the first max_candidates windows, in order
    name, boxes, scores, o = next(c for c in cases if c[0] == "edge_one_score_c4096")
    o = dict(o, iou=(1, 1))  # nothing is suppressed: every one of the 4096 is kept
    dets, counts, ncand = dc.call(lib, DEVICE, boxes, scores, o)
    assert counts.tolist() == [4096, 4096] and ncand.tolist() == [4097, 4097]
    assert (dets[:, :, 6] == np.arange(4096)).all()


def test_device_time_and_refusals(lib):
    _, boxes, scores, o = dc.named_cases()[0]
    b, s = np.ascontiguousarray(np.asarray(boxes, np.int32)), np.ascontiguousarray(scores)
    dets, counts, ncand = np.zeros((1, o["max_det"], 8), np.int32), np.zeros(1, np.int32), np.zeros(1, np.int32)
    usec = C.c_float(-1)
    co = dc.c_opts(o)
    assert lib.bnn_mi355x_detect_windows(b.ctypes.data, 2, s.ctypes.data, 1, 4, C.byref(co), dets.ctypes.data, counts.ctypes.data, ncand.ctypes.data,
                                         C.byref(usec)) == 0, err(lib)
    assert usec.value > 0
    rc, msg = dc.call(lib, DEVICE, boxes, scores, dict(o, class_mask=0), raw=True)
    assert rc == -1 and msg.startswith("detect_windows: ") and "class_mask" in msg


def test_lfc_libraries_refuse_the_device_route():
    L = gl.load("lfcW1A1")
    _, boxes, scores, o = dc.named_cases()[0]
    rc, msg = dc.call(L, DEVICE, boxes, scores, o, raw=True)
    assert rc == -1 and "CNV networks only" in msg


# ---- 2. the clip ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def param_dirs(tmp_path_factory):
    import random_params
    d = tmp_path_factory.mktemp("rp_detect")
    random_params.make(str(d), "cnvW1A1", 313)
    return {"cifar10": gl.param_dir("cifar10", "cnvW1A1"), "random": str(d)}


@pytest.fixture(scope="module")
def L():
    lib = gl.load("cnvW1A1")
    yield lib
    lib.load_parameters(gl.param_dir("cifar10", "cnvW1A1").encode())  # leave the library as found


def clip_of(mode, seed=0):
    shape = (FRAMES, H, W) if mode == "L" else (FRAMES, H, W, 3)
    return np.random.default_rng(4242 + seed + (mode == "L")).integers(0, 256, shape, dtype=np.uint8)


def scan_clip(L, clip, ncls, detail):
    frames, bands = clip.shape[0], 1 if clip.ndim == 3 else 3
    sz = np.asarray(SIZES, np.int32)
    boxes = np.full((WINDOWS, 4), -1, np.int32)
    p = L.bnn_mi355x_scan_clip(clip.ctypes.data, frames, 0, W, H, bands, 0, sz.ctypes.data, len(sz), ncls, boxes.ctypes.data, None, None, 1 if detail else 0)
    assert p, err(L)
    out = np.ctypeslib.as_array(p, shape=(frames * WINDOWS * (ncls if detail else 1),)).astype(np.int32, copy=True)
    L.free_results(p)
    return boxes, (out.reshape(frames, WINDOWS, ncls) if detail else out.reshape(frames, WINDOWS))


def detect_clip(L, clip, ncls, o, raw=False, size=(W, H), sizes=SIZES):
    frames, bands = clip.shape[0], 1 if clip.ndim == 3 else 3
    sz = np.asarray(sizes, np.int32)
    dets = np.full((frames, o["max_det"], 8), -7, np.int32)
    counts, ncand = np.full(frames, -7, np.int32), np.full(frames, -7, np.int32)
    co = dc.c_opts(o)
    usec, pre, det = C.c_float(-1), C.c_float(-1), C.c_float(-1)
    rc = L.bnn_mi355x_detect_clip(clip.ctypes.data, frames, 0, size[0], size[1], bands, 0, sz.ctypes.data, len(sz), ncls, C.byref(co), dets.ctypes.data,
                                  counts.ctypes.data, ncand.ctypes.data, C.byref(usec), C.byref(pre), C.byref(det))
    if raw:
        return rc, err(L)
    assert rc == 0, err(L)
    assert usec.value > 0 and pre.value > 0 and det.value > 0
    return dets, counts, ncand


def test_the_pyramid_of_the_clip_tests():
    """180 windows a frame, and 7/9 is the largest IoU two different windows have (checked with the level rule of scan_ref)"""
    boxes = scan_ref.boxes(W, H, 32) + scan_ref.boxes(W, H, 48)
    assert (len(scan_ref.boxes(W, H, 32)), len(scan_ref.boxes(W, H, 48)), len(boxes)) == (153, 27, WINDOWS)
    over = [(a, b) for i, a in enumerate(boxes) for b in boxes[i + 1:] if detect_ref.suppresses(a, b, 7, 9)]
    assert not over
    assert any(detect_ref.suppresses(a, b, 50971, 65536) for a in boxes[:2] for b in boxes[:2] if a != b)


@pytest.mark.parametrize("mode", ["RGB", "L"])
@pytest.mark.parametrize("params", ["cifar10", "random"])
def test_clip_equals_the_model_on_the_scan_clip_scores(L, param_dirs, params, mode):
    L.load_parameters(param_dirs[params].encode())
    assert err(L) == ""
    clip = clip_of(mode)
    boxes, scores = scan_clip(L, clip, 64, True)
    _, classes = scan_clip(L, clip, 10, False)
    assert boxes.tolist() == [list(b) for b in scan_ref.boxes(W, H, 32) + scan_ref.boxes(W, H, 48)]
    # by_score = 0, every class: the decode's class
    o = dc.options((1 << 10) - 1, min_score=int(np.median(scores[:, :, :10].max(axis=2))), iou=(1, 3), max_det=WINDOWS)
    dets, counts, ncand = detect_clip(L, clip, 10, o)
    want = detect_ref.detect(boxes, scores[:, :, :10], **o)
    print(params, mode, "by_score 0: counts", counts.tolist(), "n_candidates", ncand.tolist())
    assert np.array_equal(dets, want[0]) and np.array_equal(counts, want[1]) and np.array_equal(ncand, want[2])
    assert 0 < counts.min() and (counts < ncand).any()
    for f in range(FRAMES):  # the restated decode rule is scan_clip's
        d = dets[f, :counts[f]]
        assert (d[:, 4] == classes[f][d[:, 6]]).all()
    # ... for EVERY window: no threshold, nothing suppressed, every window kept
    everything = dc.options((1 << 10) - 1, iou=(1, 1), max_det=WINDOWS)
    dets, counts, _ = detect_clip(L, clip, 10, everything)
    assert counts.tolist() == [WINDOWS] * FRAMES
    for f in range(FRAMES):
        assert sorted(dets[f, :, 6].tolist()) == list(range(WINDOWS)) and (dets[f, :, 4] == classes[f][dets[f, :, 6]]).all()
    assert np.array_equal(dets, detect_ref.detect(boxes, scores[:, :, :10], **everything)[0])
    # by_score = 1, one class, with a threshold
    k = int(np.bincount(classes.ravel()).argmax())
    o = dc.options(1 << k, by_score=1, min_score=int(np.median(scores[:, :, k])), iou=(1, 2), max_det=32, max_candidates=64)
    dets, counts, ncand = detect_clip(L, clip, 10, o)
    want = detect_ref.detect(boxes, scores[:, :, :10], **o)
    assert np.array_equal(dets, want[0]) and np.array_equal(counts, want[1]) and np.array_equal(ncand, want[2])
    # by_score = 1 without a threshold: every window is a candidate and the geometry decides, whatever the data
    every = dc.options(1 << k, by_score=1, min_score=-32769, max_det=WINDOWS)
    dets, counts, ncand = detect_clip(L, clip, 10, dict(every, iou=(7, 9)))
    assert counts.tolist() == [WINDOWS] * FRAMES and ncand.tolist() == [WINDOWS] * FRAMES
    assert np.array_equal(dets, detect_ref.detect(boxes, scores[:, :, :10], **dict(every, iou=(7, 9)))[0])
    for iou in ((50971, 65536), (1, 2)):
        dets, counts, ncand = detect_clip(L, clip, 10, dict(every, iou=iou))
        print(params, mode, "iou", iou, "counts", counts.tolist())
        assert (counts < WINDOWS).all() and (counts > 0).all() and ncand.tolist() == [WINDOWS] * FRAMES
        assert np.array_equal(dets, detect_ref.detect(boxes, scores[:, :, :10], **dict(every, iou=iou))[0])


def test_clip_refusals(L, param_dirs):
    L.load_parameters(param_dirs["cifar10"].encode())
    clip = clip_of("RGB")
    o = dc.options(0b1, max_det=8)
    for change, word in ((dict(class_mask=0), "class_mask"), (dict(class_mask=1 << 10), "class_mask"), (dict(iou=(3, 2)), "iou_num"),
                         (dict(max_candidates=5000), "max_candidates")):
        rc, msg = detect_clip(L, clip, 10, dict(o, **change), raw=True)
        assert rc == -1 and msg.startswith("detect_clip: ") and word in msg, msg
    # what scan_clip refuses, in its words: a window size that is no multiple of 8
    sz = np.asarray([33], np.int32)
    boxes = np.zeros((WINDOWS, 4), np.int32)
    assert not L.bnn_mi355x_scan_clip(clip.ctypes.data, FRAMES, 0, W, H, 3, 0, sz.ctypes.data, 1, 10, boxes.ctypes.data, None, None, 0)
    scan_msg = err(L)
    rc, msg = detect_clip(L, clip, 10, o, raw=True, sizes=(33,))
    assert rc == -1 and msg == scan_msg.replace("scan_clip", "detect_clip", 1), (msg, scan_msg)


# ---- 3. the Python routes ---------------------------------------------------------------------------------------------------
def as_dets(found, max_det):
    """what CnvClassifier returns, as (box, class, score) rows"""
    return [[list(b) + [c, s] for b, c, s in frame] for frame in found]


def ref_dets(boxes, scores, o):
    dets, counts, _ = detect_ref.detect(boxes, scores, **o)
    return [[d[:6].tolist() for d in dets[f, :counts[f]]] for f in range(len(counts))]


def test_python_detect_clip_detect_and_suppress():
    import bnn
    clf = bnn.CnvClassifier(bnn.NETWORK_CNVW1A1, "cifar10", bnn.RUNTIME_SW)
    clip = clip_of("RGB", seed=9)
    boxes, scores = clf.scan_clip(clip, sizes=SIZES, details=True)
    cut = int(np.median(scores.max(axis=2)))
    o = dc.options((1 << len(clf.classes)) - 1, min_score=cut, iou=(32768, 65536), max_det=64)
    want = ref_dets(boxes, scores, o)
    one = clf.detect_clip(clip, sizes=SIZES, min_score=cut)
    assert as_dets(one, 64) == want and any(want)
    assert clf.usecDetect > 0 and len(clf.n_candidates) == FRAMES
    assert clf.detect_clip(list(clip), sizes=SIZES, min_score=cut, max_frames=2) == one
    assert clf.detect(clip[0], sizes=SIZES, min_score=cut) == one[0]
    # suppress on the scan's own scores is the same answer, and one frame returns one list
    assert clf.suppress(boxes, scores, min_score=cut) == one
    assert clf.suppress(boxes, scores[1], min_score=cut) == one[1]
    # RGBA frames take scan_clip(details=True) + detect_windows
    rgba = [np.dstack([f, np.full(f.shape[:2], 255, np.uint8)]) for f in clip]
    assert clf.detect_clip(rgba, sizes=SIZES, min_score=cut) == one
    # one class by score, an exact IoU
    got = clf.detect_clip(clip, 3, sizes=SIZES, by_score=True, iou=(1, 3), max_det=WINDOWS)
    assert as_dets(got, WINDOWS) == ref_dets(boxes, scores, dc.options(1 << 3, by_score=1, iou=(1, 3), max_det=WINDOWS))
    with pytest.raises(RuntimeError, match="class_mask"):
        clf.detect_clip(clip, [len(clf.classes)], sizes=SIZES)


def test_other_networks_refuse_the_clip_and_fall_back():
    """cnvW1A2 on a 48 x 40 clip, sizes (32,): 5 x 3 = 15 windows a frame"""
    import bnn
    clf = bnn.CnvClassifier(bnn.NETWORK_CNVW1A2, "cifar10", bnn.RUNTIME_SW)
    L = clf.bnn.interface
    clip = np.random.default_rng(77).integers(0, 256, (2, 40, 48, 3), dtype=np.uint8)
    assert len(scan_ref.boxes(48, 40, 32)) == 15
    o = dc.options(0b1111111111, max_det=15)
    rc, msg = detect_clip(L, clip, 10, o, raw=True, size=(48, 40), sizes=(32,))
    assert rc == -1 and "detect_clip: the dense scan is built for cnvW1A1 only" in msg, msg
    boxes, scores = clf.scan_clip(clip, sizes=(32,), details=True)
    got = clf.detect_clip(clip, sizes=(32,), iou=(1, 4), max_det=15)
    assert as_dets(got, 15) == ref_dets(boxes, scores, dict(o, iou=(1, 4)))
    assert sum(len(g) for g in got) > 0


# ---- 4. workspaces ----------------------------------------------------------------------------------------------------------
def test_deinit_between_two_identical_calls():
    L = gl.Net("cnvW1A1", "cifar10").L
    clip = clip_of("RGB", seed=5)
    o = dc.options(0b1111111111, min_score=250, iou=(1, 3), max_det=WINDOWS)
    _, boxes, scores, wo = next(c for c in dc.edge_cases() if c[0] == "edge_n257_f3_c16")

    def run():
        return [x.tobytes() for x in detect_clip(L, clip, 10, o) + dc.call(L, DEVICE, boxes, scores, wo)]

    before = run()
    L.deinit()
    after = run()
    L.deinit()
    assert before == after
    assert err(L) == ""
