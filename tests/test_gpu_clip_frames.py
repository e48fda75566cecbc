"""GPU: the clip entry points on camera frames (bnn_mi355x_scan_clip_frames / _detect_clip_frames from host memory,
bnn_mi355x_scan_clip_device / _detect_clip_device from HBM; CnvClassifier.scan_clip / detect_clip with pixel_format;
DESIGN.md 9 "Camera frames").

Everything is exact and the oracle is the code that exists: a clip of NV12, I420, YUYV or BGR frames must give what
bnn_mi355x_scan_clip / bnn_mi355x_detect_clip give on the RGB frames tests/pixfmt_ref.py makes of the same bytes -- all 64
raw scores of every window, and dets, counts and n_candidates.  The shapes are test_gpu_scan_clip.py's smallest: 3 frames
of 100 x 52 with sizes (32, 40) (147 windows a frame) and the one-window clip of 32 x 32.  cnvW1A1 with the shipped
road-signs parameters and a random set."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import detect_cases as dc
import gpu_lib as gl
import oracle_lib as ol
import pixfmt_cases as pc
import pixfmt_ref as ref
import scan_ref

sys.path.insert(0, os.path.join(gl.ROOT, "bnn-pynq_amd"))

pytestmark = pytest.mark.gpu

RAW = ["nv12", "i420", "yuyv", "bgr"]
SHAPES = {"clip": (3, 100, 52, (32, 40)), "one_window": (2, 32, 32, (32,))}


@pytest.fixture(scope="module")
def param_dirs(tmp_path_factory):
    import random_params
    d = tmp_path_factory.mktemp("rp_clip_frames")
    random_params.make(str(d), "cnvW1A1", 577)
    return {"road-signs": (gl.param_dir("road-signs", "cnvW1A1"), ol.num_classes("road-signs", "cnvW1A1")), "random": (str(d), 10)}


@pytest.fixture(scope="module")
def L():
    lib = gl.load("cnvW1A1")
    yield lib
    lib.load_parameters(gl.param_dir("cifar10", "cnvW1A1").encode())  # leave the library as found


def err(L):
    return L.bnn_mi355x_last_error().decode()


def load(L, param_dirs, params):
    pdir, ncls = param_dirs[params]
    L.load_parameters(pdir.encode())
    assert err(L) == ""
    return ncls


def n_boxes(w, h, sizes):
    return sum(len(scan_ref.boxes(w, h, s)) for s in sizes)


def pointer(a):
    return a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data


def scan_old(L, clip, sizes, ncls=64, detail=True):
    """bnn_mi355x_scan_clip on RGB [F, h, w, 3] or L [F, h, w] frames -> (boxes, [F, n, ncls] scores or [F, n] classes)"""
    frames, h, w = clip.shape[:3]
    sz, n = np.asarray(sizes, np.int32), n_boxes(w, h, sizes)
    boxes = np.full((n, 4), -1, np.int32)
    p = L.bnn_mi355x_scan_clip(clip.ctypes.data, frames, 0, w, h, 1 if clip.ndim == 3 else 3, 0, sz.ctypes.data, len(sz), ncls, boxes.ctypes.data, None,
                               None, 1 if detail else 0)
    assert p, err(L)
    out = np.ctypeslib.as_array(p, shape=(frames * n * (ncls if detail else 1),)).astype(np.int32, copy=True)
    L.free_results(p)
    return boxes, (out.reshape(frames, n, ncls) if detail else out.reshape(frames, n))


def scan_new(L, fr, pixels, sizes, ncls=64, detail=True, stream=False):
    """bnn_mi355x_scan_clip_frames, or with `stream` (a handle; None is the null stream) bnn_mi355x_scan_clip_device"""
    sz, n = np.asarray(sizes, np.int32), n_boxes(fr.width, fr.height, sizes)
    boxes = np.full((n, 4), -1, np.int32)
    usec, pre = C.c_float(-1), C.c_float(-1)
    args = [C.byref(fr), pointer(pixels), sz.ctypes.data, len(sz), ncls, boxes.ctypes.data, C.byref(usec), C.byref(pre), 1 if detail else 0]
    p = L.bnn_mi355x_scan_clip_frames(*args) if stream is False else L.bnn_mi355x_scan_clip_device(*(args + [stream]))
    assert p, err(L)
    assert usec.value > 0 and pre.value > 0
    out = np.ctypeslib.as_array(p, shape=(fr.n_frames * n * (ncls if detail else 1),)).astype(np.int32, copy=True)
    L.free_results(p)
    return boxes, (out.reshape(fr.n_frames, n, ncls) if detail else out.reshape(fr.n_frames, n))


def detect_old(L, clip, sizes, ncls, o):
    frames, h, w = clip.shape[:3]
    sz = np.asarray(sizes, np.int32)
    dets = np.full((frames, o["max_det"], 8), -7, np.int32)
    counts, ncand = np.full(frames, -7, np.int32), np.full(frames, -7, np.int32)
    co = dc.c_opts(o)
    rc = L.bnn_mi355x_detect_clip(clip.ctypes.data, frames, 0, w, h, 1 if clip.ndim == 3 else 3, 0, sz.ctypes.data, len(sz), ncls, C.byref(co),
                                  dets.ctypes.data, counts.ctypes.data, ncand.ctypes.data, None, None, None)
    assert rc == 0, err(L)
    return dets, counts, ncand


def detect_new(L, fr, pixels, sizes, ncls, o, stream=False, raw=False):
    sz = np.asarray(sizes, np.int32)
    dets = np.full((fr.n_frames, o["max_det"], 8), -7, np.int32)
    counts, ncand = np.full(fr.n_frames, -7, np.int32), np.full(fr.n_frames, -7, np.int32)
    co = dc.c_opts(o)
    usec, pre, det = C.c_float(-1), C.c_float(-1), C.c_float(-1)
    args = [C.byref(fr), pointer(pixels), sz.ctypes.data, len(sz), ncls, C.byref(co), dets.ctypes.data, counts.ctypes.data, ncand.ctypes.data,
            C.byref(usec), C.byref(pre), C.byref(det)]
    rc = L.bnn_mi355x_detect_clip_frames(*args) if stream is False else L.bnn_mi355x_detect_clip_device(*(args + [stream]))
    if raw:
        return rc, err(L)
    assert rc == 0, err(L)
    assert usec.value > 0 and pre.value > 0 and det.value > 0
    return dets, counts, ncand


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def raw_clip(fmt, shape, padded=False, seed=0):
    """(bnn_mi355x_frames, the frames' bytes, the RGB frames the numpy model makes of them)"""
    frames, w, h, _ = SHAPES[shape]
    s, fs = pc.wide_strides(fmt, w, h) if padded == "wide" else (pc.padded_strides(fmt, w, h) if padded else (0, 0))
    buf = pc.random_frames(fmt, w, h, frames, s, fs, seed)
    return pc.struct(fmt, w, h, frames, s, fs), buf, ref.unpack(buf, fmt, w, h, frames, s, fs)


def detect_options(scores, ncls, windows):
    """the detection tests' choice: every class by the decode, the median of the windows' best scores, IoU 1/3, no cap"""
    return dc.options((1 << ncls) - 1, min_score=int(np.median(scores[:, :, :ncls].max(axis=2))), iou=(1, 3), max_det=windows)


# ---- 1. host memory ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", RAW)
@pytest.mark.parametrize("params", ["road-signs", "random"])
def test_raw_frames_equal_scan_clip_and_detect_clip_on_the_model_rgb(L, param_dirs, params, fmt):
    ncls = load(L, param_dirs, params)
    for shape, padded in (("clip", False), ("clip", True), ("clip", "wide"), ("one_window", False)):
        sizes = SHAPES[shape][3]
        fr, buf, rgb = raw_clip(fmt, shape, padded)
        boxes, scores = scan_old(L, rgb, sizes)
        got_boxes, got = scan_new(L, fr, buf, sizes)
        bad = np.argwhere((got != scores).any(axis=2))
        print(params, fmt, shape, "padded" if padded else "packed", "windows", scores.shape[:2], "differing", len(bad))
        assert np.array_equal(got_boxes, boxes) and len(bad) == 0, bad[:8]
        assert np.array_equal(scan_new(L, fr, buf, sizes, ncls, False)[1], scan_old(L, rgb, sizes, ncls, False)[1])
        o = detect_options(scores, ncls, scores.shape[1])
        want = detect_old(L, rgb, sizes, ncls, o)
        assert same(detect_new(L, fr, buf, sizes, ncls, o), want), (params, fmt, shape)
        if shape == "clip":  # the reference keeps at least one detection and suppresses at least one
            print("counts", want[1].tolist(), "n_candidates", want[2].tolist())
            assert want[1].sum() > 0 and (want[1] < want[2]).any()


def test_video_range_reaches_the_kernel(L, param_dirs):
    load(L, param_dirs, "random")
    frames, w, h, sizes = SHAPES["clip"]
    buf = pc.random_frames("nv12", w, h, frames, seed=4)
    rgb = ref.unpack(buf, "nv12", w, h, frames, video_range=1)
    assert (rgb != ref.unpack(buf, "nv12", w, h, frames)).any()
    assert np.array_equal(scan_new(L, pc.struct("nv12", w, h, frames, video_range=1), buf, sizes)[1], scan_old(L, rgb, sizes)[1])


@pytest.mark.parametrize("mode", ["rgb", "l"])
def test_rgb_and_l_equal_the_older_entry_points(L, param_dirs, mode):
    ncls = load(L, param_dirs, "road-signs")
    frames, w, h, sizes = SHAPES["clip"]
    clip = np.random.default_rng(31).integers(0, 256, (frames, h, w) + ((3,) if mode == "rgb" else ()), dtype=np.uint8)
    fr = pc.struct(mode, w, h, frames)
    boxes, scores = scan_old(L, clip, sizes)
    got = scan_new(L, fr, clip, sizes)
    assert np.array_equal(got[0], boxes) and np.array_equal(got[1], scores)
    o = detect_options(scores, ncls, scores.shape[1])
    assert same(detect_new(L, fr, clip, sizes, ncls, o), detect_old(L, clip, sizes, ncls, o))
    # strided RGB / L frames, as scan_clip takes them
    s, fs = pc.padded_strides(mode, w, h)
    buf = pc.random_frames(mode, w, h, frames, s, fs, seed=6)
    tight = ref.packed(buf, mode, w, h, frames, s, fs).reshape(clip.shape)
    assert np.array_equal(scan_new(L, pc.struct(mode, w, h, frames, s, fs), buf, sizes)[1], scan_old(L, tight, sizes)[1])


def test_refusals_are_the_scans(L, param_dirs):
    ncls = load(L, param_dirs, "random")
    fr, buf, rgb = raw_clip("nv12", "clip")
    o = dc.options(0b1, max_det=8)
    rc, msg = detect_new(L, fr, buf, (33,), ncls, o, raw=True)
    sz = np.asarray([33], np.int32)
    boxes = np.zeros((256, 4), np.int32)
    assert not L.bnn_mi355x_scan_clip(rgb.ctypes.data, 3, 0, 100, 52, 3, 0, sz.ctypes.data, 1, ncls, boxes.ctypes.data, None, None, 0)
    assert rc == -1 and msg == err(L).replace("scan_clip", "detect_clip_frames", 1), msg
    rc, msg = detect_new(L, fr, buf, (32,), ncls, dict(o, class_mask=0), raw=True)
    assert rc == -1 and msg.startswith("detect_clip_frames: ") and "class_mask" in msg


# ---- 2. device memory -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", RAW)
def test_a_cuda_tensor_equals_the_host_route(L, param_dirs, fmt):
    import torch
    ncls = load(L, param_dirs, "road-signs")
    # (the kernel reads the tensor where it lies: odd strides for BGR and padded ones for NV12 take its byte path, strides
    # that are multiples of 16 its wide path)
    fr, buf, rgb = raw_clip(fmt, "clip", padded=True if fmt in ("nv12", "bgr") else "wide")
    sizes = SHAPES["clip"][3]
    want = scan_new(L, fr, buf, sizes)
    o = detect_options(want[1], ncls, want[1].shape[1])
    want_dets = detect_new(L, fr, buf, sizes, ncls, o)
    t = torch.from_numpy(buf).cuda()
    before = t.clone()
    # on the current stream ...
    cur = torch.cuda.current_stream().cuda_stream
    assert same(scan_new(L, fr, t, sizes, stream=cur), want)
    assert same(detect_new(L, fr, t, sizes, ncls, o, stream=cur), want_dets)
    # ... and on a stream of the caller's own, behind work queued there
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        t2 = torch.zeros_like(t)
        t2.copy_(before, non_blocking=True)
        assert same(detect_new(L, fr, t2, sizes, ncls, o, stream=s.cuda_stream), want_dets)
        assert same(scan_new(L, fr, t2, sizes, stream=s.cuda_stream), want)
    torch.cuda.synchronize()
    assert torch.equal(t, before) and torch.equal(t2, before)


def test_a_view_at_an_odd_byte_offset(L, param_dirs):
    import torch
    load(L, param_dirs, "random")
    fr, buf, _ = raw_clip("bgr", "clip", seed=8)
    sizes = SHAPES["clip"][3]
    want = scan_new(L, fr, buf, sizes)
    base = torch.zeros(len(buf) + 1, dtype=torch.uint8, device="cuda")
    view = base[1:]
    view.copy_(torch.from_numpy(buf))
    torch.cuda.synchronize()
    assert view.data_ptr() % 2 == 1
    assert same(scan_new(L, fr, view, sizes, stream=torch.cuda.current_stream().cuda_stream), want)
    assert base[0].item() == 0 and np.array_equal(view.cpu().numpy(), buf)


@pytest.mark.parametrize("mode", ["rgb", "l"])
def test_rgb_tensors_in_place_and_strided(L, param_dirs, mode):
    import torch
    load(L, param_dirs, "road-signs")
    frames, w, h, sizes = SHAPES["clip"]
    clip = np.random.default_rng(41).integers(0, 256, (frames, h, w) + ((3,) if mode == "rgb" else ()), dtype=np.uint8)
    want = scan_old(L, clip, sizes)
    cur = torch.cuda.current_stream().cuda_stream
    t = torch.from_numpy(clip).cuda()
    assert same(scan_new(L, pc.struct(mode, w, h, frames), t, sizes, stream=cur), want)  # packed: resized where it lies
    assert np.array_equal(t.cpu().numpy(), clip)
    s, fs = pc.padded_strides(mode, w, h)
    buf = pc.random_frames(mode, w, h, frames, s, fs, seed=7)
    tight = ref.packed(buf, mode, w, h, frames, s, fs).reshape(clip.shape)
    assert same(scan_new(L, pc.struct(mode, w, h, frames, s, fs), torch.from_numpy(buf).cuda(), sizes, stream=cur), scan_old(L, tight, sizes))


def test_a_capturing_stream_is_refused_and_the_capture_stays_valid(L, param_dirs):
    import torch
    ncls = load(L, param_dirs, "random")
    fr, buf, _ = raw_clip("nv12", "clip")
    sizes = SHAPES["clip"][3]
    t = torch.from_numpy(buf).cuda()
    scan_new(L, fr, t, sizes, stream=torch.cuda.current_stream().cuda_stream)  # (every workspace exists before the capture)
    marker = torch.zeros(4, device="cuda")
    o = dc.options(0b1, max_det=8)
    sz = np.asarray(sizes, np.int32)
    boxes = np.zeros((n_boxes(100, 52, sizes), 4), np.int32)
    s, g = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=s):
        marker.add_(1)
        handle = torch.cuda.current_stream().cuda_stream
        p = L.bnn_mi355x_scan_clip_device(C.byref(fr), t.data_ptr(), sz.ctypes.data, len(sz), 64, boxes.ctypes.data, None, None, 1, handle)
        scan_msg = err(L)
        rc, det_msg = detect_new(L, fr, t, sizes, ncls, o, stream=handle, raw=True)
    # the capture ended without an error: it was still valid.  The graph is destroyed, never replayed.
    g.reset()
    torch.cuda.synchronize()
    assert not p and scan_msg.startswith("scan_clip_device: ") and "captured" in scan_msg, scan_msg
    assert rc == -1 and det_msg.startswith("detect_clip_device: ") and "captured" in det_msg, det_msg
    assert marker.sum().item() == 0
    assert same(scan_new(L, fr, t, sizes, stream=torch.cuda.current_stream().cuda_stream), scan_new(L, fr, buf, sizes))


# ---- 3. workspaces and Python -----------------------------------------------------------------------------------------------
def test_grow_only_workspaces(L, param_dirs):
    """a small clip after a larger one, and a scan_scene call in between, still give their earlier answers"""
    load(L, param_dirs, "random")
    small = raw_clip("i420", "one_window", seed=11)
    large = raw_clip("yuyv", "clip", padded=True, seed=12)
    first_small = scan_new(L, small[0], small[1], SHAPES["one_window"][3])
    first_large = scan_new(L, large[0], large[1], SHAPES["clip"][3])
    scene = np.random.default_rng(13).integers(0, 256, (60, 120, 3), dtype=np.uint8)
    sz = np.asarray([32, 48], np.int32)

    def scan_scene():
        n = n_boxes(120, 60, (32, 48))
        boxes = np.zeros((n, 4), np.int32)
        p = L.bnn_mi355x_scan_scene(scene.ctypes.data, 120, 60, 3, 0, sz.ctypes.data, 2, 64, boxes.ctypes.data, None, None, 1)
        assert p, err(L)
        out = np.ctypeslib.as_array(p, shape=(n * 64,)).astype(np.int32, copy=True)
        L.free_results(p)
        return out

    first_scene = scan_scene()
    assert same(scan_new(L, small[0], small[1], SHAPES["one_window"][3]), first_small)
    assert np.array_equal(scan_scene(), first_scene)
    assert same(scan_new(L, large[0], large[1], SHAPES["clip"][3]), first_large)
    assert same(first_small, scan_old(L, small[2], SHAPES["one_window"][3])) and same(first_large, scan_old(L, large[2], SHAPES["clip"][3]))


def test_python_routes():
    import bnn
    import torch
    frames, w, h, sizes = SHAPES["clip"]
    buf = pc.random_frames("nv12", w, h, frames, seed=21)
    nv12 = buf.reshape(frames, h * 3 // 2, w)
    rgb = ref.unpack(buf, "nv12", w, h, frames)
    clf = bnn.CnvClassifier(bnn.NETWORK_CNVW1A1, "road-signs", bnn.RUNTIME_SW)
    assert np.array_equal(clf.unpack_frames(nv12, "nv12"), rgb)
    boxes, scores = clf.scan_clip(rgb, sizes=sizes, details=True)
    cut = int(np.median(scores.max(axis=2)))
    want = clf.detect_clip(rgb, sizes=sizes, min_score=cut)
    assert any(want)
    got_boxes, got_scores = clf.scan_clip(nv12, sizes=sizes, details=True, pixel_format="nv12")
    assert np.array_equal(got_boxes, boxes) and np.array_equal(got_scores, scores)
    assert clf.detect_clip(nv12, sizes=sizes, min_score=cut, pixel_format="nv12") == want
    assert clf.detect_clip(nv12, sizes=sizes, min_score=cut, pixel_format="nv12", max_frames=2) == want
    assert clf.usecDetect > 0 and len(clf.n_candidates) == frames
    t = torch.from_numpy(nv12).cuda()
    assert clf.detect_clip(t, sizes=sizes, min_score=cut, pixel_format="nv12") == want
    assert clf.detect(t[0], sizes=sizes, min_score=cut, pixel_format="nv12") == want[0]
    assert clf.detect_clip(torch.from_numpy(rgb).cuda(), sizes=sizes, min_score=cut) == want
    assert clf.detect_clip(nv12, sizes=sizes, min_score=cut, pixel_format="nv12", video_range=True) == clf.detect_clip(
        ref.unpack(buf, "nv12", w, h, frames, video_range=1), sizes=sizes, min_score=cut)
    bgr = np.ascontiguousarray(rgb[..., ::-1])
    assert clf.detect_clip(bgr, sizes=sizes, min_score=cut, pixel_format="bgr") == want
    with pytest.raises(ValueError, match="pixel_format"):
        clf.detect_clip(nv12, sizes=sizes, pixel_format="p010")
    with pytest.raises(ValueError, match="nv12 clip"):
        clf.detect_clip(rgb, sizes=sizes, pixel_format="nv12")


def test_another_network_falls_back_to_the_host_model():
    """cnvW1A2 on a 48 x 40 clip, sizes (32,): 15 windows a frame"""
    import bnn
    import torch
    clf = bnn.CnvClassifier(bnn.NETWORK_CNVW1A2, "cifar10", bnn.RUNTIME_SW)
    buf = pc.random_frames("nv12", 48, 40, 2, seed=22)
    nv12 = buf.reshape(2, 60, 48)
    rgb = ref.unpack(buf, "nv12", 48, 40, 2)
    want = clf.detect_clip(rgb, sizes=(32,), iou=(1, 4), max_det=15)
    assert sum(len(f) for f in want) > 0
    assert clf.detect_clip(nv12, sizes=(32,), iou=(1, 4), max_det=15, pixel_format="nv12") == want
    assert clf.detect_clip(torch.from_numpy(nv12).cuda(), sizes=(32,), iou=(1, 4), max_det=15, pixel_format="nv12") == want
    boxes, scores = clf.scan_clip(rgb, sizes=(32,), details=True)
    got = clf.scan_clip(nv12, sizes=(32,), details=True, pixel_format="nv12")
    assert np.array_equal(got[0], boxes) and np.array_equal(got[1], scores)
