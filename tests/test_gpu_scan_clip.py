"""GPU: the clip scan (bnn_mi355x_scan_clip / debug_scan_clip_stage, CnvClassifier.scan_clip / locate_clip;
csrc/scan_clip_kernels.hip).

Everything is exact and the oracle is the code that exists: frame f of a clip must equal bnn_mi355x_scan_scene on frame
f, bit for bit on all 64 raw scores, and every map of every stage must equal bnn_mi355x_debug_scan_stage on that frame's
level planes.  Frames are seeded random and differ from one another, so that a kernel reading the wrong frame shows.
cnvW1A1 with the shipped cifar10 parameters, the road-signs ones and a random set."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import gpu_lib as gl
import oracle_lib as ol
import scan_clip_ref as ref
import scan_ref

PIL = pytest.importorskip("PIL")
from PIL import Image  # noqa: E402

sys.path.insert(0, os.path.join(gl.ROOT, "bnn-pynq_amd"))

pytestmark = pytest.mark.gpu

SETS = ["cifar10", "road-signs", "random"]


@pytest.fixture(scope="module")
def param_dirs(tmp_path_factory):
    import random_params
    d = tmp_path_factory.mktemp("rp_scan_clip")
    random_params.make(str(d), "cnvW1A1", 271)
    return {"cifar10": gl.param_dir("cifar10", "cnvW1A1"), "road-signs": gl.param_dir("road-signs", "cnvW1A1"), "random": str(d)}


@pytest.fixture(scope="module")
def L():
    lib = gl.load("cnvW1A1")
    yield lib
    lib.load_parameters(gl.param_dir("cifar10", "cnvW1A1").encode())  # leave the library as found


def load(L, pdir):
    L.load_parameters(pdir.encode())
    assert L.bnn_mi355x_last_error() == b"", L.bnn_mi355x_last_error()


def err(L):
    return L.bnn_mi355x_last_error().decode()


def clip_of(frames, w, h, mode="RGB", seed=0):
    """seeded random frames [F, h, w(, 3)], every frame different"""
    shape = (frames, h, w) if mode == "L" else (frames, h, w, 3)
    a = np.random.default_rng(100000 * frames + 1000 * w + h + seed).integers(0, 256, shape, dtype=np.uint8)
    assert all((a[f] != a[g]).any() for f in range(frames) for g in range(f))
    return a


def n_boxes(w, h, sizes):
    return sum(len(scan_ref.boxes(w, h, s)) for s in sizes)


def scan_scene(L, a, sizes, ncls, detail):
    """the oracle: bnn_mi355x_scan_scene on one picture"""
    sz = np.asarray(sizes, np.int32)
    n = n_boxes(a.shape[1], a.shape[0], sizes)
    boxes = np.full((n, 4), -1, np.int32)
    p = L.bnn_mi355x_scan_scene(a.ctypes.data, a.shape[1], a.shape[0], 1 if a.ndim == 2 else 3, 0, sz.ctypes.data, len(sz), ncls, boxes.ctypes.data,
                                None, None, 1 if detail else 0)
    assert p, err(L)
    out = np.ctypeslib.as_array(p, shape=(n * (ncls if detail else 1),)).astype(np.int32, copy=True)
    L.free_results(p)
    return boxes, (out.reshape(n, ncls) if detail else out)


def scan_clip(L, clip, sizes, ncls, detail, row_stride=0, frame_stride=0, shape=None):
    """bnn_mi355x_scan_clip -> (boxes [n, 4], [F, n] classes or [F, n, ncls] scores); `shape` = (F, h, w, bands) for a clip
    handed over as a strided byte buffer"""
    frames, h, w, bands = shape if shape else (clip.shape[0], clip.shape[1], clip.shape[2], 1 if clip.ndim == 3 else 3)
    sz = np.asarray(sizes, np.int32)
    n = n_boxes(w, h, sizes)
    boxes = np.full((n, 4), -1, np.int32)
    usec, pre = C.c_float(-1), C.c_float(-1)
    p = L.bnn_mi355x_scan_clip(clip.ctypes.data, frames, frame_stride, w, h, bands, row_stride, sz.ctypes.data, len(sz), ncls, boxes.ctypes.data,
                               C.byref(usec), C.byref(pre), 1 if detail else 0)
    assert p, err(L)
    assert usec.value > 0 and pre.value > 0
    out = np.ctypeslib.as_array(p, shape=(frames * n * (ncls if detail else 1),)).astype(np.int32, copy=True)
    L.free_results(p)
    return boxes, (out.reshape(frames, n, ncls) if detail else out.reshape(frames, n))


def check_against_scan_scene(L, clip, sizes, ncls, what):
    """boxes, classes and all raw scores (number_class 64) of every frame, frame-major"""
    boxes, classes = scan_clip(L, clip, sizes, ncls, False)
    boxes_d, scores = scan_clip(L, clip, sizes, 64, True)
    assert (boxes == boxes_d).all()
    for f in range(len(clip)):
        want_boxes, want_classes = scan_scene(L, clip[f], sizes, ncls, False)
        _, want_scores = scan_scene(L, clip[f], sizes, 64, True)
        assert (boxes == want_boxes).all(), what
        bad = np.argwhere((scores[f] != want_scores).any(axis=1)).ravel()
        print(what, "frame", f, "windows", len(want_scores), "differing", len(bad))
        assert len(bad) == 0, (what, "frame", f, bad[:8])
        assert (classes[f] == want_classes).all(), (what, "frame", f)
    return boxes, classes, scores


def ncls_of(params):
    return ol.num_classes(params, "cnvW1A1") if params != "random" else 10


@pytest.mark.parametrize("params", SETS)
def test_every_frame_equals_scan_scene(L, param_dirs, params):
    """3 frames of 100 x 52 RGB, sizes (32, 40): levels 100 x 52 (18 x 6 windows, not resized) and 80 x 41 (13 x 3): two
    geometries, in every stage a map boundary that is no block boundary, stage-5 maps smaller than a block"""
    load(L, param_dirs[params])
    assert [g for _, _, g in ref.levels(100, 52, (32, 40))] == [(18, 6), (13, 3)]
    check_against_scan_scene(L, clip_of(3, 100, 52), (32, 40), ncls_of(params), params)


@pytest.mark.parametrize("params", SETS)
def test_one_frame_merges_the_levels_of_a_scene(L, param_dirs, params):
    """F = 1: the merged-levels case by itself"""
    load(L, param_dirs[params])
    check_against_scan_scene(L, clip_of(1, 100, 52, seed=3), (32, 40), ncls_of(params), params)


@pytest.mark.parametrize("params", SETS)
def test_smallest_clip(L, param_dirs, params):
    """2 frames of 32 x 32, sizes (32,): two maps of one window each"""
    load(L, param_dirs[params])
    boxes, classes, _ = check_against_scan_scene(L, clip_of(2, 32, 32), (32,), ncls_of(params), params)
    assert boxes.tolist() == [[0, 0, 32, 32]] and classes.shape == (2, 1)


@pytest.mark.parametrize("params", SETS)
def test_strides(L, param_dirs, params):
    """2 frames of 50 x 41, mode L, sizes (32, 40): rows 56 bytes apart, frames 56 * 41 + 24, the padding random bytes -- the
    results of the packed clip and of scan_scene per frame"""
    load(L, param_dirs[params])
    ncls = ncls_of(params)
    clip = clip_of(2, 50, 41, mode="L")
    _, _, want = check_against_scan_scene(L, clip, (32, 40), ncls, params)
    row_stride, frame_stride = 56, 56 * 41 + 24
    buf = np.random.default_rng(5).integers(0, 256, 2 * frame_stride, dtype=np.uint8)
    for f in range(2):
        rows = buf[f * frame_stride:f * frame_stride + 41 * row_stride].reshape(41, row_stride)
        rows[:, :50] = clip[f]
    _, got = scan_clip(L, buf, (32, 40), 64, True, row_stride=row_stride, frame_stride=frame_stride, shape=(2, 41, 50, 1))
    assert (got == want).all()
    # rows packed, frames apart; rows apart, frames packed behind their rows
    apart = np.random.default_rng(6).integers(0, 256, (2, 50 * 41 + 7), dtype=np.uint8)
    apart[:, :50 * 41] = clip.reshape(2, -1)
    assert (scan_clip(L, apart, (32, 40), 64, True, frame_stride=50 * 41 + 7, shape=(2, 41, 50, 1))[1] == want).all()
    rows = np.random.default_rng(7).integers(0, 256, (2, 41, 56), dtype=np.uint8)
    rows[:, :, :50] = clip
    assert (scan_clip(L, rows, (32, 40), 64, True, row_stride=56, shape=(2, 41, 50, 1))[1] == want).all()


def level_planes(L, a, lw, lh):
    got = np.zeros((3, lh, lw), np.uint8)
    assert L.bnn_mi355x_scan_resize(a.ctypes.data, a.shape[1], a.shape[0], 1 if a.ndim == 2 else 3, 0, lw, lh, got.ctypes.data) == 0, err(L)
    return got


def scan_stage(L, planes, stage):
    _, h, w = planes.shape
    nx, ny = scan_ref.grid(w, h)
    mw, mh = ref.stage_sizes(nx, ny)[stage]
    out = np.zeros((mh, mw, scan_ref.STAGE_DWORDS[stage]), np.uint32)
    gw, gh = C.c_int(0), C.c_int(0)
    assert L.bnn_mi355x_debug_scan_stage(planes.ctypes.data, w, h, stage, out.ctypes.data, out.nbytes, C.byref(gw), C.byref(gh)) == out.nbytes, err(L)
    return out


@pytest.mark.parametrize("params", SETS)
def test_every_stage_map_of_every_frame(L, param_dirs, params):
    """the clip of the first test: for every stage 0..5 and every map, the map's slice of debug_scan_clip_stage at the
    offsets scan_clip_layout gives equals debug_scan_stage of that frame's level planes (bnn_mi355x_scan_resize); stages
    in order, so that a wrong kernel is named by the first stage that differs"""
    load(L, param_dirs[params])
    sizes, w, h, frames = (32, 40), 100, 52, 3
    clip = clip_of(frames, w, h)
    sz = np.asarray(sizes, np.int32)
    m = frames * len(sizes)
    mw, mh, off = np.zeros((m, 6), np.int32), np.zeros((m, 6), np.int32), np.zeros((m, 6), np.int64)
    buf = np.zeros(2, np.int64)
    assert L.bnn_mi355x_scan_clip_layout(w, h, sz.ctypes.data, len(sz), frames, mw.ctypes.data, mh.ctypes.data, off.ctypes.data, None, None,
                                         buf.ctypes.data) == m, err(L)
    planes = [[level_planes(L, clip[f], *scan_ref.level(w, h, s)) for s in sizes] for f in range(frames)]
    for stage in range(6):
        total = ref.layout(w, h, sizes, frames)["stage_bytes"][stage]
        out = np.zeros(total, np.uint8)
        assert L.bnn_mi355x_debug_scan_clip_stage(clip.ctypes.data, frames, 0, w, h, 3, 0, sz.ctypes.data, len(sz), stage, out.ctypes.data, total - 1) == -1
        assert L.bnn_mi355x_debug_scan_clip_stage(clip.ctypes.data, frames, 0, w, h, 3, 0, sz.ctypes.data, len(sz), stage, out.ctypes.data,
                                                  out.nbytes) == total, err(L)
        for f in range(frames):
            for k in range(len(sizes)):
                i = f * len(sizes) + k
                want = scan_stage(L, planes[f][k], stage)
                assert want.shape[:2] == (mh[i, stage], mw[i, stage])
                got = out[off[i, stage]:off[i, stage] + want.nbytes].view(np.uint32).reshape(want.shape)
                assert (got == want).all(), (params, "stage", stage, "frame", f, "size", sizes[k], int((got != want).sum()))


def test_scores_where_layers_6_and_7_take_their_matrix_forms(L, param_dirs):
    """24 frames of 96 x 64, sizes (32,): 24 x 153 = 3 672 windows, past the edge (3 072 images) from which run_cnv takes
    layers 6 and 7 to the matrix pipe -- the clip enters the existing pass at stage 6 ONCE, with all its windows"""
    load(L, param_dirs["cifar10"])
    clip = clip_of(24, 96, 64)
    assert n_boxes(96, 64, (32,)) == 153
    if not os.environ.get("BNN_MI355X_CONV") and not os.environ.get("BNN_MI355X_TAIL_MFMA_MIN"):
        assert L.bnn_mi355x_matrix_stages(24 * 153) & 0xC0 == 0xC0
    _, scores = scan_clip(L, clip, (32,), 64, True)
    for f in range(24):
        assert (scores[f] == scan_scene(L, clip[f], (32,), 64, True)[1]).all(), f


def test_grow_only_workspaces(L, param_dirs):
    """a small clip, a larger one, the first again: the same answers as the first time; a scan_scene call in between still
    gives its own"""
    load(L, param_dirs["road-signs"])
    ncls = ncls_of("road-signs")
    small, big = clip_of(2, 44, 40, seed=1), clip_of(5, 168, 120, seed=2)
    first = scan_clip(L, small, (32,), 64, True)[1]
    scene = scan_scene(L, big[0], (96, 32), 64, True)[1]
    big_scores = scan_clip(L, big, (96, 32), 64, True)[1]
    assert (big_scores[0] == scene).all()
    assert (scan_scene(L, big[0], (96, 32), 64, True)[1] == scene).all()
    assert (scan_clip(L, small, (32,), 64, True)[1] == first).all()
    for f in range(2):
        assert (first[f] == scan_scene(L, small[f], (32,), 64, True)[1]).all()
    assert (scan_clip(L, big, (96, 32), ncls, False)[1][4] == scan_scene(L, big[4], (96, 32), ncls, False)[1]).all()


def test_python_scan_clip_and_locate_clip():
    """CnvClassifier.scan_clip / locate_clip: the arrays' shapes, the C entry point's answers, max_frames, the per-frame
    locate(dense=True); a cnvW1A2 classifier returns what the loop over scan_scene returns"""
    import bnn
    clf = bnn.CnvClassifier(bnn.NETWORK_CNVW1A1, "cifar10", bnn.RUNTIME_SW)
    L = clf.bnn.interface
    ncls = len(clf.classes)
    sizes = (64, 48)
    clip = clip_of(5, 80, 72, seed=4)
    want_boxes, want = scan_clip(L, clip, sizes, ncls, False)
    boxes, res = clf.scan_clip(clip, sizes=sizes)
    assert res.shape == (5, len(want_boxes)) and (boxes == want_boxes).all() and (res == want).all()
    assert clf.usecPerImage > 0 and clf.usecPreprocess > 0
    _, det = clf.scan_clip([Image.fromarray(f) for f in clip], sizes=sizes, details=True)
    assert det.shape == (5, len(want_boxes), ncls) and (det == scan_clip(L, clip, sizes, ncls, True)[1]).all()
    b2, r2 = clf.scan_clip(list(clip), sizes=sizes, max_frames=2)
    assert (b2 == boxes).all() and (r2 == res).all()
    grey = clip_of(2, 50, 41, mode="L")
    assert (clf.scan_clip(grey, sizes=(32, 40))[1] == np.stack([clf.scan_scene(g, sizes=(32, 40))[1] for g in grey])).all()
    # RGBA frames take the loop over scan_scene (its host route): the same answers
    rgba = [np.dstack([f, np.full(f.shape[:2], 255, np.uint8)]) for f in clip[:2]]
    assert (clf.scan_clip(rgba, sizes=sizes)[1] == res[:2]).all()
    k = int(np.bincount(want.ravel()).argmax())
    assert clf.locate_clip(clip, k, sizes=sizes) == [clf.locate(f, k, sizes=sizes, dense=True) for f in clip]
    cut = int(np.median(det[:, :, k]))
    assert clf.locate_clip(clip, k, sizes=sizes, min_score=cut) == [clf.locate(f, k, sizes=sizes, min_score=cut, dense=True) for f in clip]
    with pytest.raises(ValueError):
        clf.scan_clip([clip[0], clip[1][:40]], sizes=sizes)
    other = bnn.CnvClassifier(bnn.NETWORK_CNVW1A2, "cifar10", bnn.RUNTIME_SW)
    ob, ores = other.scan_clip(clip[:2], sizes=sizes)
    loop = [other.scan_scene(f, sizes=sizes) for f in clip[:2]]
    assert (ob == loop[0][0]).all() and (ores == np.stack([r for _, r in loop])).all() and ores.shape == (2, len(want_boxes))


@pytest.mark.parametrize("network, dataset, what", [("cnvW1A2", "cifar10", "built for cnvW1A1 only"), ("lfcW1A1", "mnist", "CNV networks only")])
def test_other_networks_refuse_with_parameters_loaded(network, dataset, what):
    net = gl.Net(network, dataset)
    clip = clip_of(2, 40, 40)
    one = np.array([32], np.int32)
    boxes = np.zeros((16, 4), np.int32)
    assert not net.L.bnn_mi355x_scan_clip(clip.ctypes.data, 2, 0, 40, 40, 3, 0, one.ctypes.data, 1, 10, boxes.ctypes.data, None, None, 0)
    assert what in net.L.bnn_mi355x_last_error().decode()
    assert net.L.bnn_mi355x_debug_scan_clip_stage(clip.ctypes.data, 2, 0, 40, 40, 3, 0, one.ctypes.data, 1, 0, boxes.ctypes.data, boxes.nbytes) == -1
    assert what in net.L.bnn_mi355x_last_error().decode()
