"""GPU: the dense scan (bnn_mi355x_scan_planes / scan_device / scan_scene / debug_scan_stage / scan_resize,
CnvClassifier.scan / scan_scene / locate(dense=True); csrc/scan_kernels.hip).

The oracle is in the tree: a 32 x 32 window is pasted unresampled, so window (i, j) of a scan must equal, bit for bit on
all 64 raw scores, what the per-window pass returns for the record cut at columns 4i .. 4i + 31, rows 4j .. 4j + 31 --
bnn_mi355x_inference_raw on the cut records, the CPU restatement (oracle/) on two shapes, bnn_mi355x_debug_stage_output
stage by stage, and the merged public route classify_windows with 32 x 32 boxes at stride 4.  The resize is compared
with Pillow itself.  cnvW1A1 with the shipped cifar10 parameters, the road-signs ones and a random set."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import gpu_lib as gl
import oracle_lib as ol
import scan_ref

PIL = pytest.importorskip("PIL")
from PIL import Image  # noqa: E402

sys.path.insert(0, os.path.join(gl.ROOT, "bnn-pynq_amd"))

pytestmark = pytest.mark.gpu

# shape -> what it pins (the grid in brackets)
SHAPES = [(32, 32),    # one window (1 x 1)
          (36, 32),    # tells the x stride from the y stride (2 x 1)
          (32, 36),    # ... and the y stride from the x stride (1 x 2)
          (35, 38),    # the ignored margin (1 x 2)
          (44, 40),    # a grid in both directions (4 x 3)
          (100, 52),   # rows longer than a wave, odd L4 / L5 sizes (18 x 6)
          (96, 64)]    # more than one block per layer (17 x 9)
ORACLE_SHAPES = [(36, 32), (44, 40)]
SETS = ["cifar10", "road-signs", "random"]


@pytest.fixture(scope="module")
def param_dirs(tmp_path_factory):
    import random_params
    d = tmp_path_factory.mktemp("rp_scan")
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


def planes_of(w, h, seed=0):
    """seeded random uint8 planes [3, h, w]"""
    return np.random.default_rng(1000 * w + h + seed).integers(0, 256, (3, h, w), dtype=np.uint8)


def stride4_boxes(w, h):
    nx, ny = scan_ref.grid(w, h)
    return np.array([(4 * i, 4 * j, 4 * i + 32, 4 * j + 32) for j in range(ny) for i in range(nx)], np.int32)


def raw_scores(L, records):
    out = np.zeros((len(records), 64), np.int16)
    usec = C.c_float(0)
    assert L.bnn_mi355x_inference_raw(records.ctypes.data, len(records), out.ctypes.data, None, C.byref(usec)) == 0, err(L)
    return out


def scan_planes(L, planes, ncls, detail):
    _, h, w = planes.shape
    planes = np.ascontiguousarray(planes)
    nx, ny, usec = C.c_int(0), C.c_int(0), C.c_float(0)
    p = L.bnn_mi355x_scan_planes(planes.ctypes.data, w, h, ncls, C.byref(nx), C.byref(ny), C.byref(usec), 1 if detail else 0)
    assert p, err(L)
    assert (nx.value, ny.value) == scan_ref.grid(w, h)
    n = nx.value * ny.value
    out = np.ctypeslib.as_array(p, shape=(n * (ncls if detail else 1),)).astype(np.int32, copy=True)
    L.free_results(p)
    return out.reshape(n, ncls) if detail else out


def classify_windows(L, picture, boxes, ncls, detail):
    picture = np.ascontiguousarray(picture)
    bands = 1 if picture.ndim == 2 else picture.shape[2]
    p = L.bnn_mi355x_classify_windows(picture.ctypes.data, picture.shape[1], picture.shape[0], bands, 0, boxes.ctypes.data, len(boxes), ncls, None,
                                      None, 1 if detail else 0)
    assert p, err(L)
    out = np.ctypeslib.as_array(p, shape=(len(boxes) * (ncls if detail else 1),)).astype(np.int32, copy=True)
    L.free_results(p)
    return out.reshape(len(boxes), ncls) if detail else out


def scan_stage(L, planes, stage):
    _, h, w = planes.shape
    planes = np.ascontiguousarray(planes)
    nx, ny = scan_ref.grid(w, h)
    mw, mh = scan_ref.map_sizes(nx)[stage], scan_ref.map_sizes(ny)[stage]
    out = np.zeros((mh, mw, scan_ref.STAGE_DWORDS[stage]), np.uint32)
    gw, gh = C.c_int(0), C.c_int(0)
    assert L.bnn_mi355x_debug_scan_stage(planes.ctypes.data, w, h, stage, out.ctypes.data, out.nbytes, C.byref(gw), C.byref(gh)) == out.nbytes, err(L)
    assert (gw.value, gh.value) == (mw, mh)
    return out


def record_stage(L, records, stage):
    side, dw = scan_ref.STAGE_SIDE[stage], scan_ref.STAGE_DWORDS[stage]
    out = np.zeros((len(records), side, side, dw), np.uint32)
    assert L.bnn_mi355x_debug_stage_output(records.ctypes.data, len(records), stage, out.ctypes.data, out.nbytes) == side * side * dw * 4, err(L)
    return out


@pytest.mark.parametrize("params", SETS)
def test_scores_equal_the_per_window_pass(L, param_dirs, params):
    """all 64 raw scores of every window of every shape; two shapes also against the CPU restatement"""
    load(L, param_dirs[params])
    oracle = ol.Oracle("cnvW1A1", param_dirs[params])
    for w, h in SHAPES:
        planes = planes_of(w, h)
        records = scan_ref.cut_records(planes)
        got = scan_planes(L, planes, 64, True)
        want = raw_scores(L, records)
        bad = np.argwhere((got != want).any(axis=1)).ravel()
        print(params, (w, h), "windows", len(records), "differing", len(bad))
        assert got.shape == want.shape and len(bad) == 0, (params, w, h, bad[:8])
        if (w, h) in ORACLE_SHAPES:
            assert (got == np.asarray(oracle.scores_fast(records))).all(), (params, w, h)
    oracle.close()


def test_scores_where_layers_6_and_7_take_their_matrix_forms(L, param_dirs):
    """288 x 256: 65 x 57 = 3 705 windows, past the edge (3 072 images) from which run_cnv takes layers 6 and 7 to the matrix
    pipe -- the scan enters the existing pass at stage 6 and inherits its policy"""
    load(L, param_dirs["cifar10"])
    planes = planes_of(288, 256)
    records = scan_ref.cut_records(planes)
    assert len(records) == 3705
    if not os.environ.get("BNN_MI355X_CONV") and not os.environ.get("BNN_MI355X_TAIL_MFMA_MIN"):
        assert L.bnn_mi355x_matrix_stages(len(records)) & 0xC0 == 0xC0
    assert (scan_planes(L, planes, 64, True) == raw_scores(L, records)).all()


@pytest.mark.parametrize("params", SETS)
def test_every_stage_map_holds_the_windows_maps(L, param_dirs, params):
    """stages 0-5: window (i, j)'s slice of the picture's map -- from (4i, 4j) in layer 0's, (2i, 2j) in layer 1's and 2's,
    (i, j) from layer 3 on -- equals that window's own map.  Every window of 44 x 40, the corner windows of 100 x 52."""
    load(L, param_dirs[params])
    for (w, h), corners_only in (((44, 40), False), ((100, 52), True)):
        planes = planes_of(w, h, seed=5)
        nx, ny = scan_ref.grid(w, h)
        cells = [(i, j) for j in range(ny) for i in range(nx) if not corners_only or (i in (0, nx - 1) and j in (0, ny - 1))]
        records = scan_ref.cut_records(planes)[[j * nx + i for i, j in cells]]
        for stage in range(6):
            whole = scan_stage(L, planes, stage)
            per_window = record_stage(L, records, stage)
            sc, side = scan_ref.STAGE_SCALE[stage], scan_ref.STAGE_SIDE[stage]
            for k, (i, j) in enumerate(cells):
                piece = whole[sc * j:sc * j + side, sc * i:sc * i + side]
                assert (piece == per_window[k]).all(), (params, w, h, "stage", stage, "window", (i, j), int((piece != per_window[k]).sum()))


@pytest.mark.parametrize("params", SETS)
def test_classes_equal_classify_windows_and_the_device_form(L, param_dirs, params):
    """scan_planes without detail == classify_windows with 32 x 32 boxes at stride 4 (the merged public route);
    scan_device on a torch tensor returns the same classes, and the scan's scores"""
    import torch
    load(L, param_dirs[params])
    ncls = ol.num_classes(params, "cnvW1A1") if params != "random" else 10
    for w, h in SHAPES:
        planes = planes_of(w, h, seed=9)
        got = scan_planes(L, planes, ncls, False)
        want = classify_windows(L, planes.transpose(1, 2, 0), stride4_boxes(w, h), ncls, False)
        assert (got == want).all(), (params, w, h)
        d_planes = torch.from_numpy(planes).cuda()
        d_classes = torch.full((len(got),), -1, dtype=torch.int32, device="cuda")
        d_scores = torch.zeros((len(got), 64), dtype=torch.int16, device="cuda")
        stream = torch.cuda.current_stream()
        assert L.bnn_mi355x_scan_device(d_planes.data_ptr(), w, h, ncls, d_classes.data_ptr(), d_scores.data_ptr(), stream.cuda_stream) == 0, err(L)
        stream.synchronize()
        assert (d_classes.cpu().numpy() == got).all(), (params, w, h)
        assert (d_scores.cpu().numpy()[:, :ncls] == scan_planes(L, planes, ncls, True)).all(), (params, w, h)


def pillow_planes(a, size):
    """Image.resize(size, LANCZOS) of a picture, as planar [3, h, w] (L: the grey plane three times)"""
    r = np.asarray(Image.fromarray(a).resize(size, Image.LANCZOS))
    return np.ascontiguousarray(np.broadcast_to(r[None], (3,) + r.shape) if r.ndim == 2 else r.transpose(2, 0, 1))


@pytest.mark.parametrize("w, h, mode, out_w, out_h", [(80, 72, "RGB", 40, 36), (80, 72, "RGB", 53, 48), (50, 41, "L", 33, 32),
                                                       (40, 40, "RGB", 53, 53), (48, 40, "RGB", 48, 40)])
def test_resize_equals_pillow(L, w, h, mode, out_w, out_h):
    """a level's picture, byte for byte: two shrinking levels, an L picture, one enlargement (40 x 40 with size 24), and a
    level of the picture's own size (re-laid out only)"""
    a = np.random.default_rng(w + h).integers(0, 256, (h, w) if mode == "L" else (h, w, 3), dtype=np.uint8)
    got = np.zeros((3, out_h, out_w), np.uint8)
    assert L.bnn_mi355x_scan_resize(a.ctypes.data, w, h, 1 if mode == "L" else 3, 0, out_w, out_h, got.ctypes.data) == 0, err(L)
    want = pillow_planes(a, (out_w, out_h))
    assert (got == want).all(), int((got != want).sum())
    if (out_w, out_h) == (53, 53):
        assert scan_ref.level(40, 40, 24) == (53, 53)


def scan_scene(L, a, sizes, ncls, detail):
    sz = np.asarray(sizes, np.int32)
    n = sum(len(scan_ref.boxes(a.shape[1], a.shape[0], s)) for s in sizes)
    boxes = np.full((n, 4), -1, np.int32)
    usec, pre = C.c_float(0), C.c_float(0)
    p = L.bnn_mi355x_scan_scene(a.ctypes.data, a.shape[1], a.shape[0], 1 if a.ndim == 2 else 3, 0, sz.ctypes.data, len(sz), ncls, boxes.ctypes.data,
                                C.byref(usec), C.byref(pre), 1 if detail else 0)
    assert p, err(L)
    out = np.ctypeslib.as_array(p, shape=(n * (ncls if detail else 1),)).astype(np.int32, copy=True)
    L.free_results(p)
    return boxes, (out.reshape(n, ncls) if detail else out)


def scene_by_windows(L, a, sizes, ncls, detail):
    """the route a user has without the scan: Pillow's level pictures, classify_windows with 32 x 32 boxes at stride 4"""
    res = []
    for s in sizes:
        lw, lh = scan_ref.level(a.shape[1], a.shape[0], s)
        level = np.asarray(Image.fromarray(a).resize((lw, lh), Image.LANCZOS))
        res.append(classify_windows(L, level, stride4_boxes(lw, lh), ncls, detail))
    return np.concatenate(res)


@pytest.mark.parametrize("params", SETS)
def test_scan_scene(L, param_dirs, params):
    """80 x 72 RGB, sizes (64, 48): the boxes of the restatement; classes and scores of classify_windows on Pillow's level
    pictures, size-major; the same again after a larger and a smaller picture (grow-only workspaces); an L picture"""
    load(L, param_dirs[params])
    ncls = ol.num_classes(params, "cnvW1A1") if params != "random" else 10
    sizes = (64, 48)
    a = np.random.default_rng(7).integers(0, 256, (72, 80, 3), dtype=np.uint8)
    boxes, classes = scan_scene(L, a, sizes, ncls, False)
    assert boxes.tolist() == [list(b) for s in sizes for b in scan_ref.boxes(80, 72, s)]
    assert (classes == scene_by_windows(L, a, sizes, ncls, False)).all()
    boxes_d, scores = scan_scene(L, a, sizes, ncls, True)
    assert (boxes_d == boxes).all() and (scores == scene_by_windows(L, a, sizes, ncls, True)).all()
    big = np.random.default_rng(8).integers(0, 256, (120, 168, 3), dtype=np.uint8)
    _, big_classes = scan_scene(L, big, (96, 32), ncls, False)
    assert (big_classes == scene_by_windows(L, big, (96, 32), ncls, False)).all()
    small = np.random.default_rng(9).integers(0, 256, (40, 41), dtype=np.uint8)
    _, small_scores = scan_scene(L, small, (32, 40), ncls, True)
    assert (small_scores == scene_by_windows(L, small, (32, 40), ncls, True)).all()
    again = scan_scene(L, a, sizes, ncls, True)
    assert (again[0] == boxes).all() and (again[1] == scores).all()


def test_python_scan_and_locate_dense():
    """CnvClassifier.scan / scan_scene / locate(dense=True): the arrays' shapes, the C entry points' answers, and locate
    returns exactly the boxes whose class matches (or whose score exceeds min_score)"""
    import bnn
    clf = bnn.CnvClassifier(bnn.NETWORK_CNVW1A1, "cifar10", bnn.RUNTIME_SW)
    L = clf.bnn.interface
    ncls = len(clf.classes)
    planes = planes_of(44, 40, seed=3)
    img = Image.fromarray(np.ascontiguousarray(planes.transpose(1, 2, 0)))
    records = scan_ref.cut_records(planes)
    classes = clf.scan(img)
    assert classes.shape == (3, 4) and (classes.ravel() == np.asarray(clf.classify_array(records))).all()
    scores = clf.scan(np.asarray(img), details=True)
    assert scores.shape == (3, 4, ncls) and (scores.reshape(-1, ncls) == np.asarray(clf.classify_array(records, detail=True)).reshape(-1, ncls)).all()
    a = np.random.default_rng(7).integers(0, 256, (72, 80, 3), dtype=np.uint8)
    boxes, res = clf.scan_scene(Image.fromarray(a), sizes=(64, 48))
    want_boxes, want = scan_scene(L, a, (64, 48), ncls, False)
    assert (boxes == want_boxes).all() and (res == want).all()
    _, det = clf.scan_scene(a, sizes=(64, 48), details=True)
    assert (det == scan_scene(L, a, (64, 48), ncls, True)[1]).all()
    # a mode other than RGB / L takes the host route (PIL resizes, numpy cuts, classify_array): the same answers
    rgba = np.dstack([a, np.full(a.shape[:2], 255, np.uint8)])
    assert (clf.scan_scene(Image.fromarray(rgba, "RGBA"), sizes=(64, 48))[1] == want).all()
    k = int(np.bincount(want).argmax())
    assert clf.locate(Image.fromarray(a), k, sizes=(64, 48), dense=True) == [tuple(int(v) for v in b) for b, c in zip(want_boxes, want) if c == k]
    cut = int(np.median(det[:, k]))
    assert clf.locate(a, k, sizes=(64, 48), min_score=cut, dense=True) == [tuple(int(v) for v in b) for b, s in zip(want_boxes, det) if s[k] > cut]
    # the default stays the notebook's tiling
    assert clf.locate(Image.fromarray(a), k, sizes=(64,)) == [b for b, c in zip(clf.tile_boxes((80, 72), (64,)), clf.classify_windows(Image.fromarray(a), clf.tile_boxes((80, 72), (64,)))) if c == k]


@pytest.mark.parametrize("network, dataset, what", [("cnvW1A2", "cifar10", "built for cnvW1A1 only"), ("lfcW1A1", "mnist", "CNV networks only")])
def test_other_networks_refuse_with_parameters_loaded(network, dataset, what):
    net = gl.Net(network, dataset)
    planes = planes_of(40, 40)
    nx, ny = C.c_int(0), C.c_int(0)
    assert not net.L.bnn_mi355x_scan_planes(planes.ctypes.data, 40, 40, 10, C.byref(nx), C.byref(ny), None, 0)
    assert what in net.L.bnn_mi355x_last_error().decode()
    one = np.array([32], np.int32)
    boxes = np.zeros((16, 4), np.int32)
    assert not net.L.bnn_mi355x_scan_scene(planes.ctypes.data, 40, 40, 1, 0, one.ctypes.data, 1, 10, boxes.ctypes.data, None, None, 0)
    assert what in net.L.bnn_mi355x_last_error().decode()
    assert net.L.bnn_mi355x_scan_device(planes.ctypes.data, 40, 40, 10, None, None, None) == -1
    assert what in net.L.bnn_mi355x_last_error().decode()
