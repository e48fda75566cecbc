"""GPU: the fine clip scan (bnn_mi355x_scan_clip_fine / debug_scan_clip_fine_stage, CnvClassifier.scan_clip(stride=2);
csrc/scan_phase_kernels.hip, DESIGN.md 9 "Fine scan").

Everything is exact and the oracle is the code that exists: the windows of phase (px, py) of a level must equal, on all 64
raw scores, bnn_mi355x_scan_clip at size 32 on the level picture (the frame, or Pillow's LANCZOS resize of it) cropped at
[2py:, 2px:]; the smallest cases also equal bnn_mi355x_inference_raw on the cut records.  Frames are seeded random and differ
from one another.  Band constants of k_clip_conv_phase: stage 2 bands are 16 rows x 64 columns, stage 3 bands lie 15 rows and
62 columns apart."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import gpu_lib as gl

PIL = pytest.importorskip("PIL")
from PIL import Image  # noqa: E402

sys.path.insert(0, os.path.join(gl.ROOT, "bnn-pynq_amd"))

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def param_dirs(tmp_path_factory):
    import random_params
    d = tmp_path_factory.mktemp("rp_scan_fine")
    random_params.make(str(d), "cnvW1A1", 613)
    return {"cifar10": gl.param_dir("cifar10", "cnvW1A1"), "random": str(d)}


@pytest.fixture(scope="module")
def L():
    lib = gl.load("cnvW1A1")
    yield lib
    lib.load_parameters(gl.param_dir("cifar10", "cnvW1A1").encode())  # leave the library as found


def err(L):
    return L.bnn_mi355x_last_error().decode()


def clip_of(frames, w, h, mode):
    shape = (frames, h, w) if mode == "L" else (frames, h, w, 3)
    a = np.random.default_rng(100000 * frames + 1000 * w + h).integers(0, 256, shape, dtype=np.uint8)
    assert all((a[f] != a[g]).any() for f in range(frames) for g in range(f))
    return a


def scan(L, entry, clip, sizes, n):
    """a clip entry point with all 64 raw scores -> (boxes [n, 4], scores [F, n, 64])"""
    frames, h, w = clip.shape[:3]
    sz, boxes = np.asarray(sizes, np.int32), np.full((n, 4), -1, np.int32)
    usec = C.c_float(-1)
    p = entry(clip.ctypes.data, frames, 0, w, h, 1 if clip.ndim == 3 else 3, 0, sz.ctypes.data, len(sz), 64, boxes.ctypes.data, C.byref(usec), None, 1)
    assert p, err(L)
    assert usec.value > 0
    out = np.ctypeslib.as_array(p, shape=(frames * n * 64,)).astype(np.int32, copy=True)
    L.free_results(p)
    return boxes, out.reshape(frames, n, 64)


def level_clip(clip, size):
    """the level pictures of every frame: the frames at size 32, else Pillow's LANCZOS resize"""
    h, w = clip.shape[1:3]
    if size == 32:
        return clip
    return np.stack([np.asarray(Image.fromarray(f).resize((w * 32 // size, h * 32 // size), Image.LANCZOS)) for f in clip])


def phases_of(level):
    """(px, py, the level cropped for that phase) for the phases that have windows, in result order"""
    return [(px, py, np.ascontiguousarray(level[:, 2 * py:, 2 * px:])) for py in (0, 1) for px in (0, 1)
            if level.shape[2] - 2 * px >= 32 and level.shape[1] - 2 * py >= 32]


def reference(L, clip, sizes):
    """(boxes, scores [F, n, 64]) from bnn_mi355x_scan_clip on the cropped levels, and the level positions [n, 2] of the windows"""
    boxes, scores, at = [], [], []
    for s in sizes:
        for px, py, crop in phases_of(level_clip(clip, s)):
            nx, ny = (crop.shape[2] - 32) // 4 + 1, (crop.shape[1] - 32) // 4 + 1
            scores.append(scan(L, L.bnn_mi355x_scan_clip, crop, (32,), nx * ny)[1])
            ij = np.stack(np.meshgrid(2 * np.arange(nx) + px, 2 * np.arange(ny) + py), axis=-1).reshape(-1, 2)
            boxes.append(np.concatenate([ij * s // 16, ij * s // 16 + s], axis=1))
            at.append(2 * ij)
    return np.concatenate(boxes).astype(np.int32), np.concatenate(scores, axis=1), np.concatenate(at)


CASES = [  # w, h, mode, frames, sizes, (scan_form, scan_stage0_form) or None
    (32, 32, "RGB", 1, (32,), None),    # one window; three phases are empty
    (36, 34, "RGB", 2, (32,), None),    # nx2 = 3, ny2 = 2: four phases of 2, 1, 2 and 1 windows
    (35, 37, "L", 2, (32,), None),      # an unused last column, ny2 = 3
    (140, 48, "RGB", 2, (32,), None),   # stage 3 conv 64 x 18: a second band of 2 columns and 3 rows; stage 2 66 x 20
    (140, 48, "RGB", 2, (32,), (0, 0)),
    (140, 48, "RGB", 2, (32,), (2, 1)),
    (139, 75, "L", 1, (32,), None),     # stage 3 conv 63 x 31: column 62 and row 30 start nothing; stage 2 65 x 33: a last band of one row and column
    (96, 72, "RGB", 2, (32, 48), None),  # a resized level (64 x 48) and two sizes in one call
]


@pytest.mark.parametrize("params", ["cifar10", "random"])
@pytest.mark.parametrize("w,h,mode,frames,sizes,forms", CASES)
def test_every_phase_equals_the_cropped_scan(L, param_dirs, params, w, h, mode, frames, sizes, forms):
    L.load_parameters(param_dirs[params].encode())
    assert err(L) == ""
    clip = clip_of(frames, w, h, mode)
    want_boxes, want, at = reference(L, clip, sizes)
    was = (L.bnn_mi355x_scan_form(forms[0]), L.bnn_mi355x_scan_stage0_form(forms[1])) if forms else None
    try:
        boxes, got = scan(L, L.bnn_mi355x_scan_clip_fine, clip, sizes, len(want_boxes))
    finally:
        if was:
            L.bnn_mi355x_scan_form(was[0])
            L.bnn_mi355x_scan_stage0_form(was[1])
    assert (boxes == want_boxes).all()
    bad = np.argwhere((got != want).any(axis=2))
    print(w, h, mode, sizes, forms, "windows", want.shape[1], "differing", len(bad))
    assert len(bad) == 0, bad[:8]
    if w <= 36 and mode == "RGB":  # the chain anchored outside the scan code: the cut records through the per-window pass
        planes = clip.transpose(0, 3, 1, 2)
        recs = np.stack([planes[f, :, y:y + 32, x:x + 32].reshape(3072) for f in range(frames) for x, y in at])
        raw = np.zeros((len(recs), 64), np.int16)
        assert L.bnn_mi355x_inference_raw(recs.ctypes.data, len(recs), raw.ctypes.data, None, None) == 0, err(L)
        assert (got.reshape(-1, 64) == raw).all()


def test_stage_maps_equal_the_cropped_scans(L, param_dirs):
    """the stage-2 map and the four stage-3 phase maps of 139 x 75 frames, as they lie in HBM, against debug_scan_clip_stage of
    the (cropped) clips on their common extent"""
    L.load_parameters(param_dirs["random"].encode())
    clip = clip_of(2, 139, 75, "RGB")
    sz = np.asarray([32], np.int32)

    def stage(entry, c, st, shape, *phase):
        out = np.zeros((len(c),) + shape + (4,), np.uint32)
        n = entry(c.ctypes.data, len(c), 0, c.shape[2], c.shape[1], 3, 0, sz.ctypes.data, 1, st, *phase, out.ctypes.data, out.nbytes)
        assert n == out.nbytes, (n, out.nbytes, err(L))
        return out

    nx2, ny2 = (139 - 32) // 2 + 1, (75 - 32) // 2 + 1
    coarse = lambda c: ((c.shape[2] - 32) // 4 + 1, (c.shape[1] - 32) // 4 + 1)  # noqa: E731
    nx, ny = coarse(clip)
    got = stage(L.bnn_mi355x_debug_scan_clip_fine_stage, clip, 2, (ny2 + 11, nx2 + 11), 0)
    want = stage(L.bnn_mi355x_debug_scan_clip_stage, clip, 2, (2 * ny + 10, 2 * nx + 10))
    hh, ww = min(got.shape[1], want.shape[1]), min(got.shape[2], want.shape[2])
    assert (got[:, :hh, :ww] == want[:, :hh, :ww]).all()
    for px, py, crop in phases_of(clip):
        nx, ny = coarse(crop)
        got = stage(L.bnn_mi355x_debug_scan_clip_fine_stage, clip, 3, ((ny2 - py + 1) // 2 + 4, (nx2 - px + 1) // 2 + 4), 2 * py + px)
        want = stage(L.bnn_mi355x_debug_scan_clip_stage, crop, 3, (ny + 4, nx + 4))
        assert got.shape == want.shape and (got == want).all(), (px, py)


def test_refused_without_the_operand_tables(L, param_dirs, monkeypatch):
    """BNN_MI355X_CONV=valu (read at every load_parameters) leaves out the tables stages 2 and 3 run on: the two calls that
    run kernels refuse, the box rule still answers, and the tables' return brings the scan back"""
    clip, sz, out = clip_of(1, 36, 34, "RGB"), np.asarray([32], np.int32), np.zeros(1 << 16, np.uint8)
    boxes = np.zeros((6, 4), np.int32)
    monkeypatch.setenv("BNN_MI355X_CONV", "valu")
    L.load_parameters(param_dirs["cifar10"].encode())
    try:
        assert not L.bnn_mi355x_scan_clip_fine(clip.ctypes.data, 1, 0, 36, 34, 3, 0, sz.ctypes.data, 1, 64, boxes.ctypes.data, None, None, 1)
        assert "BNN_MI355X_CONV=valu leaves out" in err(L)
        assert L.bnn_mi355x_debug_scan_clip_fine_stage(clip.ctypes.data, 1, 0, 36, 34, 3, 0, sz.ctypes.data, 1, 2, 0, out.ctypes.data, out.nbytes) == -1
        assert "BNN_MI355X_CONV=valu leaves out" in err(L)
        assert L.bnn_mi355x_scan_fine_boxes(36, 34, 32, None, 0, None, None) == 6
    finally:
        monkeypatch.delenv("BNN_MI355X_CONV")
        L.load_parameters(param_dirs["cifar10"].encode())
    assert scan(L, L.bnn_mi355x_scan_clip_fine, clip, (32,), 6)[1].shape == (1, 6, 64)


def test_python_stride_2():
    """scan_clip(stride=2) equals the entry point; a cnvW1A2 classifier returns the same windows through the host route"""
    import bnn
    clf = bnn.CnvClassifier(bnn.NETWORK_CNVW1A1, "cifar10", bnn.RUNTIME_SW)
    lib = clf.bnn.interface
    clip = clip_of(2, 72, 54, "RGB")
    boxes, res = clf.scan_clip(clip, sizes=(32, 48), details=True, stride=2)
    want_boxes, want = scan(lib, lib.bnn_mi355x_scan_clip_fine, clip, (32, 48), len(boxes))
    ncls = len(clf.classes)
    assert (boxes == want_boxes).all() and (res == want[:, :, :ncls]).all()
    assert (clf.scan_scene(clip[0], sizes=(32, 48), details=True, stride=2)[1] == res[0]).all()
    hits = clf.locate_clip(clip, int(res[0].argmax(axis=1)[0]), sizes=(32, 48), stride=2)
    assert tuple(boxes[0]) in hits[0]
    assert clf.detect_clip(clip, sizes=(32, 48), stride=2) == clf.suppress(boxes, res)
    with pytest.raises(ValueError):
        clf.scan_clip(clip, stride=3)
    other = bnn.CnvClassifier(bnn.NETWORK_CNVW1A2, "cifar10", bnn.RUNTIME_SW)
    ob, ores = other.scan_clip(clip[:1], sizes=(32, 48), stride=2)
    assert (ob == boxes).all() and ores.shape == (1, len(boxes))
    (lw, lh), b48 = bnn.CnvClassifier.scan_fine_boxes((72, 54), 48)
    level = np.asarray(Image.fromarray(clip[0]).resize((lw, lh), Image.LANCZOS)).transpose(2, 0, 1)
    x, y = 2 * (int(b48[-1][0]) // 3), 2 * (int(b48[-1][1]) // 3)  # the last window's level position: its box is (3I, 3J, ..) at size 48
    assert ores[0, -1] == np.asarray(other.classify_array(np.ascontiguousarray(level[:, y:y + 32, x:x + 32]).reshape(1, 3072)))[0]
