"""CPU: the dense scan's host-only entry points (bnn_mi355x_scan_grid, bnn_mi355x_scan_boxes; csrc/scan.cpp) against
the plain-Python restatement tests/scan_ref.py, and every refusal that must come before anything touches a GPU.  No test
here touches a GPU: dlopen of the product library needs none, and the refused calls return before the first HIP call."""
import ctypes as C
import re

import numpy as np
import pytest

import gpu_lib as gl
import scan_ref

SIZES = (8, 32, 48, 64, 96)


@pytest.fixture(scope="module")
def L():
    return gl.load("cnvW1A1")


def err(L):
    return L.bnn_mi355x_last_error().decode()


def c_grid(L, w, h):
    nx, ny = C.c_int(-7), C.c_int(-7)
    rc = L.bnn_mi355x_scan_grid(w, h, C.byref(nx), C.byref(ny))
    return (nx.value, ny.value) if rc == 0 else None


def c_boxes(L, w, h, size):
    lw, lh = C.c_int(0), C.c_int(0)
    n = L.bnn_mi355x_scan_boxes(w, h, size, None, 0, C.byref(lw), C.byref(lh))
    if n < 0:
        return None
    out = np.full((n, 4), -1, np.int32)
    assert L.bnn_mi355x_scan_boxes(w, h, size, out.ctypes.data, n, None, None) == n
    return (lw.value, lh.value), out


def test_the_stated_limits_agree():
    with open(gl.ROOT + "/include/bnn_mi355x.h") as f:
        header = f.read()
    with open(gl.ROOT + "/bnn-pynq_amd/csrc/scan.h") as f:
        model = f.read()
    stated = {k: int(re.search(r"#define BNN_MI355X_SCAN_%s (\d+)" % k, header).group(1)) for k in ("MAX_SIDE", "MAX_WINDOWS", "MAX_MAP_BYTES")}
    assert stated == {"MAX_SIDE": scan_ref.MAX_SIDE, "MAX_WINDOWS": scan_ref.MAX_WINDOWS, "MAX_MAP_BYTES": scan_ref.MAX_MAP_BYTES}
    assert int(re.search(r"constexpr int kScanMaxSide = (\d+);", model).group(1)) == scan_ref.MAX_SIDE
    assert 1 << int(re.search(r"constexpr long kScanMaxWindows = 1L << (\d+);", model).group(1)) == scan_ref.MAX_WINDOWS
    assert 1 << int(re.search(r"constexpr size_t kScanMaxMapBytes = \(size_t\)1 << (\d+);", model).group(1)) == scan_ref.MAX_MAP_BYTES


def test_grid_and_boxes_agree_with_the_restatement(L):
    """every width and height in 32..80, sizes 8, 32, 48, 64, 96: the grid, the level, the boxes; boxes lie inside"""
    for w in range(32, 81):
        for h in range(32, 81):
            assert c_grid(L, w, h) == scan_ref.grid(w, h), (w, h)
            for s in SIZES:
                want = scan_ref.boxes(w, h, s)
                got = c_boxes(L, w, h, s)
                if want is None:
                    assert got is None, (w, h, s)
                    continue
                assert got is not None, (w, h, s, err(L))
                assert got[0] == scan_ref.level(w, h, s), (w, h, s)
                assert got[1].tolist() == [list(b) for b in want], (w, h, s)
                b = got[1]
                assert (b[:, 0] >= 0).all() and (b[:, 1] >= 0).all() and (b[:, 2] <= w).all() and (b[:, 3] <= h).all(), (w, h, s)
                assert (b[:, 2] - b[:, 0] == s).all() and (b[:, 3] - b[:, 1] == s).all()


def test_map_sizes_of_the_restatement():
    """the table of the issue: 14 + 2 (n - 1), 5 + (n - 1), n; one window gives the per-image maps of DESIGN.md 3"""
    assert scan_ref.map_sizes(1) == scan_ref.STAGE_SIDE
    for n in range(1, 40):
        s = scan_ref.map_sizes(n)
        assert s[1] == 14 + 2 * (n - 1) and s[3] == 5 + (n - 1) and s[5] == n
        assert s[0] % 2 == 0 and s[2] % 2 == 0  # the conv outputs under a pool, and layer 2's: whole 2 x 2 quads


def test_boxes_cap_and_large_levels(L):
    """fewer boxes written than there are; a 640 x 480 picture: 153 x 113 cells of 32, 73 x 53 of 64, 46 x 33 of 96"""
    out = np.full((3, 4), -1, np.int32)
    assert L.bnn_mi355x_scan_boxes(64, 48, 32, out.ctypes.data, 2, None, None) == 9 * 5
    assert out.tolist() == [[0, 0, 32, 32], [4, 0, 36, 32], [-1, -1, -1, -1]]
    for s, n in ((32, 153 * 113), (64, 73 * 53), (96, 46 * 33)):
        assert L.bnn_mi355x_scan_boxes(640, 480, s, None, 0, None, None) == n == len(scan_ref.boxes(640, 480, s))


@pytest.mark.parametrize("w, h, what", [(31, 32, "32 x 32 pixels or more"), (32, 31, "32 x 32 pixels or more"), (0, 40, "32 x 32"),
                                        (-5, 40, "32 x 32"), (8193, 32, "limit of 8192 pixels a side"), (32, 8193, "limit of 8192"),
                                        (8192, 8192, "windows, more than the limit"), (4200, 4200, "windows, more than the limit"),
                                        (4096, 4096, "bytes, more than the limit"), (4096, 2048, None), (8192, 32, None)])
def test_grid_refusals(L, w, h, what):
    got = c_grid(L, w, h)
    assert (got is not None) == scan_ref.acceptable(w, h) == (what is None), (w, h, err(L))
    if what:
        assert what in err(L) and err(L).startswith("scan_grid: "), err(L)
    else:
        assert got == scan_ref.grid(w, h)


def test_grid_null_pointers(L):
    nx = C.c_int(0)
    assert L.bnn_mi355x_scan_grid(64, 64, None, C.byref(nx)) == -1 and "null pointer" in err(L)
    assert L.bnn_mi355x_scan_grid(64, 64, C.byref(nx), None) == -1 and "null pointer" in err(L)


@pytest.mark.parametrize("w, h, size, what", [(64, 64, 0, "multiple of 8"), (64, 64, 4, "multiple of 8"), (64, 64, 36, "multiple of 8"),
                                              (64, 64, -8, "multiple of 8"), (64, 64, 72, "level below 32 x 32"), (100, 40, 48, "level below 32 x 32"),
                                              (31, 64, 32, "32 x 32 pixels or more"), (8193, 64, 32, "limit of 8192"),
                                              (4096, 4096, 8, "limit of 8192 pixels a side"), (4096, 4096, 16, "windows, more than the limit")])
def test_boxes_refusals(L, w, h, size, what):
    assert scan_ref.boxes(w, h, size) is None
    assert L.bnn_mi355x_scan_boxes(w, h, size, None, 0, None, None) == -1
    assert what in err(L) and err(L).startswith("scan_boxes: "), err(L)


def test_device_entry_points_refuse_before_the_gpu(L):
    """scan_planes / scan_device / scan_scene / debug_scan_stage / scan_resize: bad sizes, limits, null pointers and a bad
    number_class come back as -1 / NULL + last_error without a single HIP call (none could succeed on a machine without a
    GPU, and the messages name the argument, not the device)"""
    nx, ny = C.c_int(0), C.c_int(0)
    px = np.zeros(3 * 40 * 40, np.uint8)
    one = np.array([64], np.int32)
    boxes = np.zeros((64, 4), np.int32)
    assert not L.bnn_mi355x_scan_planes(px.ctypes.data, 31, 40, 10, C.byref(nx), C.byref(ny), None, 0) and "32 x 32 pixels or more" in err(L)
    assert not L.bnn_mi355x_scan_planes(None, 40, 40, 10, C.byref(nx), C.byref(ny), None, 0) and "null pointer" in err(L)
    assert not L.bnn_mi355x_scan_planes(px.ctypes.data, 40, 40, 10, None, C.byref(ny), None, 0) and "null pointer" in err(L)
    assert not L.bnn_mi355x_scan_planes(px.ctypes.data, 8200, 40, 10, C.byref(nx), C.byref(ny), None, 0) and "limit of 8192" in err(L)
    assert not L.bnn_mi355x_scan_planes(px.ctypes.data, 40, 40, 65, C.byref(nx), C.byref(ny), None, 0) and "number_class" in err(L)
    assert L.bnn_mi355x_scan_device(None, 40, 40, 10, None, None, None) == -1 and "null pointer" in err(L)
    assert L.bnn_mi355x_scan_device(px.ctypes.data, 40, 20, 10, None, None, None) == -1 and "32 x 32 pixels or more" in err(L)
    assert L.bnn_mi355x_scan_device(px.ctypes.data, 8192, 8192, 10, None, None, None) == -1 and "more than the limit" in err(L)
    assert L.bnn_mi355x_scan_device(px.ctypes.data, 40, 40, 0, None, None, None) == -1 and "number_class" in err(L)
    scene = lambda *a: L.bnn_mi355x_scan_scene(*a)  # noqa: E731
    assert not scene(px.ctypes.data, 40, 40, 3, 0, one.ctypes.data, 1, 10, boxes.ctypes.data, None, None, 0) and "level below 32 x 32" in err(L)
    assert not scene(None, 80, 72, 3, 0, one.ctypes.data, 1, 10, boxes.ctypes.data, None, None, 0) and "null pointer" in err(L)
    assert not scene(px.ctypes.data, 80, 72, 3, 0, None, 1, 10, boxes.ctypes.data, None, None, 0) and "null pointer" in err(L)
    assert not scene(px.ctypes.data, 80, 72, 3, 0, one.ctypes.data, 1, 10, None, None, None, 0) and "null pointer" in err(L)
    assert not scene(px.ctypes.data, 80, 72, 3, 0, one.ctypes.data, 0, 10, boxes.ctypes.data, None, None, 0) and "one window size or more" in err(L)
    assert not scene(px.ctypes.data, 80, 72, 4, 0, one.ctypes.data, 1, 10, boxes.ctypes.data, None, None, 0) and "bands must be 1 (L) or 3 (RGB)" in err(L)
    assert not scene(px.ctypes.data, 80, 72, 3, 100, one.ctypes.data, 1, 10, boxes.ctypes.data, None, None, 0) and "row stride shorter" in err(L)
    bad = np.array([64, 20], np.int32)
    assert not scene(px.ctypes.data, 80, 72, 3, 0, bad.ctypes.data, 2, 10, boxes.ctypes.data, None, None, 0) and "window size 20 is not a multiple of 8" in err(L)
    assert not scene(px.ctypes.data, 80, 72, 3, 0, one.ctypes.data, 1, 99, boxes.ctypes.data, None, None, 0) and "number_class" in err(L)
    mw, mh = C.c_int(0), C.c_int(0)
    out = np.zeros(16, np.uint8)
    dbg = lambda *a: L.bnn_mi355x_debug_scan_stage(*a)  # noqa: E731
    assert dbg(px.ctypes.data, 40, 40, 6, out.ctypes.data, out.size, C.byref(mw), C.byref(mh)) == -1 and "bad arguments" in err(L)
    assert dbg(px.ctypes.data, 40, 40, -1, out.ctypes.data, out.size, C.byref(mw), C.byref(mh)) == -1 and "bad arguments" in err(L)
    assert dbg(None, 40, 40, 0, out.ctypes.data, out.size, C.byref(mw), C.byref(mh)) == -1 and "bad arguments" in err(L)
    assert dbg(px.ctypes.data, 40, 40, 0, out.ctypes.data, out.size, C.byref(mw), C.byref(mh)) == -1 and "takes %d bytes" % (38 * 38 * 8) in err(L)
    assert L.bnn_mi355x_scan_resize(None, 40, 40, 3, 0, 20, 20, out.ctypes.data) == -1 and "null pointer" in err(L)
    assert L.bnn_mi355x_scan_resize(px.ctypes.data, 40, 40, 4, 0, 20, 20, out.ctypes.data) == -1 and "bands must be" in err(L)
    assert L.bnn_mi355x_scan_resize(px.ctypes.data, 40, 40, 3, 0, 0, 20, out.ctypes.data) == -1 and "pixels a side" in err(L)
    assert L.bnn_mi355x_scan_resize(px.ctypes.data, 40, 40, 3, 0, 20, 8193, out.ctypes.data) == -1 and "pixels a side" in err(L)


@pytest.mark.parametrize("network, what", [("cnvW1A2", "built for cnvW1A1 only"), ("cnvW2A2", "built for cnvW1A1 only"),
                                           ("lfcW1A1", "CNV networks only"), ("lfcW1A2", "CNV networks only")])
def test_other_networks_refuse(network, what):
    """the 2-bit nets and the LFC nets: every new entry point says so, host-only ones included"""
    lib = gl.load(network)
    nx, ny = C.c_int(0), C.c_int(0)
    px = np.zeros(3 * 40 * 40, np.uint8)
    one = np.array([32], np.int32)
    boxes = np.zeros((64, 4), np.int32)
    calls = [lambda: lib.bnn_mi355x_scan_grid(40, 40, C.byref(nx), C.byref(ny)),
             lambda: lib.bnn_mi355x_scan_boxes(40, 40, 32, None, 0, None, None),
             lambda: -1 if not lib.bnn_mi355x_scan_planes(px.ctypes.data, 40, 40, 10, C.byref(nx), C.byref(ny), None, 0) else 0,
             lambda: lib.bnn_mi355x_scan_device(px.ctypes.data, 40, 40, 10, None, None, None),
             lambda: -1 if not lib.bnn_mi355x_scan_scene(px.ctypes.data, 40, 40, 3, 0, one.ctypes.data, 1, 10, boxes.ctypes.data, None, None, 0) else 0,
             lambda: lib.bnn_mi355x_debug_scan_stage(px.ctypes.data, 40, 40, 0, boxes.ctypes.data, boxes.nbytes, C.byref(nx), C.byref(ny)),
             lambda: lib.bnn_mi355x_scan_resize(px.ctypes.data, 40, 40, 3, 0, 20, 20, boxes.ctypes.data)]
    for call in calls:
        assert call() == -1
        assert what in lib.bnn_mi355x_last_error().decode()
