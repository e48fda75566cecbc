"""CPU: bnn_mi355x_order_lines -- the line model of read_page on boxes the caller has (csrc/page.cpp: order_lines) --
against hand-worked cases whose expected order is written out here, against tests/lines_ref.py (the model restated in
plain Python) on random box sets, and what it refuses.  Host only: any library, no GPU."""
import ctypes as C

import numpy as np
import pytest

import gpu_lib as gl
import lines_ref


@pytest.fixture(scope="module")
def lib():
    return gl.load("cnvW1A1")  # any library: the model touches no GPU and no network


def order_lines(lib, boxes, first, word_gap=0, want_line=True, want_gap=True):
    n = len(first)
    b = np.ascontiguousarray(np.asarray(boxes, np.int32).reshape(-1, 4))
    f = np.ascontiguousarray(np.asarray(first, np.int32))
    m = max(n, 1)
    b = b if n else np.zeros((1, 4), np.int32)
    f = f if n else np.zeros(1, np.int32)
    order, line, gap = np.full(m + 1, -7, np.int32), np.full(m + 1, -7, np.int32), np.full(m + 1, -7, np.int32)
    rc = lib.bnn_mi355x_order_lines(b.ctypes.data, f.ctypes.data, n, word_gap, order.ctypes.data, line.ctypes.data if want_line else None,
                                    gap.ctypes.data if want_gap else None)
    assert rc == 0, lib.bnn_mi355x_last_error().decode()
    assert (order[n:] == -7).all() and (line[n:] == -7).all() and (gap[n:] == -7).all()  # nothing is written past n
    return order[:n].tolist(), line[:n].tolist(), gap[:n].tolist()


def check(lib, boxes, first, word_gap, order, line, gap):
    got = order_lines(lib, boxes, first, word_gap)
    assert got == (order, line, gap)
    assert lines_ref.order_lines(boxes, first, word_gap) == (order, line, gap)  # the oracle agrees with the hand-worked answer


def test_two_rows_of_unequal_heights(lib):
    # row 0: A (0..20 high) and B (5..15); row 1: D (28..50) and C (30..40).  Given as D, B, C, A.
    boxes = [(12, 28, 30, 50), (15, 5, 25, 15), (0, 30, 8, 40), (0, 0, 10, 20)]
    first = [28 * 100 + 12, 5 * 100 + 15, 30 * 100 + 0, 0]
    check(lib, boxes, first, 0, [3, 1, 2, 0], [0, 0, 1, 1], [0, 0, 0, 0])


def test_a_box_over_two_rows_joins_the_larger_overlap_and_on_a_tie_the_earlier(lib):
    # a opens line 0 = [0, 30); b (20..50) overlaps it by 10 of 30: line 1 = [20, 50).  T (22..36, h 14) overlaps line 0
    # by 8 and line 1 by 14, both at least half of 14: line 1.  U (24..30, h 6) overlaps both by 6: the earlier, line 0.
    boxes = [(0, 0, 10, 30), (0, 20, 10, 50), (20, 22, 30, 36), (40, 24, 50, 30)]
    first = [0, 2000, 2220, 2440]
    check(lib, boxes, first, 0, [0, 3, 1, 2], [0, 0, 1, 1], [0, 0, 0, 0])


def test_half_inside_a_band_joins_one_pixel_less_does_not(lib):
    a = (0, 0, 10, 20)
    check(lib, [a, (20, 10, 30, 30)], [0, 1020], 0, [0, 1], [0, 0], [0, 0])   # ov 10, h 20: 2 ov == min(20, 20)
    check(lib, [a, (20, 11, 30, 31)], [0, 1120], 0, [0, 1], [0, 1], [0, 0])   # ov 9: a line of its own
    # the band is the smaller of the two: a 4-high box half inside the lower end of a 20-high band
    check(lib, [a, (20, 18, 30, 22)], [0, 1820], 0, [0, 1], [0, 0], [0, 0])   # ov 2, h 4
    check(lib, [a, (20, 19, 30, 23)], [0, 1920], 0, [0, 1], [0, 1], [0, 0])   # ov 1
    # a band grows with what joins it: c joins [0, 30) after b made it so, and would not have joined [0, 20)
    check(lib, [a, (20, 10, 30, 30), (40, 21, 50, 39)], [0, 1020, 2140], 0, [0, 1, 2], [0, 0, 0], [0, 0, 0])
    check(lib, [a, (40, 21, 50, 39)], [0, 2140], 0, [0, 1], [0, 1], [0, 0])


def test_identical_boxes_go_by_first_pixel(lib):
    check(lib, [(5, 5, 10, 10)] * 3, [30, 10, 20], 3, [1, 2, 0], [0, 0, 0], [0, 0, 0])


def test_one_box_and_none(lib):
    check(lib, [(3, 4, 5, 6)], [7], 1, [0], [0], [0])
    check(lib, [], [], 0, [], [], [])
    check(lib, [], [], 5, [], [], [])


def test_word_gap_at_the_distance_one_below_and_off(lib):
    boxes, first = [(0, 0, 10, 10), (15, 0, 20, 10)], [0, 15]
    check(lib, boxes, first, 5, [0, 1], [0, 0], [0, 1])   # 15 - 10 == 5
    check(lib, boxes, first, 6, [0, 1], [0, 0], [0, 0])
    check(lib, boxes, first, 0, [0, 1], [0, 0], [0, 0])
    # the distance is taken from the furthest right edge so far, not from the previous glyph's
    boxes, first = [(0, 0, 30, 10), (5, 2, 8, 9), (33, 0, 40, 10)], [0, 205, 33]
    check(lib, boxes, first, 3, [0, 1, 2], [0, 0, 0], [0, 0, 1])
    check(lib, boxes, first, 4, [0, 1, 2], [0, 0, 0], [0, 0, 0])
    # the first glyph of a line never has a gap, however far to the right it starts
    check(lib, [(50, 0, 60, 10), (80, 30, 90, 40)], [50, 3080], 1, [0, 1], [0, 1], [0, 0])


def test_line_and_gap_may_be_null(lib):
    boxes, first = [(15, 0, 20, 10), (0, 0, 10, 10)], [15, 0]
    assert order_lines(lib, boxes, first, 5, want_line=False, want_gap=False) == ([1, 0], [-7, -7], [-7, -7])
    assert order_lines(lib, boxes, first, 5, want_line=False) == ([1, 0], [-7, -7], [0, 1])
    assert order_lines(lib, boxes, first, 5, want_gap=False) == ([1, 0], [0, 0], [-7, -7])


def random_boxes(rng):
    n = int(rng.integers(0, 41))
    rows = int(rng.integers(1, 5))
    boxes, first = [], []
    for _ in range(n):
        row = int(rng.integers(0, rows))
        u = row * 40 + int(rng.integers(0, 25))
        h = int(rng.integers(1, 60 if rng.random() < 0.1 else 30))
        l = int(rng.integers(0, 300))
        w = int(rng.integers(1, 40))
        boxes.append((l, u, l + w, u + h))
        first.append(u * 400 + l + int(rng.integers(0, w)))
    return boxes, first


def test_random_box_sets_equal_the_oracle(lib):
    rng = np.random.default_rng(20)
    lines_seen = set()
    for k in range(400):
        boxes, first = random_boxes(rng)
        if k % 7 == 0 and boxes:  # duplicates: ties down to the input index
            boxes += boxes[:3]
            first += first[:3]
        word_gap = int(rng.integers(0, 30))
        want = lines_ref.order_lines(boxes, first, word_gap)
        assert order_lines(lib, boxes, first, word_gap) == want, (k, boxes, first, word_gap)
        order, line, gap = want
        assert sorted(order) == list(range(len(boxes))) and line == sorted(line)
        lines_seen.add(len(set(line)))
    assert len(lines_seen) > 3  # the sets are not all one line


def refused(lib, boxes, first, n, word_gap, order=True):
    out = np.full(max(n, 1), -7, np.int32)
    rc = lib.bnn_mi355x_order_lines(None if boxes is None else boxes.ctypes.data, None if first is None else first.ctypes.data, n, word_gap,
                                    out.ctypes.data if order else None, None, None)
    assert rc == -1 and (out == -7).all()
    return lib.bnn_mi355x_last_error().decode()


def test_refusals(lib):
    b, f = np.array([[0, 0, 4, 4], [5, 0, 9, 4]], np.int32), np.array([0, 5], np.int32)
    for kw in (dict(boxes=None, first=f), dict(boxes=b, first=None), dict(boxes=b, first=f, order=False)):
        err = refused(lib, n=2, word_gap=0, **kw)
        assert err == "order_lines: bad arguments (null pointer)"
    assert refused(lib, b, f, -1, 0) == "order_lines: negative number of boxes"
    assert refused(lib, b, f, 2, -1) == "order_lines: word_gap must be 0 (none) or more"
    bad = np.array([[0, 0, 4, 4], [5, 3, 9, 3]], np.int32)
    assert refused(lib, bad, f, 2, 0) == "order_lines: box 1 (5, 3, 9, 3) is empty or inverted (need right > left and lower > upper)"


def test_the_limit(lib):
    n = 65536
    boxes = np.zeros((n + 1, 4), np.int32)
    boxes[:, 0] = np.arange(n + 1)[::-1]
    boxes[:, 2] = boxes[:, 0] + 1
    boxes[:, 3] = 5
    first = np.ascontiguousarray(boxes[:, 0])
    err = refused(lib, boxes, first, n + 1, 0)
    assert err == "order_lines: more than 65536 components to put into lines (65537): raise min_pixels"
    order, line = np.zeros(n, np.int32), np.zeros(n, np.int32)
    assert lib.bnn_mi355x_order_lines(boxes.ctypes.data, first.ctypes.data, n, 0, order.ctypes.data, line.ctypes.data, None) == 0
    assert np.array_equal(order, np.arange(n)[::-1]) and not line.any()  # one line, left to right
