"""Exhaustive single-fault sweeps, host side (no GPU): bnn_mi355x_enumerate_faults lists every distinct single fault
of a layer's weight or threshold memory -- the positions plan_faults can draw, bit aligned down to a multiple of the
word size as apply_fault aligns it, ordered by (mem, ind, thresh, bit) -- and bnn_mi355x_fault_sweep refuses bad
arguments before anything touches the device."""
import ctypes as C
import sys

import numpy as np
import pytest

import gpu_lib as gl

sys.path.insert(0, gl.ROOT + "/bnn-pynq_amd")
from bnn import params_io  # noqa: E402

NETS = ["cnvW1A1", "cnvW1A2", "cnvW2A2", "lfcW1A1", "lfcW1A2"]
WORD_SIZES = [1, 2, 3, 8, 13, 64]


def elem_bits(net, layer, target):
    """bits of one memory element: a weight word of SIMD * WPI bits; a threshold of 16 bits (24 in CNV layer 0)"""
    L = params_io.layout(net)[layer]
    if target == 0:
        return L["simd"] * L["wbits"]
    return 24 if (net.startswith("cnv") and layer == 0) else 16


def shape(net, layer, target):
    L = params_io.layout(net)[layer]
    return (L["pe"], L["wmem"], 1) if target == 0 else (L["pe"], L["tmem"], L["nthr"])


def enumerate_all(L, layer, target, ws):
    k = L.bnn_mi355x_enumerate_faults(layer, target, ws, 0, None, 0)
    rec = np.zeros((max(k, 1), 8), np.int32)
    assert L.bnn_mi355x_enumerate_faults(layer, target, ws, 0, rec.ctypes.data_as(C.POINTER(C.c_int)), k) == k
    return rec[:k]


@pytest.mark.parametrize("net", NETS)
def test_counts_match_the_memories(net):
    """per layer and target: elements x ceil(element bits / word size); the word-size-1 counts add up to the
    memory bits of params_io.layout"""
    L = gl.load(net)
    total = 0
    for layer, lay in enumerate(params_io.layout(net)):
        for target in (0, 1):
            pe, inds, thr = shape(net, layer, target)
            eb = elem_bits(net, layer, target)
            for ws in WORD_SIZES:
                want = pe * inds * thr * -(-eb // ws)
                assert L.bnn_mi355x_enumerate_faults(layer, target, ws, 0, None, 0) == want, (layer, target, ws)
            total += pe * inds * thr * eb
    bits = sum(l["pe"] * l["wmem"] * l["simd"] * l["wbits"] + l["pe"] * l["tmem"] * l["nthr"] * 16
               for l in params_io.layout(net))
    if net.startswith("cnv"):
        l0 = params_io.layout(net)[0]
        bits += l0["pe"] * l0["tmem"] * l0["nthr"] * 8  # (layer 0: 24-bit thresholds)
    assert total == bits
    expected = {"cnvW1A1": 1601728, "cnvW1A2": 1632960, "cnvW2A2": 3203456, "lfcW1A1": 3064832, "lfcW1A2": 3113984}
    assert total == expected[net]


@pytest.mark.parametrize("net", NETS)
@pytest.mark.parametrize("ws", [1, 3, 8])
def test_records_unique_in_range_in_order(net, ws):
    L = gl.load(net)
    for layer in range(len(params_io.layout(net))):
        for target in (0, 1):
            rec = enumerate_all(L, layer, target, ws)
            if len(rec) == 0:
                assert target == 1 and params_io.layout(net)[layer]["nthr"] == 0
                continue
            pe, inds, thr = shape(net, layer, target)
            eb = elem_bits(net, layer, target)
            assert (rec[:, 0] == 0).all() and (rec[:, 1] == target).all() and (rec[:, 2] == layer).all()
            assert (rec[:, 7] == ws).all()
            m, i, t, b = rec[:, 3], rec[:, 4], rec[:, 5], rec[:, 6]
            assert (m >= 0).all() and (m < pe).all() and (i >= 0).all() and (i < inds).all()
            assert (t >= 0).all() and (t < thr).all() and (b >= 0).all() and (b < eb).all() and (b % ws == 0).all()
            key = ((m.astype(np.int64) * inds + i) * thr + t) * 64 + b
            assert (np.diff(key) > 0).all(), "strictly increasing in (mem, ind, thresh, bit): unique and ordered"
            # a window [first, first + cap) is that slice of the whole list
            first, cap = len(rec) // 3, 7
            part = np.zeros((cap, 8), np.int32)
            assert L.bnn_mi355x_enumerate_faults(layer, target, ws, first, part.ctypes.data_as(C.POINTER(C.c_int)), cap) == len(rec)
            got = min(cap, len(rec) - first)
            assert (part[:got] == rec[first:first + got]).all()


@pytest.mark.parametrize("net", NETS)
@pytest.mark.parametrize("ws,target", [(1, -1), (4, 0), (8, 1), (64, -1)])
def test_every_planned_fault_is_enumerated(net, ws, target):
    """each record plan_faults draws, its bit aligned down to a multiple of word_size, appears in the enumeration"""
    L = gl.load(net)
    tables = {}
    for seed in (11, 12345):
        rec = (C.c_int * (8 * 400))()
        k = L.bnn_mi355x_plan_faults(seed, 1000, 400, ws, target, None, 0, rec, 400)
        assert k == 400
        plan = np.array(rec[:8 * k], np.int32).reshape(k, 8)
        for r in plan:
            key = (int(r[2]), int(r[1]))
            if key not in tables:
                tables[key] = {tuple(x[3:]) for x in enumerate_all(L, key[0], key[1], ws)}
            aligned = (int(r[3]), int(r[4]), int(r[5]), int(r[6]) // ws * ws, int(r[7]))
            assert aligned in tables[key], r


def test_bad_arguments():
    L = gl.load("cnvW1A1")
    for layer, target, ws, first in ((-1, 0, 1, 0), (9, 0, 1, 0), (0, 2, 1, 0), (0, -1, 1, 0), (0, 0, 0, 0), (0, 0, 65, 0),
                                     (0, 0, 1, -1)):
        assert L.bnn_mi355x_enumerate_faults(layer, target, ws, first, None, 0) == -1
        assert b"enumerate_faults" in L.bnn_mi355x_last_error()
    Lf = gl.load("lfcW1A1")
    assert Lf.bnn_mi355x_enumerate_faults(4, 0, 1, 0, None, 0) == -1
    assert Lf.bnn_mi355x_enumerate_faults(3, 0, 1, 0, None, 0) > 0


def test_sweep_refusals_without_a_gpu():
    """argument checks come first: no records / changed array, cap_diffs without diffs, a negative count"""
    L = gl.load("cnvW1A1")
    rec = (C.c_int * 8)(0, 0, 1, 0, 0, 0, 0, 1)
    ch = (C.c_int * 1)()
    for args in ((None, 1, ch, None, 0), (rec, 1, None, None, 0), (rec, 1, ch, None, 5), (rec, -1, ch, None, 0)):
        assert L.bnn_mi355x_fault_sweep(b"/nonexistent", 10, args[0], args[1], args[2], args[3], args[4], None, None) == -1
        assert b"fault_sweep" in L.bnn_mi355x_last_error()
    assert L.bnn_mi355x_last_sweep_stages(None, 0) == 0


def test_variant_refused(variant_libs):
    """the hardened overlays' fault model is not modelled: the sweep is refused like the campaigns are"""
    L = gl.load("cnvW1A1-TMR")
    rec = (C.c_int * 8)(0, 0, 1, 0, 0, 0, 0, 1)
    ch = (C.c_int * 1)()
    assert L.bnn_mi355x_fault_sweep(b"/nonexistent", 10, rec, 1, ch, None, 0, None, None) == -1
    assert b"not modelled" in L.bnn_mi355x_last_error()
