"""Activation-fault sweeps, host side (no GPU): bnn_mi355x_enumerate_act_faults lists every site x shift of a layer's
output map -- as many as the CPU restatement's layer_ref has elements, times levels - 1 -- ordered by (y, x, channel,
shift), and bnn_mi355x_act_fault_sweep refuses bad arguments and bad records before anything touches the device."""
import ctypes as C

import numpy as np
import pytest

import gpu_lib as gl
import oracle_lib as ol

NETS = [("cnvW1A1", "cifar10"), ("cnvW1A2", "cifar10"), ("cnvW2A2", "cifar10"), ("lfcW1A1", "mnist"), ("lfcW1A2", "mnist")]
ip = C.POINTER(C.c_int)
# (h, w, c) of every non-last layer's output as the next layer reads it (CNV layers 1 and 3 after the max-pool)
CNV_MAPS = [(30, 30, 64), (14, 14, 64), (12, 12, 128), (5, 5, 128), (3, 3, 256), (1, 1, 256), (1, 1, 512), (1, 1, 512)]
LFC_MAPS = [(1, 1, 1024)] * 3


def enumerate_all(L, layer):
    k = L.bnn_mi355x_enumerate_act_faults(layer, 0, None, 0)
    rec = np.zeros((max(k, 1), 5), np.int32)
    assert L.bnn_mi355x_enumerate_act_faults(layer, 0, rec.ctypes.data_as(ip), k) == k
    return rec[:k]


def maps(network):
    return CNV_MAPS if network.startswith("cnv") else LFC_MAPS


@pytest.mark.parametrize("network,dataset", NETS, ids=lambda x: x)
def test_totals_equal_layer_ref_elements(network, dataset):
    L = gl.load(network)
    o = ol.Oracle(network, ol.param_dir(dataset, network))
    img = np.random.default_rng(3).integers(0, 256, o.isz, dtype=np.uint8)
    levels = 3 if network.endswith("A2") else 2
    for layer, (h, w, c) in enumerate(maps(network)):
        elems = o.layer_ref(img, layer).size
        assert elems == h * w * c
        assert L.bnn_mi355x_enumerate_act_faults(layer, 0, None, 0) == elems * (levels - 1), layer
    o.close()


@pytest.mark.parametrize("network,dataset", NETS, ids=lambda x: x)
def test_order_and_fields(network, dataset):
    L = gl.load(network)
    levels = 3 if network.endswith("A2") else 2
    for layer, (h, w, c) in enumerate(maps(network)):
        rec = enumerate_all(L, layer)
        y, x, ch, s = np.meshgrid(np.arange(h), np.arange(w), np.arange(c), np.arange(1, levels), indexing="ij")
        want = np.stack([np.full(y.size, layer), y.ravel(), x.ravel(), ch.ravel(), s.ravel()], axis=1)
        assert (rec == want).all(), layer


def test_windows_and_null_records():
    L = gl.load("cnvW2A2")
    full = enumerate_all(L, 3)
    k = len(full)
    assert k == 5 * 5 * 128 * 2
    for first, cap in ((0, 1), (7, 100), (k - 3, 10), (k - 1, 1), (k, 5), (k + 9, 5), (123, 0)):
        buf = np.full((max(cap, 1) + 1, 5), -7, np.int32)
        assert L.bnn_mi355x_enumerate_act_faults(3, first, buf.ctypes.data_as(ip), cap) == k
        got = max(0, min(cap, k - first))
        assert (buf[:got] == full[first:first + got]).all()
        assert (buf[got:] == -7).all(), (first, cap)  # nothing written past the window
    assert L.bnn_mi355x_enumerate_act_faults(3, 5, None, 10) == k


@pytest.mark.parametrize("network,last", [("cnvW1A1", 8), ("cnvW1A2", 8), ("cnvW2A2", 8), ("lfcW1A1", 3), ("lfcW1A2", 3)])
def test_last_and_out_of_range_layers_refused(network, last):
    L = gl.load(network)
    for layer in (last, last + 1, -1, 100):
        assert L.bnn_mi355x_enumerate_act_faults(layer, 0, None, 0) == -1
        assert b"enumerate_act_faults" in L.bnn_mi355x_last_error()
    assert L.bnn_mi355x_enumerate_act_faults(0, -1, None, 0) == -1
    assert L.bnn_mi355x_enumerate_act_faults(last - 1, 0, None, 0) > 0


def test_sweep_argument_refusals_without_a_gpu():
    L = gl.load("cnvW1A1")
    rec = (C.c_int * 5)(7, 0, 0, 3, 1)
    ch = (C.c_int * 1)()
    for args in ((None, 1, ch, None, 0), (rec, 1, None, None, 0), (rec, 1, ch, None, 5), (rec, -1, ch, None, 0)):
        assert L.bnn_mi355x_act_fault_sweep(b"/nonexistent", 10, args[0], args[1], args[2], args[3], args[4], None, None) == -1
        assert b"act_fault_sweep" in L.bnn_mi355x_last_error()
    assert L.bnn_mi355x_last_act_sweep_stages(None, 0) == 0


@pytest.mark.parametrize("network,bad", [
    ("cnvW1A1", (8, 0, 0, 0, 1)),      # the last layer: scores, not activations
    ("cnvW1A1", (9, 0, 0, 0, 1)),      # out of range
    ("cnvW1A1", (-1, 0, 0, 0, 1)),
    ("cnvW1A1", (0, 30, 0, 0, 1)),     # y outside the 30 x 30 map
    ("cnvW1A1", (1, 0, 14, 0, 1)),     # x outside the pooled 14 x 14 map
    ("cnvW1A1", (2, 0, 0, 128, 1)),    # channel
    ("cnvW1A1", (5, 0, 0, 0, 2)),      # shift 2 of a 1-bit activation
    ("cnvW2A2", (4, 0, 0, 0, 3)),      # shift 3 of a 2-bit activation
    ("cnvW2A2", (4, 0, 0, 0, 0)),      # shift 0 changes nothing
    ("lfcW1A1", (3, 0, 0, 0, 1)),      # the last layer: words
    ("lfcW1A2", (0, 1, 0, 0, 1)),      # FC layers: y = x = 0
    ("lfcW1A2", (2, 0, 0, 1024, 2)),
])
def test_bad_records_refused_up_front(network, bad):
    """validated on the host before anything runs on the device: no GPU is needed to refuse them, and the message
    names the record"""
    L = gl.load(network)
    good = (0, 0, 0, 0, 1)
    recs = np.array([good, good, bad], np.int32)
    ch = np.zeros(3, np.int32)
    assert L.bnn_mi355x_act_fault_sweep(b"/nonexistent", 10, recs.ctypes.data_as(ip), 3, ch.ctypes.data_as(ip), None, 0,
                                        None, None) == -1
    err = L.bnn_mi355x_last_error().decode()
    assert "record 2 {%s}" % ", ".join(str(v) for v in bad) in err, err
    assert L.bnn_mi355x_last_act_sweep_stages(None, 0) == 0


def test_variant_refused(variant_libs):
    """the hardened overlays: "not modelled", the one rule of every fault entry point"""
    L = gl.load("cnvW1A1-TMR")
    rec = (C.c_int * 5)(0, 0, 0, 0, 1)
    ch = (C.c_int * 1)()
    assert L.bnn_mi355x_act_fault_sweep(b"/nonexistent", 10, rec, 1, ch, None, 0, None, None) == -1
    assert b"not modelled" in L.bnn_mi355x_last_error()
