#!/usr/bin/env python3
"""Activation-fault sweeps (bnn_mi355x_act_fault_sweep): every site x shift of every non-last layer, one whole layer
per call, on N random images, for cnvW1A1, cnvW2A2 and lfcW1A1.  Per layer: wall and device time, (site, image) pairs
per second of wall time, the share of sites that change some image, and the pairs each layer had to run
(bnn_mi355x_last_act_sweep_stages).
usage: act_fault_sweep_rate.py [n_images]"""
import ctypes as C
import os
import struct
import sys
import tempfile
import time

import numpy as np
import torch  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gpu_lib as gl  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
ip = C.POINTER(C.c_int)
NETS = ["cnvW1A1", "cnvW2A2", "lfcW1A1"]


def sites(L, layer):
    k = L.bnn_mi355x_enumerate_act_faults(layer, 0, None, 0)
    rec = np.zeros((k, 5), np.int32)
    L.bnn_mi355x_enumerate_act_faults(layer, 0, rec.ctypes.data_as(ip), k)
    return rec


def sweep(L, path, recs):
    k = len(recs)
    changed = np.zeros(k, np.int32)
    cnt, usec = C.c_int(0), C.c_float(0)
    t0 = time.perf_counter()
    total = L.bnn_mi355x_act_fault_sweep(path, 10, recs.ctypes.data_as(ip), k, changed.ctypes.data_as(ip), None, 0,
                                         C.byref(cnt), C.byref(usec))
    wall = time.perf_counter() - t0
    assert total >= 0, L.bnn_mi355x_last_error()
    s = L.bnn_mi355x_last_act_sweep_stages(None, 0)
    st = (C.c_long * s)()
    L.bnn_mi355x_last_act_sweep_stages(st, s)
    return wall * 1e3, usec.value * k * cnt.value / 1e3, list(st), changed


rng = np.random.default_rng(0)
print("activation-fault sweeps on %d random images: every site x shift of the layer's output in one call; ms" % n)
for net in NETS:
    cnv = net.startswith("cnv")
    L = gl.load(net)
    L.load_parameters(gl.param_dir("cifar10" if cnv else "mnist", net).encode())
    with tempfile.NamedTemporaryFile(dir="/tmp", suffix=".bin") as f:
        if cnv:
            f.write(np.concatenate([np.ones((n, 1), np.uint8), rng.integers(0, 256, (n, 3072), dtype=np.uint8)], axis=1).tobytes())
        else:
            f.write(struct.pack(">4I", 0x803, n, 28, 28) + rng.integers(0, 256, (n, 784), dtype=np.uint8).tobytes())
        f.flush()
        path = f.name.encode()
        sweep(L, path, sites(L, 0)[:64])  # (warm-up: buffers grown, kernels loaded)
        all_wall = all_dev = all_pairs = 0.0
        for layer in range(8 if cnv else 3):
            recs = sites(L, layer)
            wall, dev, st, changed = sweep(L, path, recs)
            pairs = len(recs) * n
            all_wall, all_dev, all_pairs = all_wall + wall, all_dev + dev, all_pairs + pairs
            print("%s L%d %8d sites x shifts: %9.1f ms wall (device %9.1f)  %6.1f M pairs/s  %5.1f%% change an image" % (
                net, layer, len(recs), wall, dev, pairs / wall / 1e3, 100.0 * (changed > 0).mean()))
            print("    pairs per layer: " + " ".join("%d" % x for x in st))
            sys.stdout.flush()
        print("%s all layers: %.1f ms wall (device %.1f), %.1f M pairs/s" % (net, all_wall, all_dev, all_pairs / all_wall / 1e3))
