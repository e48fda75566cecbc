#!/usr/bin/env python3
"""Exhaustive single-fault sweeps (bnn_mi355x_fault_sweep) against the dense route at the same number of image passes.
Per network, on N random images: every weight fault (word size 1) of an early, a middle and an FC layer, and every
threshold fault of the network; wall and device time of the sweep, and per layer the (fault, image) pairs that ran
through it (bnn_mi355x_last_sweep_stages).  The dense baseline is bnn_mi355x_fault_campaigns with flip_count = 1 on the
same layer and target -- every run classifies every image once with one fault -- measured with R runs and scaled to
the sweep's fault count (its cost is linear in the runs: one blob copy and one pass of N images each).
usage: fault_sweep_rate.py [n_images [dense_runs]]"""
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
R = int(sys.argv[2]) if len(sys.argv) > 2 else 4096
ip = C.POINTER(C.c_int)
CASES = {"cnvW1A1": [1, 4, 7], "cnvW2A2": [1, 4, 7], "lfcW1A1": [0, 1, 3]}


def records(L, layers, target):
    out = []
    for layer in layers:
        k = L.bnn_mi355x_enumerate_faults(layer, target, 1, 0, None, 0)
        rec = np.zeros((max(k, 1), 8), np.int32)
        L.bnn_mi355x_enumerate_faults(layer, target, 1, 0, rec.ctypes.data_as(ip), k)
        out.append(rec[:k])
    return np.concatenate(out)


def sweep(L, path, recs):
    k = len(recs)
    changed = np.zeros(k, np.int32)
    cnt, usec = C.c_int(0), C.c_float(0)
    t0 = time.perf_counter()
    total = L.bnn_mi355x_fault_sweep(path, 10, recs.ctypes.data_as(ip), k, changed.ctypes.data_as(ip), None, 0,
                                     C.byref(cnt), C.byref(usec))
    wall = time.perf_counter() - t0
    assert total >= 0, L.bnn_mi355x_last_error()
    s = L.bnn_mi355x_last_sweep_stages(None, 0)
    st = (C.c_long * s)()
    L.bnn_mi355x_last_sweep_stages(st, s)
    return wall * 1e3, usec.value * k * cnt.value / 1e3, list(st), changed


def dense(L, path, runs, target, layers):
    tl = (C.c_int * max(len(layers), 1))(*layers)
    cnt, usec = C.c_int(0), C.c_float(0)
    t0 = time.perf_counter()
    p = L.bnn_mi355x_fault_campaigns(path, 10, runs, 1000, 1, 1, target, tl if layers else None, len(layers), C.byref(cnt),
                                     C.byref(usec))
    wall = time.perf_counter() - t0
    assert p, L.bnn_mi355x_last_error()
    L.free_results(p)
    return wall * 1e3, usec.value * runs * cnt.value / 1e3


rng = np.random.default_rng(0)
print("single-fault sweeps on %d random images, every fault of the layer (word size 1); dense = fault_campaigns with "
      "flip_count 1, %d runs measured and scaled to the fault count; ms" % (n, R))
for net, layers in CASES.items():
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
        dense(L, path, 64, 0, [layers[0]])  # (warm-up: buffers grown, kernels loaded)
        sweep(L, path, records(L, [layers[0]], 0)[:64])
        for what, recs, target, tl in [("L%d weights" % l, records(L, [l], 0), 0, [l]) for l in layers] + [
                ("all thresholds", records(L, range(9 if cnv else 4), 1), 1, [])]:
            sw_wall, sw_dev, st, changed = sweep(L, path, recs)
            runs = min(R, len(recs))
            d_wall, d_dev = dense(L, path, runs, target, tl)
            scale = len(recs) / runs
            print("%s %-14s %8d faults: sweep %9.1f ms (device %9.1f)  dense %9.1f ms (device %9.1f, %d runs x%.1f)  "
                  "x%.2f wall  %.1f%% of faults change an image" % (
                      net, what, len(recs), sw_wall, sw_dev, d_wall * scale, d_dev * scale, runs, scale,
                      d_wall * scale / sw_wall, 100.0 * (changed > 0).mean()))
            print("    pairs per layer: " + " ".join("%d" % x for x in st))
            sys.stdout.flush()
