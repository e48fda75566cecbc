#!/usr/bin/env python3
"""What a propagation profile costs (bnn_mi355x_sweep_profile): one whole-layer single-fault sweep per case -- cnvW1A1
weight faults of layer 4, cnvW1A1 activation sites of layer 0, lfcW1A1 weight faults of layer 1 -- on N random images,
profiling off and on alternating in ONE process for `reps` rounds.  Every call's wall and device time, the ratio of the
medians (on / off) and the spread between repeats of the same setting; the results of both settings must agree.
usage: sweep_profile_rate.py [n_images] [reps]"""
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
reps = max(3, int(sys.argv[2])) if len(sys.argv) > 2 else 3
ip, lp = C.POINTER(C.c_int), C.POINTER(C.c_long)
CASES = [("cnvW1A1", "parameter", 4), ("cnvW1A1", "activation", 0), ("lfcW1A1", "parameter", 1)]


def records(L, kind, layer):
    if kind == "parameter":
        k = L.bnn_mi355x_enumerate_faults(layer, 0, 1, 0, None, 0)
        rec = np.zeros((k, 8), np.int32)
        L.bnn_mi355x_enumerate_faults(layer, 0, 1, 0, rec.ctypes.data_as(ip), k)
    else:
        k = L.bnn_mi355x_enumerate_act_faults(layer, 0, None, 0)
        rec = np.zeros((k, 5), np.int32)
        L.bnn_mi355x_enumerate_act_faults(layer, 0, rec.ctypes.data_as(ip), k)
    return rec


def sweep(L, kind, path, recs):
    """-> (wall ms, device ms, changed)"""
    k = len(recs)
    changed = np.zeros(k, np.int32)
    cnt, usec = C.c_int(0), C.c_float(0)
    fn = L.bnn_mi355x_fault_sweep if kind == "parameter" else L.bnn_mi355x_act_fault_sweep
    t0 = time.perf_counter()
    total = fn(path, 10, recs.ctypes.data_as(ip), k, changed.ctypes.data_as(ip), None, 0, C.byref(cnt), C.byref(usec))
    wall = time.perf_counter() - t0
    assert total >= 0, L.bnn_mi355x_last_error()
    return wall * 1e3, usec.value * k * cnt.value / 1e3, changed


def image_file(f, cnv):
    if cnv:
        f.write(np.concatenate([np.ones((n, 1), np.uint8), rng.integers(0, 256, (n, 3072), dtype=np.uint8)], axis=1).tobytes())
    else:
        f.write(struct.pack(">4I", 0x803, n, 28, 28) + rng.integers(0, 256, (n, 784), dtype=np.uint8).tobytes())
    f.flush()
    return f.name.encode()


rng = np.random.default_rng(0)
print("propagation profile off vs on, %d random images, every fault of the layer per call, %d alternations; ms" % (n, reps))
for net, kind, layer in CASES:
    cnv = net.startswith("cnv")
    L = gl.load(net)
    L.load_parameters(gl.param_dir("cifar10" if cnv else "mnist", net).encode())
    with tempfile.NamedTemporaryFile(dir="/tmp", suffix=".bin") as f:
        path = image_file(f, cnv)
        recs = records(L, kind, layer)
        for on in (0, 1):  # (warm-up of both settings: buffers grown, kernels loaded)
            L.bnn_mi355x_sweep_profile(on)
            sweep(L, kind, path, recs[:64])
        wall, dev, ref = {0: [], 1: []}, {0: [], 1: []}, None
        for _ in range(reps):
            for on in (0, 1):
                L.bnn_mi355x_sweep_profile(on)
                w, d, changed = sweep(L, kind, path, recs)
                wall[on].append(w)
                dev[on].append(d)
                if ref is None:
                    ref = changed.copy()
                assert (changed == ref).all(), "the two settings disagree"
        L.bnn_mi355x_sweep_profile(0)
        cols = C.c_int(0)
        rows = L.bnn_mi355x_last_sweep_profile(0, None, None, 0, C.byref(cols))
        alive = np.zeros((rows, cols.value), np.int64)
        flipped = np.zeros((rows, cols.value), np.int64)
        L.bnn_mi355x_last_sweep_profile(0, alive.ctypes.data_as(lp), flipped.ctypes.data_as(lp), rows, None)
        m = {on: (float(np.median(wall[on])), float(np.median(dev[on]))) for on in (0, 1)}
        spread = {on: (max(wall[on]) - min(wall[on]), max(dev[on]) - min(dev[on])) for on in (0, 1)}
        print("%s %s layer %d, %d faults:" % (net, kind, layer, len(recs)))
        for on in (0, 1):
            print("    profile %s: wall %s | device %s" % ("on " if on else "off", " ".join("%.1f" % x for x in wall[on]),
                                                          " ".join("%.1f" % x for x in dev[on])))
        print("    medians on / off: wall %.1f / %.1f = x%.3f, device %.1f / %.1f = x%.3f; spread between repeats: wall %.1f (off) %.1f (on), "
              "device %.1f (off) %.1f (on)" % (m[1][0], m[0][0], m[1][0] / m[0][0], m[1][1], m[0][1], m[1][1] / m[0][1], spread[0][0],
                                                spread[1][0], spread[0][1], spread[1][1]))
        print("    share of pairs alive per layer: " + " ".join("%.4f" % x for x in alive.sum(axis=0) / float(max(rows, 1) * n)))
        sys.stdout.flush()
