#!/usr/bin/env python3
"""Hardened memory schemes in the memory upset campaigns (bnn_mi355x_hardened_mem_noise_campaigns): RUNS runs over N random
images of cnvW1A1, every weight and threshold rate 2^-6.  Configurations, alternating in one process: mem_noise_campaigns at
the same rates (the baseline: independent single-bit flips, by the plain route's own kernels), then each supported
scheme (0 none, 1 TMR, 2 interleaved, 3 resilient-interleaved) at burst 1 and 4.  Per configuration: wall and device time
(best of three calls), the ratio to the baseline's device time, the physical bits flipped and the logical bits that differ
after voting and de-interleaving, and the mean accuracy against the fault-free classes.
usage: hardened_mem_noise_rate.py [n_images [runs [network]]]"""
import ctypes as C
import os
import sys
import tempfile
import time

import numpy as np
import torch  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gpu_lib as gl  # noqa: E402

args = sys.argv[1:]
n = int(args[0]) if len(args) > 0 else 1000
runs = int(args[1]) if len(args) > 1 else 100
net = args[2] if len(args) > 2 else "cnvW1A1"
SEED, RATE = 12345, 1 << 26
NAMES = ("none", "TMR", "interleaved", "resilient-interleaved")


def call(L, path, rw, rt, scheme=None, burst=1):
    """-> (wall ms, device ms, physical bits, logical bits, classes)"""
    up = C.c_uint * len(rw)
    cnt, usec = C.c_int(0), C.c_float(0)
    t0 = time.perf_counter()
    if scheme is None:
        p = L.bnn_mi355x_mem_noise_campaigns(path, 10, runs, SEED, up(*rw), up(*rt), len(rw), C.byref(cnt), C.byref(usec))
    else:
        p = L.bnn_mi355x_hardened_mem_noise_campaigns(path, 10, scheme, burst, runs, SEED, up(*rw), up(*rt), len(rw), C.byref(cnt), C.byref(usec))
    wall = time.perf_counter() - t0
    assert p, L.bnn_mi355x_last_error()
    classes = np.ctypeslib.as_array(p, shape=(runs * cnt.value,)).copy().reshape(runs, cnt.value)
    L.free_results(p)
    k = runs * len(rw) * (2 if scheme is None else 4)
    c = (C.c_long * k)()
    (L.bnn_mi355x_last_mem_noise_counts if scheme is None else L.bnn_mi355x_last_hardened_mem_noise_counts)(c, k)
    c = np.array(c[:], np.int64)
    phys, logical = (int(c.sum()), int(c.sum())) if scheme is None else (int(c[0::2].sum()), int(c[1::2].sum()))
    return wall * 1e3, usec.value * runs * cnt.value / 1e3, phys, logical, classes


L = gl.load(net)
L.load_parameters(gl.param_dir("cifar10", net).encode())
nl = 9
rw, rt = [RATE] * nl, [RATE] * 8 + [0]
schemes = [s for s in range(4) if L.bnn_mi355x_hardening_layout(s, 0, (C.c_int * 3)()) == 0]
configs = [("mem_noise_campaigns", None, 1)] + [("%s burst %d" % (NAMES[s], b), s, b) for s in schemes for b in (1, 4)]
rng = np.random.default_rng(0)
print("%s: %d runs x %d random images, every weight and threshold rate 2^-6; ms, best of 3, configurations alternating" % (net, runs, n))
with tempfile.NamedTemporaryFile(suffix=".bin") as f:
    f.write(np.concatenate([np.ones((n, 1), np.uint8), rng.integers(0, 256, (n, 3072), dtype=np.uint8)], axis=1).tobytes())
    f.flush()
    path = f.name.encode()
    clean = call(L, path, [0] * nl, [0] * nl)[4][0]
    call(L, path, rw, rt, 1, 4)  # (warm-up: buffers grown, kernels loaded)
    best = {}
    for _ in range(3):
        for name, s, b in configs:
            got = call(L, path, rw, rt, s, b)
            if name not in best or got[1] < best[name][1]:
                best[name] = got
    for name, s, b in configs:
        g = best[name]
        print("%-32s %8.2f ms wall, device %8.2f (x%.2f of mem_noise_campaigns)  physical bits %9d  logical %9d  mean accuracy %6.2f %%" % (
            name, g[0], g[1], g[1] / best["mem_noise_campaigns"][1], g[2], g[3], 100.0 * (g[4] == clean[None]).mean()))
