#!/usr/bin/env python3
"""Datapath upset-rate campaigns (bnn_mi355x_act_noise_campaigns): RUNS runs over N random images for cnvW1A1, cnvW2A2
and lfcW1A1, every layer at rate 0 (the yardstick: the same pairs through the same stage kernels, no upset launches),
2^-10 and 2^-4.  Per rate: wall and device time (best of three calls), pairs per second, the ratio to rate 0, the upsets
counted on the device against their expectation.
usage: act_noise_rate.py [n_images [runs [network ...]]]     (one call per rate only: act_noise_rate.py N RUNS NET once)"""
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

args = sys.argv[1:]
once = bool(args) and args[-1] == "once"  # (under a profiler: no warm-up, no repeats)
if once:
    args = args[:-1]
n = int(args[0]) if len(args) > 0 else 1000
runs = int(args[1]) if len(args) > 1 else 100
NETS = args[2:] or ["cnvW1A1", "cnvW2A2", "lfcW1A1"]
RATES = [(0, "0"), (1 << 22, "2^-10"), (1 << 28, "2^-4")]


def campaign(L, path, nl, rate):
    rq = (C.c_uint * nl)(*([rate] * nl))
    cnt, usec = C.c_int(0), C.c_float(0)
    t0 = time.perf_counter()
    p = L.bnn_mi355x_act_noise_campaigns(path, 10, runs, 12345, rq, nl, C.byref(cnt), C.byref(usec))
    wall = time.perf_counter() - t0
    assert p, L.bnn_mi355x_last_error()
    L.free_results(p)
    c = (C.c_long * (runs * nl))()
    L.bnn_mi355x_last_act_noise_counts(c, runs * nl)
    return wall * 1e3, usec.value * runs * cnt.value / 1e3, int(np.sum(c[:]))


rng = np.random.default_rng(0)
print("upset-rate campaigns: %d runs x %d random images, every layer at the same rate; ms, best of %d" % (runs, n, 1 if once else 3))
for net in NETS:
    cnv = net.startswith("cnv")
    L = gl.load(net)
    L.load_parameters(gl.param_dir("cifar10" if cnv else "mnist", net).encode())
    nl = 8 if cnv else 3
    sites = sum(L.bnn_mi355x_enumerate_act_faults(l, 0, None, 0) for l in range(nl)) // (2 if net.endswith("A2") else 1)
    with tempfile.NamedTemporaryFile(suffix=".bin") as f:
        if cnv:
            f.write(np.concatenate([np.ones((n, 1), np.uint8), rng.integers(0, 256, (n, 3072), dtype=np.uint8)], axis=1).tobytes())
        else:
            f.write(struct.pack(">4I", 0x803, n, 28, 28) + rng.integers(0, 256, (n, 784), dtype=np.uint8).tobytes())
        f.flush()
        path = f.name.encode()
        if not once:
            campaign(L, path, nl, 1 << 22)  # (warm-up: buffers grown, kernels loaded)
        base = None
        for rate, name in RATES:
            best = min(campaign(L, path, nl, rate) for _ in range(1 if once else 3))
            base = base or best
            print("%s rate %-6s %9.1f ms wall, device %9.1f  %7.1f M pairs/s  x%.2f of rate 0 (device)  upsets %d (expected %.0f)" % (
                net, name, best[0], best[1], runs * n / best[0] / 1e3, best[1] / base[1], best[2],
                float(sites) * runs * n * rate / 2.0 ** 32))
            sys.stdout.flush()
