#!/usr/bin/env python3
"""Memory upset-rate campaigns (bnn_mi355x_mem_noise_campaigns): RUNS runs over N random images for cnvW1A1, cnvW2A2 and
lfcW1A1.  Configurations, alternating in one process: all rates 0 (the yardstick: the same pairs through the same MULTI
stage kernels, no copy made, nothing drawn), every weight rate 2^-12 / 2^-6, the same with the threshold rates, and layer
0 alone (the CNV nets: the part the host draws and patches).  Per configuration: wall and device time (best of three
calls), pairs per second, the ratio to rate 0, the flips counted against sites x rate.  Then, on the host, the route the
tests use as oracle for the same runs: bnn_mi355x_mem_noise_mask of every layer and target + bnn_mi355x_pack_params_faulty
per run (no classification at all) -- what drawing on the host would cost before a single image is classified.
usage: mem_noise_rate.py [n_images [runs [network ...]]]     (one call per configuration only, no host route:
mem_noise_rate.py N RUNS NET once -- under a profiler)"""
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
once = bool(args) and args[-1] == "once"
if once:
    args = args[:-1]
n = int(args[0]) if len(args) > 0 else 1000
runs = int(args[1]) if len(args) > 1 else 100
NETS = args[2:] or ["cnvW1A1", "cnvW2A2", "lfcW1A1"]
SEED = 12345
ip = C.POINTER(C.c_int)


def campaign(L, path, rw, rt):
    up = C.c_uint * len(rw)
    cnt, usec = C.c_int(0), C.c_float(0)
    t0 = time.perf_counter()
    p = L.bnn_mi355x_mem_noise_campaigns(path, 10, runs, SEED, up(*rw), up(*rt), len(rw), C.byref(cnt), C.byref(usec))
    wall = time.perf_counter() - t0
    assert p, L.bnn_mi355x_last_error()
    L.free_results(p)
    k = runs * len(rw) * 2
    c = (C.c_long * k)()
    L.bnn_mi355x_last_mem_noise_counts(c, k)
    return wall * 1e3, usec.value * runs * cnt.value / 1e3, int(np.sum(c[:]))


def host_route(L, pdir, rw, rt):
    """-> seconds for mask + pack_params_faulty of every run"""
    size = L.bnn_mi355x_pack_params(pdir.encode(), None, 0)
    blob = np.zeros(size, np.uint8)
    t0 = time.perf_counter()
    for r in range(runs):
        recs = []
        for l in range(len(rw)):
            for t, rate in ((0, rw[l]), (1, rt[l])):
                k = L.bnn_mi355x_mem_noise_mask(SEED + r, l, t, rate, 0, None, 0)
                rec = np.zeros((max(k, 1), 8), np.int32)
                L.bnn_mi355x_mem_noise_mask(SEED + r, l, t, rate, 0, rec.ctypes.data_as(ip), k)
                recs.append(rec[:k])
        recs = np.ascontiguousarray(np.concatenate(recs))
        assert L.bnn_mi355x_pack_params_faulty(pdir.encode(), recs.ctypes.data_as(ip), len(recs), blob.ctypes.data, size) == size
    return time.perf_counter() - t0


rng = np.random.default_rng(0)
print("memory upset-rate campaigns: %d runs x %d random images; ms, best of %d, configurations alternating" % (runs, n, 1 if once else 3))
for net in NETS:
    cnv = net.startswith("cnv")
    L = gl.load(net)
    pdir = gl.param_dir("cifar10" if cnv else "mnist", net)
    L.load_parameters(pdir.encode())
    nl = 9 if cnv else 4
    sw = [L.bnn_mi355x_enumerate_faults(l, 0, 1, 0, None, 0) for l in range(nl)]
    st = [L.bnn_mi355x_enumerate_faults(l, 1, 1, 0, None, 0) for l in range(nl)]
    z = [0] * nl
    thr = lambda q: [q if st[l] else 0 for l in range(nl)]
    configs = [("0", z, z), ("w 2^-12", [1 << 20] * nl, z), ("w 2^-6", [1 << 26] * nl, z), ("w+t 2^-12", [1 << 20] * nl, thr(1 << 20)),
               ("w+t 2^-6", [1 << 26] * nl, thr(1 << 26))]
    if cnv:
        configs.append(("L0 w+t 2^-6", [1 << 26] + [0] * 8, [1 << 26] + [0] * 8))
    with tempfile.NamedTemporaryFile(suffix=".bin") as f:
        if cnv:
            f.write(np.concatenate([np.ones((n, 1), np.uint8), rng.integers(0, 256, (n, 3072), dtype=np.uint8)], axis=1).tobytes())
        else:
            f.write(struct.pack(">4I", 0x803, n, 28, 28) + rng.integers(0, 256, (n, 784), dtype=np.uint8).tobytes())
        f.flush()
        path = f.name.encode()
        if not once:
            campaign(L, path, configs[3][1], configs[3][2])  # (warm-up: buffers grown, kernels loaded)
        best = {}
        for _ in range(1 if once else 3):
            for name, rw, rt in configs:
                got = campaign(L, path, rw, rt)
                best[name] = min(best.get(name, got), got)
        for name, rw, rt in configs:
            b = best[name]
            expected = sum((sw[l] * rw[l] + st[l] * rt[l]) for l in range(nl)) * runs / 2.0 ** 32
            print("%s %-12s %8.2f ms wall, device %8.2f, host %6.2f  %7.1f M pairs/s  x%.2f of rate 0 (device)  flips %d (expected %.0f)" % (
                net, name, b[0], b[1], b[0] - b[1], runs * n / b[0] / 1e3, b[1] / best["0"][1], b[2], expected))
        if not once:
            for name, rw, rt in (configs[3], configs[4]):
                s = host_route(L, pdir, rw, rt)
                print("%s %-12s host route (mask + pack_params_faulty, %d runs, nothing classified) %9.1f ms = x%.1f of the whole campaign's wall time" % (
                    net, name, runs, s * 1e3, s * 1e3 / best[name][0]))
        sys.stdout.flush()
