#!/usr/bin/env python3
"""Coded weight memories in the exposure campaigns (bnn_mi355x_wecc_exposure_campaigns, weight_code 1): RUNS runs over N
random images of cnvW1A1, every weight and threshold rate 2^-10 PER EPOCH, 100 epochs of N/100 images.
Timing, per organisation (TMR; scheme 0 + SEC-DED thresholds; burst 1) and schedule (rewrite every epoch; repair every
epoch; repair every epoch + rewrite every 10; never): the yardstick is bnn_mi355x_repair_exposure_campaigns with the
same arguments, and against it, on the same images, seeds and rates, wecc_exposure_campaigns with weight_code 1.  The
two calls alternate in one process, three rounds, best of three by device time.  Per configuration: wall and device
time, the ratio to the yardstick, next to the yardstick's own run-to-run spread (worst / best of its three device times).
What the code buys: the same configurations at bursts 1 and 2, with and without weight_code 1: the agreement with the
fault-free classes over the first epoch, the last epoch and all images, the logical bits that differ after the last epoch
(weights, thresholds), and for the coded weights the code words at status 1 and 2 after the last epoch, those the repairs
rewrote over all epochs and those still unlike the loaded ones after the last repair.
usage: wecc_rate.py [n_images [runs [network]]]"""
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
SEED, RATE = 12345, 1 << 22
ORGS = (("TMR", 1, 0), ("none + SEC-DED", 0, 1))
# (name, scrub_every, repair_every)
CONFIGS = (("rewrite every epoch", 1, 0), ("repair every epoch", 0, 1), ("repair every epoch + rewrite every 10", 10, 1), ("never", 0, 0))


def call(L, path, rw, rt, scheme, code, weight_code, burst, epoch_images, scrub_every, repair_every):
    """weight_code None: repair_exposure_campaigns (counts widened to twelve), the yardstick.
    -> (wall ms, device ms, counts [run, epoch, layer, 12], classes)"""
    up = C.c_uint * len(rw)
    cnt, usec = C.c_int(0), C.c_float(0)
    t0 = time.perf_counter()
    if weight_code is None:
        p = L.bnn_mi355x_repair_exposure_campaigns(path, 10, scheme, code, burst, runs, SEED, up(*rw), up(*rt), len(rw), epoch_images, scrub_every,
                                                   repair_every, C.byref(cnt), C.byref(usec))
    else:
        p = L.bnn_mi355x_wecc_exposure_campaigns(path, 10, scheme, code, weight_code, burst, runs, SEED, up(*rw), up(*rt), len(rw), epoch_images,
                                                 scrub_every, repair_every, C.byref(cnt), C.byref(usec))
    wall = time.perf_counter() - t0
    assert p, L.bnn_mi355x_last_error()
    classes = np.ctypeslib.as_array(p, shape=(runs * cnt.value,)).copy().reshape(runs, cnt.value)
    L.free_results(p)
    last = L.bnn_mi355x_last_repair_exposure_counts if weight_code is None else L.bnn_mi355x_last_wecc_exposure_counts
    k = last(None, 0)
    c = (C.c_long * k)()
    last(c, k)
    counts = np.array(c[:], np.int64).reshape(runs, -1, len(rw), 8 if weight_code is None else 12)
    if weight_code is None:
        counts = np.concatenate([counts, np.zeros(counts.shape[:3] + (4,), np.int64)], axis=3)
    return wall * 1e3, usec.value * runs * cnt.value / 1e3, counts, classes


L = gl.load(net)
L.load_parameters(gl.param_dir("cifar10", net).encode())
nl = 9
rw, rt = [RATE] * nl, [RATE] * 8 + [0]
rng = np.random.default_rng(0)
ei = max(n // 100, 1)
print("%s: %d runs x %d random images, every weight and threshold rate 2^-10 per epoch, epochs of %d images" % (net, runs, n, ei))
with tempfile.NamedTemporaryFile(suffix=".bin") as f:
    f.write(np.concatenate([np.ones((n, 1), np.uint8), rng.integers(0, 256, (n, 3072), dtype=np.uint8)], axis=1).tobytes())
    f.flush()
    path = f.name.encode()
    clean = call(L, path, [0] * nl, [0] * nl, 0, 0, None, 1, n, 0, 0)[3][0]
    call(L, path, rw, rt, 1, 0, 1, 1, ei, 10, 1)  # (warm-up: buffers grown, kernels loaded)
    print("timing: ms, best of 3 (by device time), weight_code 1 alternating with the yardstick: repair_exposure_campaigns, same arguments")
    for name, scheme, code in ORGS:
        for cname, every, repair in CONFIGS:
            yard, got = [], []
            for _ in range(3):
                yard.append(call(L, path, rw, rt, scheme, code, None, 1, ei, every, repair))
                got.append(call(L, path, rw, rt, scheme, code, 1, 1, ei, every, repair))
            yb, yw = min(v[1] for v in yard), min(v[0] for v in yard)
            print("%-15s %-38s yardstick wall %8.2f device %8.2f (spread x%.3f: %s) | coded weights wall %8.2f device %8.2f (%s) | device x%.3f of the "
                  "yardstick, wall x%.3f" % (name, cname + ":", yw, yb, max(v[1] for v in yard) / yb, " ".join("%.2f" % v[1] for v in yard),
                                             min(g[0] for g in got), min(g[1] for g in got), " ".join("%.2f" % g[1] for g in got),
                                             min(g[1] for g in got) / yb, min(g[0] for g in got) / yw))
    print("what the code buys: agreement with the fault-free classes in %; after the last epoch: logical bits that differ, weight code words by status")
    for burst in (1, 2):
        for name, scheme, code in ORGS:
            for cname, every, repair in CONFIGS:
                for wc in (None, 1):
                    _, _, counts, classes = call(L, path, rw, rt, scheme, code, wc, burst, ei, every, repair)
                    E = counts.shape[1]
                    agree = [100.0 * (classes[:, t * ei: (t + 1) * ei] == clean[None, t * ei: (t + 1) * ei]).mean() for t in (0, E - 1)]
                    repaired = np.nonzero(counts[..., 10].sum(axis=(0, 2)) + counts[..., 11].sum(axis=(0, 2)))[0]
                    print("burst %d %-15s %-38s %-15s agreement first epoch %6.2f last epoch %6.2f all images %6.2f | logical bits weights %8d "
                          "thresholds %7d | weight code words status 1 %7d status 2 %7d | rewritten by repairs %9d, still unlike the loaded ones "
                          "after the last repair %7d" % (
                              burst, name, cname + ":", "coded weights" if wc else "uncoded weights", agree[0], agree[1],
                              100.0 * (classes == clean[None]).mean(), int(counts[:, -1, :, 1].sum()), int(counts[:, -1, :, 3].sum()),
                              int(counts[:, -1, :, 8].sum()), int(counts[:, -1, :, 9].sum()), int(counts[..., 10].sum()),
                              int(counts[:, repaired[-1], :, 11].sum()) if len(repaired) else 0))
