#!/usr/bin/env python3
"""Repair scrubs in the exposure campaigns (bnn_mi355x_repair_exposure_campaigns): RUNS runs over N random images of
cnvW1A1, every weight and threshold rate 2^-10 PER EPOCH, 100 epochs of N/100 images.
Timing, per organisation (TMR; scheme 0 + SEC-DED; interleaved + SEC-DED; burst 1): the yardstick is
bnn_mi355x_ecc_exposure_campaigns with scrub_every 1 -- a full rewrite before every epoch -- and against it, on the same
images, seeds and rates: repair_every 1; repair_every 1 with scrub_every 10; neither.  The four calls alternate in one
process, three rounds, best of three by device time.  Per configuration: wall and device time, their ratios to the
yardstick, next to the yardstick's own run-to-run spread (worst / best of its three device times).
What each scrub buys: the same four configurations at bursts 1 and 2: the agreement with the fault-free classes over the
first epoch, the last epoch and all images, the logical bits that differ after the last epoch (weights, thresholds), and
over all epochs the words the repairs rewrote and, after the last repair, the words still unlike the loaded ones.
usage: repair_rate.py [n_images [runs [network]]]"""
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
ORGS = (("TMR", 1, 0), ("none + SEC-DED", 0, 1), ("interleaved + SEC-DED", 2, 1))
# (name, scrub_every, repair_every); None: ecc_exposure_campaigns, the yardstick
CONFIGS = (("rewrite every epoch", 1, None), ("repair every epoch", 0, 1), ("repair every epoch + rewrite every 10", 10, 1), ("never", 0, 0))


def call(L, path, rw, rt, scheme, code, burst, epoch_images, scrub_every, repair_every):
    """repair_every None: ecc_exposure_campaigns (counts widened to eight).  -> (wall ms, device ms, counts [run, epoch, layer, 8], classes)"""
    up = C.c_uint * len(rw)
    cnt, usec = C.c_int(0), C.c_float(0)
    t0 = time.perf_counter()
    if repair_every is None:
        p = L.bnn_mi355x_ecc_exposure_campaigns(path, 10, scheme, code, burst, runs, SEED, up(*rw), up(*rt), len(rw), epoch_images, scrub_every,
                                                C.byref(cnt), C.byref(usec))
    else:
        p = L.bnn_mi355x_repair_exposure_campaigns(path, 10, scheme, code, burst, runs, SEED, up(*rw), up(*rt), len(rw), epoch_images, scrub_every,
                                                   repair_every, C.byref(cnt), C.byref(usec))
    wall = time.perf_counter() - t0
    assert p, L.bnn_mi355x_last_error()
    classes = np.ctypeslib.as_array(p, shape=(runs * cnt.value,)).copy().reshape(runs, cnt.value)
    L.free_results(p)
    last = L.bnn_mi355x_last_ecc_exposure_counts if repair_every is None else L.bnn_mi355x_last_repair_exposure_counts
    k = last(None, 0)
    c = (C.c_long * k)()
    last(c, k)
    counts = np.array(c[:], np.int64).reshape(runs, -1, len(rw), 6 if repair_every is None else 8)
    if repair_every is None:
        counts = np.concatenate([counts, np.zeros(counts.shape[:3] + (2,), np.int64)], axis=3)
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
    clean = call(L, path, [0] * nl, [0] * nl, 0, 0, 1, n, 0, 0)[3][0]
    call(L, path, rw, rt, 1, 0, 1, ei, 10, 1)  # (warm-up: buffers grown, kernels loaded)
    print("timing: ms, best of 3 (by device time), the four configurations alternating; the yardstick is ecc_exposure_campaigns with scrub_every 1")
    for name, scheme, code in ORGS:
        got = {c[0]: [] for c in CONFIGS}
        for _ in range(3):
            for cname, every, repair in CONFIGS:
                got[cname].append(call(L, path, rw, rt, scheme, code, 1, ei, every, repair))
        yard = got[CONFIGS[0][0]]
        yb = min(v[1] for v in yard)
        yw = min(v[0] for v in yard)
        print("%-21s yardstick (rewrite every epoch): wall %8.2f device %8.2f (spread x%.3f: %s)" % (
            name, yw, yb, max(v[1] for v in yard) / yb, " ".join("%.2f" % v[1] for v in yard)))
        for cname, _, _ in CONFIGS[1:]:
            v = got[cname]
            print("%-21s %-38s wall %8.2f device %8.2f | device x%.3f of the yardstick, wall x%.3f" % (
                name, cname + ":", min(g[0] for g in v), min(g[1] for g in v), min(g[1] for g in v) / yb, min(g[0] for g in v) / yw))
    print("what each scrub buys: agreement with the fault-free classes in %; after the last epoch: logical bits that differ")
    for burst in (1, 2):
        for name, scheme, code in ORGS:
            for cname, every, repair in CONFIGS:
                _, _, counts, classes = call(L, path, rw, rt, scheme, code, burst, ei, every, repair)
                E = counts.shape[1]
                agree = [100.0 * (classes[:, t * ei: (t + 1) * ei] == clean[None, t * ei: (t + 1) * ei]).mean() for t in (0, E - 1)]
                repaired = np.nonzero(counts[..., 6].sum(axis=(0, 2)) + counts[..., 7].sum(axis=(0, 2)))[0]
                print("burst %d %-21s %-38s agreement first epoch %6.2f last epoch %6.2f all images %6.2f | logical bits weights %8d "
                      "thresholds %7d | words rewritten by repairs %8d, still unlike the loaded ones after the last repair %6d" % (
                          burst, name, cname + ":", agree[0], agree[1], 100.0 * (classes == clean[None]).mean(), int(counts[:, -1, :, 1].sum()),
                          int(counts[:, -1, :, 3].sum()), int(counts[..., 6].sum()), int(counts[:, repaired[-1], :, 7].sum()) if len(repaired) else 0))
