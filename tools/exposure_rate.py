#!/usr/bin/env python3
"""Exposure campaigns (bnn_mi355x_exposure_campaigns): RUNS runs over N random images of cnvW1A1, every weight and
threshold rate 2^-10 PER EPOCH, schemes 0 (none) and 1 (TMR), epochs of N / N/10 / N/100 images, scrub_every 0 and 1.
Every configuration alternates in one process with bnn_mi355x_hardened_mem_noise_campaigns on the same images, scheme and
rates (the yardstick: all upsets before the first image), best of three calls each.  Per configuration: wall and device
time of both, the ratio of the device times, the yardstick's own run-to-run spread (worst / best of its three device
times), and the host's layer-0 share: 1 - wall(the same call with layer 0's two rates 0, so that the host steps no
physical state and uploads no patches) / wall.  Also the physical bits flipped over all epochs, the logical bits that
differ after the last epoch, and the agreement with the fault-free classes in the first and the last epoch.
usage: exposure_rate.py [n_images [runs [network]]]"""
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
NAMES = ("none", "TMR", "interleaved", "resilient-interleaved")


def call(L, path, rw, rt, scheme, epoch_images=None, scrub_every=0):
    """epoch_images None: the hardened campaign.  -> (wall ms, device ms, counts, classes)"""
    up = C.c_uint * len(rw)
    cnt, usec = C.c_int(0), C.c_float(0)
    t0 = time.perf_counter()
    if epoch_images is None:
        p = L.bnn_mi355x_hardened_mem_noise_campaigns(path, 10, scheme, 1, runs, SEED, up(*rw), up(*rt), len(rw), C.byref(cnt), C.byref(usec))
    else:
        p = L.bnn_mi355x_exposure_campaigns(path, 10, scheme, 1, runs, SEED, up(*rw), up(*rt), len(rw), epoch_images, scrub_every, C.byref(cnt),
                                            C.byref(usec))
    wall = time.perf_counter() - t0
    assert p, L.bnn_mi355x_last_error()
    classes = np.ctypeslib.as_array(p, shape=(runs * cnt.value,)).copy().reshape(runs, cnt.value)
    L.free_results(p)
    last = L.bnn_mi355x_last_hardened_mem_noise_counts if epoch_images is None else L.bnn_mi355x_last_exposure_counts
    k = last(None, 0)
    c = (C.c_long * k)()
    last(c, k)
    return wall * 1e3, usec.value * runs * cnt.value / 1e3, np.array(c[:], np.int64).reshape(runs, -1, len(rw), 2, 2), classes


L = gl.load(net)
L.load_parameters(gl.param_dir("cifar10", net).encode())
nl = 9
rw, rt = [RATE] * nl, [RATE] * 8 + [0]
rw0, rt0 = [0] + rw[1:], [0] + rt[1:]  # (layer 0 left alone: nothing for the host to step)
rng = np.random.default_rng(0)
print("%s: %d runs x %d random images, every weight and threshold rate 2^-10 per epoch, burst 1; ms, best of 3 (by device time), "
      "each configuration alternating with hardened_mem_noise_campaigns" % (net, runs, n))
with tempfile.NamedTemporaryFile(suffix=".bin") as f:
    f.write(np.concatenate([np.ones((n, 1), np.uint8), rng.integers(0, 256, (n, 3072), dtype=np.uint8)], axis=1).tobytes())
    f.flush()
    path = f.name.encode()
    clean = call(L, path, [0] * nl, [0] * nl, 0)[3][0]
    call(L, path, rw, rt, 1, max(n // 10, 1), 1)  # (warm-up: buffers grown, kernels loaded)
    for scheme in (0, 1):
        for ei in (n, max(n // 10, 1), max(n // 100, 1)):
            for every in (0, 1):
                hard, expo, bare = [], [], []
                for _ in range(3):
                    hard.append(call(L, path, rw, rt, scheme))
                    expo.append(call(L, path, rw, rt, scheme, ei, every))
                    bare.append(call(L, path, rw0, rt0, scheme, ei, every))
                h, x, b = (min(v, key=lambda g: g[1]) for v in (hard, expo, bare))
                E = x[2].shape[1]
                agree = [100.0 * (x[3][:, t * ei: (t + 1) * ei] == clean[None, t * ei: (t + 1) * ei]).mean() for t in (0, E - 1)]
                print("%-5s epochs of %5d (%4d) scrub_every %d: wall %9.2f device %8.2f | hardened wall %7.2f device %6.2f (spread x%.3f) | "
                      "device x%.3f of hardened | host layer-0 share of wall %5.1f %% | physical bits %9d, logical after the last epoch %9d | "
                      "agreement first / last epoch %6.2f / %6.2f %%" % (
                          NAMES[scheme], ei, E, every, x[0], x[1], h[0], h[1], max(g[1] for g in hard) / h[1], x[1] / h[1],
                          100.0 * (1.0 - min(g[0] for g in bare) / min(g[0] for g in expo)), int(x[2][..., 0].sum()), int(x[2][:, -1, :, :, 1].sum()),
                          agree[0], agree[1]))
