#!/usr/bin/env python3
"""SEC-DED coded threshold memories in the exposure campaigns (bnn_mi355x_ecc_exposure_campaigns): RUNS runs over N random
images of cnvW1A1, every weight and threshold rate 2^-10 PER EPOCH.
Timing: code 1 under schemes 0 and 2 (burst 1) against bnn_mi355x_exposure_campaigns on the same images, scheme and rates
(the yardstick: the same campaign without the code), the calls alternating in one process, best of three by device time;
1 epoch and 10 epochs.  Per configuration: wall and device time of both, the ratio of the device times and the
yardstick's own run-to-run spread (worst / best of its three device times).
What the code is for: layer 0's rates at 0 (it is not coded), 100 epochs of N/100 images, scrub_every 0 and 1, bursts 1, 2
and 4, for (scheme, code) = (0, 0), (0, 1), (2, 0), (2, 1): the agreement with the fault-free classes over the first
epoch, the last epoch and all images, the physical bits flipped, the logical threshold bits that differ after the last
epoch, and the threshold words corrected / detected after it.
usage: ecc_rate.py [n_images [runs [network]]]"""
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


def call(L, path, rw, rt, scheme, code, burst, epoch_images, scrub_every=0):
    """code None: exposure_campaigns (counts widened to six).  -> (wall ms, device ms, counts [run, epoch, layer, 6], classes)"""
    up = C.c_uint * len(rw)
    cnt, usec = C.c_int(0), C.c_float(0)
    t0 = time.perf_counter()
    if code is None:
        p = L.bnn_mi355x_exposure_campaigns(path, 10, scheme, burst, runs, SEED, up(*rw), up(*rt), len(rw), epoch_images, scrub_every, C.byref(cnt),
                                            C.byref(usec))
    else:
        p = L.bnn_mi355x_ecc_exposure_campaigns(path, 10, scheme, code, burst, runs, SEED, up(*rw), up(*rt), len(rw), epoch_images, scrub_every,
                                                C.byref(cnt), C.byref(usec))
    wall = time.perf_counter() - t0
    assert p, L.bnn_mi355x_last_error()
    classes = np.ctypeslib.as_array(p, shape=(runs * cnt.value,)).copy().reshape(runs, cnt.value)
    L.free_results(p)
    last = L.bnn_mi355x_last_exposure_counts if code is None else L.bnn_mi355x_last_ecc_exposure_counts
    k = last(None, 0)
    c = (C.c_long * k)()
    last(c, k)
    counts = np.array(c[:], np.int64).reshape(runs, -1, len(rw), 4 if code is None else 6)
    if code is None:
        counts = np.concatenate([counts, np.zeros(counts.shape[:3] + (2,), np.int64)], axis=3)
    return wall * 1e3, usec.value * runs * cnt.value / 1e3, counts, classes


L = gl.load(net)
L.load_parameters(gl.param_dir("cifar10", net).encode())
nl = 9
rw, rt = [RATE] * nl, [RATE] * 8 + [0]
rw0, rt0 = [0] + rw[1:], [0] + rt[1:]  # (layer 0 left alone: it is not coded)
rng = np.random.default_rng(0)
print("%s: %d runs x %d random images, every weight and threshold rate 2^-10 per epoch" % (net, runs, n))
with tempfile.NamedTemporaryFile(suffix=".bin") as f:
    f.write(np.concatenate([np.ones((n, 1), np.uint8), rng.integers(0, 256, (n, 3072), dtype=np.uint8)], axis=1).tobytes())
    f.flush()
    path = f.name.encode()
    clean = call(L, path, [0] * nl, [0] * nl, 0, 1, 1, n)[3][0]
    call(L, path, rw, rt, 2, 1, 1, max(n // 10, 1), 1)  # (warm-up: buffers grown, kernels loaded)
    print("timing: ms, best of 3 (by device time), code 1 alternating with exposure_campaigns (the same campaign without the code), burst 1")
    for scheme in (0, 2):
        for ei in (n, max(n // 10, 1)):
            base, coded = [], []
            for _ in range(3):
                base.append(call(L, path, rw, rt, scheme, None, 1, ei))
                coded.append(call(L, path, rw, rt, scheme, 1, 1, ei))
            b, x = (min(v, key=lambda g: g[1]) for v in (base, coded))
            print("%-11s + SEC-DED epochs of %5d (%3d): wall %8.2f device %8.2f | exposure_campaigns wall %8.2f device %8.2f (spread x%.3f) | "
                  "device x%.3f of exposure_campaigns, wall x%.3f" % (NAMES[scheme], ei, x[2].shape[1], x[0], x[1], b[0], b[1],
                                                                     max(g[1] for g in base) / b[1], x[1] / b[1],
                                                                     min(g[0] for g in coded) / min(g[0] for g in base)))
    ei = max(n // 100, 1)
    print("what the code buys: layer 0's rates 0, epochs of %d images, agreement with the fault-free classes in %%" % ei)
    for burst in (1, 2, 4):
        for every in (0, 1):
            for scheme, code in ((0, 0), (0, 1), (2, 0), (2, 1)):
                _, _, counts, classes = call(L, path, rw0, rt0, scheme, code, burst, ei, every)
                E = counts.shape[1]
                agree = [100.0 * (classes[:, t * ei: (t + 1) * ei] == clean[None, t * ei: (t + 1) * ei]).mean() for t in (0, E - 1)]
                print("burst %d scrub_every %d %-11s code %d: agreement first epoch %6.2f last epoch %6.2f all images %6.2f | physical bits %9d "
                      "(thresholds %7d) | after the last epoch: logical threshold bits %6d, words corrected %6d, detected %6d" % (
                          burst, every, NAMES[scheme], code, agree[0], agree[1], 100.0 * (classes == clean[None]).mean(),
                          int(counts[..., [0, 2]].sum()), int(counts[..., 2].sum()), int(counts[:, -1, :, 3].sum()), int(counts[:, -1, :, 4].sum()),
                          int(counts[:, -1, :, 5].sum())))
