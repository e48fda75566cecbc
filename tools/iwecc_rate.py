#!/usr/bin/env python3
"""Column-interleaved code words over the coded weight memories (bnn_mi355x_iwecc_exposure_campaigns, weight_interleave 1):
RUNS runs over N random images of cnvW1A1, every weight and threshold rate 2^-10 PER EPOCH, 100 epochs of N/100 images.
Timing, per organisation (TMR; scheme 0 + SEC-DED thresholds), burst (1, 2) and schedule (rewrite every epoch; repair every
epoch; repair every epoch + rewrite every 10; never): the yardstick is bnn_mi355x_wecc_exposure_campaigns with weight_code
1 and the same arguments, and against it, on the same images, seeds and rates, iwecc_exposure_campaigns with
weight_interleave 1.  The two calls alternate in one process, three rounds, best of three by device time.  Per
configuration: wall and device time, the ratio to the yardstick, next to the yardstick's own run-to-run spread (worst /
best of its three device times).
What the interleave buys: from the same calls, coded and coded + interleaved: the agreement with the fault-free classes
over the first epoch, the last epoch and all images, the logical weight bits that differ after the last epoch, and the
weight code words at status 1 and 2 after the last epoch.
usage: iwecc_rate.py [n_images [runs [network]]]"""
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


def call(L, path, rw, rt, scheme, code, interleave, burst, epoch_images, scrub_every, repair_every):
    """interleave None: wecc_exposure_campaigns with weight_code 1, the yardstick.
    -> (wall ms, device ms, counts [run, epoch, layer, 12], classes)"""
    up = C.c_uint * len(rw)
    cnt, usec = C.c_int(0), C.c_float(0)
    t0 = time.perf_counter()
    if interleave is None:
        p = L.bnn_mi355x_wecc_exposure_campaigns(path, 10, scheme, code, 1, burst, runs, SEED, up(*rw), up(*rt), len(rw), epoch_images,
                                                 scrub_every, repair_every, C.byref(cnt), C.byref(usec))
    else:
        p = L.bnn_mi355x_iwecc_exposure_campaigns(path, 10, scheme, code, 1, interleave, burst, runs, SEED, up(*rw), up(*rt), len(rw),
                                                  epoch_images, scrub_every, repair_every, C.byref(cnt), C.byref(usec))
    wall = time.perf_counter() - t0
    assert p, L.bnn_mi355x_last_error()
    classes = np.ctypeslib.as_array(p, shape=(runs * cnt.value,)).copy().reshape(runs, cnt.value)
    L.free_results(p)
    last = L.bnn_mi355x_last_wecc_exposure_counts if interleave is None else L.bnn_mi355x_last_iwecc_exposure_counts
    k = last(None, 0)
    c = (C.c_long * k)()
    last(c, k)
    return wall * 1e3, usec.value * runs * cnt.value / 1e3, np.array(c[:], np.int64).reshape(runs, -1, len(rw), 12), classes


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
    print("ms, best of 3 (by device time), weight_interleave 1 alternating with the yardstick: wecc_exposure_campaigns (weight_code 1), same arguments")
    rows = []
    for burst in (1, 2):
        for name, scheme, code in ORGS:
            for cname, every, repair in CONFIGS:
                yard, got = [], []
                for _ in range(3):
                    yard.append(call(L, path, rw, rt, scheme, code, None, burst, ei, every, repair))
                    got.append(call(L, path, rw, rt, scheme, code, 1, burst, ei, every, repair))
                yb, yw = min(v[1] for v in yard), min(v[0] for v in yard)
                print("burst %d %-15s %-38s yardstick wall %8.2f device %8.2f (spread x%.3f: %s) | interleaved wall %8.2f device %8.2f (%s) | device "
                      "x%.3f of the yardstick, wall x%.3f" % (burst, name, cname + ":", yw, yb, max(v[1] for v in yard) / yb,
                                                              " ".join("%.2f" % v[1] for v in yard), min(g[0] for g in got), min(g[1] for g in got),
                                                              " ".join("%.2f" % g[1] for g in got), min(g[1] for g in got) / yb,
                                                              min(g[0] for g in got) / yw))
                assert (yard[0][2][..., 0] == got[0][2][..., 0]).all()  # the events are the same
                for what, (_, _, counts, classes) in (("coded weights", yard[0]), ("coded + interleaved", got[0])):
                    E = counts.shape[1]
                    agree = [100.0 * (classes[:, t * ei: (t + 1) * ei] == clean[None, t * ei: (t + 1) * ei]).mean() for t in (0, E - 1)]
                    rows.append("burst %d %-15s %-38s %-20s agreement first epoch %6.2f last epoch %6.2f all images %6.2f | logical weight bits %8d | "
                                "weight code words status 1 %7d status 2 %7d | rewritten by repairs %9d" % (
                                    burst, name, cname + ":", what, agree[0], agree[1], 100.0 * (classes == clean[None]).mean(),
                                    int(counts[:, -1, :, 1].sum()), int(counts[:, -1, :, 8].sum()), int(counts[:, -1, :, 9].sum()),
                                    int(counts[..., 10].sum())))
    print("what the interleave buys: agreement with the fault-free classes in %; after the last epoch: logical weight bits that differ, weight code "
          "words by status")
    print("\n".join(rows))
