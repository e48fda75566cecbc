#!/usr/bin/env python3
"""Input-buffer upset-rate campaigns (bnn_mi355x_input_noise_campaigns): RUNS runs over N random images for cnvW1A1,
cnvW2A2 and lfcW1A1 at rate 0 (the yardstick: the same pairs through the same passes, no upset launch), 2^-10 and 2^-4.
Per rate: wall and device time (best of three calls), pairs per second, the ratio to rate 0, the flips counted on the
device against bits x pairs x rate.  Then one whole-image sweep (bnn_mi355x_input_fault_sweep, every bit of the image)
of cnvW1A1 on the N images: wall and device time and the pairs that had to run each layer.
usage: input_noise_rate.py [n_images [runs [network ...]]]     (one call per rate only: input_noise_rate.py N RUNS NET once)
The record: python tools/input_noise_rate.py > profiles/r12_input_noise_rate.txt"""
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
ip = C.POINTER(C.c_int)


def campaign(L, path, rate):
    cnt, usec = C.c_int(0), C.c_float(0)
    t0 = time.perf_counter()
    p = L.bnn_mi355x_input_noise_campaigns(path, 10, runs, 12345, rate, C.byref(cnt), C.byref(usec))
    wall = time.perf_counter() - t0
    assert p, L.bnn_mi355x_last_error()
    L.free_results(p)
    c = (C.c_long * runs)()
    L.bnn_mi355x_last_input_noise_counts(c, runs)
    return wall * 1e3, usec.value * runs * cnt.value / 1e3, int(np.sum(c[:]))


def write_set(f, cnv, imgs):
    if cnv:
        f.write(np.concatenate([np.ones((len(imgs), 1), np.uint8), imgs], axis=1).tobytes())
    else:
        f.write(struct.pack(">4I", 0x803, len(imgs), 28, 28) + imgs.tobytes())
    f.flush()


rng = np.random.default_rng(0)
print("input upset-rate campaigns: %d runs x %d random images; ms, best of %d" % (runs, n, 1 if once else 3))
for net in NETS:
    cnv = net.startswith("cnv")
    L = gl.load(net)
    L.load_parameters(gl.param_dir("cifar10" if cnv else "mnist", net).encode())
    bits = L.bnn_mi355x_image_bytes() * 8
    with tempfile.NamedTemporaryFile(suffix=".bin") as f:
        write_set(f, cnv, rng.integers(0, 256, (n, bits // 8), dtype=np.uint8))
        path = f.name.encode()
        if not once:
            campaign(L, path, 1 << 22)  # (warm-up: buffers grown, kernels loaded)
        base = None
        for rate, name in RATES:
            best = min(campaign(L, path, rate) for _ in range(1 if once else 3))
            base = base or best
            print("%s rate %-6s %9.1f ms wall, device %9.1f  %7.1f M pairs/s  x%.2f of rate 0 (device)  flips %d (bits x pairs x rate %.0f)" % (
                net, name, best[0], best[1], runs * n / best[0] / 1e3, best[1] / base[1], best[2],
                float(bits) * runs * n * rate / 2.0 ** 32))
            sys.stdout.flush()
        if net != "cnvW1A1" or once:
            continue
        # every bit of the image, each alone on the n images
        rec = np.stack([np.arange(bits) >> 3, np.arange(bits) & 7], axis=1).astype(np.int32)
        changed = np.zeros(bits, np.int32)
        cnt, usec = C.c_int(0), C.c_float(0)
        t0 = time.perf_counter()
        total = L.bnn_mi355x_input_fault_sweep(path, 10, rec.ctypes.data_as(ip), bits, changed.ctypes.data_as(ip), None, 0, C.byref(cnt),
                                               C.byref(usec))
        wall = time.perf_counter() - t0
        assert total >= 0, L.bnn_mi355x_last_error()
        st = (C.c_long * 9)()
        L.bnn_mi355x_last_input_sweep_stages(st, 9)
        pairs = bits * cnt.value
        print("%s whole-image sweep: %d sites x %d images = %d pairs, %.2f s wall, %.2f s device, %.1f M pairs/s; %d pairs change the class, "
              "%d sites change some image" % (net, bits, cnt.value, pairs, wall, usec.value * pairs / 1e6, pairs / wall / 1e6, total,
                                              int((changed > 0).sum())))
        print("%s pairs that ran each layer: %s" % (net, " ".join("L%d %d (%.2f %%)" % (l, st[l], 100.0 * st[l] / pairs) for l in range(9))))
        print("%s sites that change some image, by bit 0..7: %s" % (net, (changed.reshape(-1, 8) > 0).sum(axis=0).tolist()))
        sys.stdout.flush()
