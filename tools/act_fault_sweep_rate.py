#!/usr/bin/env python3
"""Activation-fault sweeps (bnn_mi355x_act_fault_sweep): every site x shift of every non-last layer, one whole layer
per call, on N random images, for cnvW1A1, cnvW2A2 and lfcW1A1.  Per layer: wall and device time, (site, image) pairs
per second of wall time, the share of sites that change some image, and the pairs each layer had to run
(bnn_mi355x_last_act_sweep_stages).
--window-ab: the windowed first stage of CNV site layers 0-2 against the dense one in ONE process: per
(net, site layer) every site x shift of the layer in one call, the switch BNN_MI355X_ACT_WINDOW alternating off / on for
`reps` rounds; wall time of every call, the medians' ratio, and the spread between repeats of the same route.
usage: act_fault_sweep_rate.py [n_images]
       act_fault_sweep_rate.py --window-ab [n_images] [reps]"""
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

window_ab = len(sys.argv) > 1 and sys.argv[1] == "--window-ab"
args = sys.argv[2:] if window_ab else sys.argv[1:]
n = int(args[0]) if args else 1000
reps = int(args[1]) if len(args) > 1 else 3
ip = C.POINTER(C.c_int)
NETS = ["cnvW1A1", "cnvW2A2", "lfcW1A1"]


def sites(L, layer):
    k = L.bnn_mi355x_enumerate_act_faults(layer, 0, None, 0)
    rec = np.zeros((k, 5), np.int32)
    L.bnn_mi355x_enumerate_act_faults(layer, 0, rec.ctypes.data_as(ip), k)
    return rec


def sweep(L, path, recs):
    k = len(recs)
    changed = np.zeros(k, np.int32)
    cnt, usec = C.c_int(0), C.c_float(0)
    t0 = time.perf_counter()
    total = L.bnn_mi355x_act_fault_sweep(path, 10, recs.ctypes.data_as(ip), k, changed.ctypes.data_as(ip), None, 0,
                                         C.byref(cnt), C.byref(usec))
    wall = time.perf_counter() - t0
    assert total >= 0, L.bnn_mi355x_last_error()
    s = L.bnn_mi355x_last_act_sweep_stages(None, 0)
    st = (C.c_long * s)()
    L.bnn_mi355x_last_act_sweep_stages(st, s)
    return wall * 1e3, usec.value * k * cnt.value / 1e3, list(st), changed


def image_file(f, cnv):
    if cnv:
        f.write(np.concatenate([np.ones((n, 1), np.uint8), rng.integers(0, 256, (n, 3072), dtype=np.uint8)], axis=1).tobytes())
    else:
        f.write(struct.pack(">4I", 0x803, n, 28, 28) + rng.integers(0, 256, (n, 784), dtype=np.uint8).tobytes())
    f.flush()
    return f.name.encode()


def window_ab_mode():
    """dense (BNN_MI355X_ACT_WINDOW=0, the route before the window kernels) and windowed calls alternate; a case counts as
    faster only if the gap between the routes' medians exceeds the spread (max - min) of either route's repeats"""
    print("windowed vs dense first stage, %d random images, every site x shift of the layer per call, %d alternations; ms wall" % (n, reps))
    for net in ["cnvW1A1", "cnvW1A2", "cnvW2A2"]:
        L = gl.load(net)
        L.load_parameters(gl.param_dir("cifar10", net).encode())
        with tempfile.NamedTemporaryFile(dir="/tmp", suffix=".bin") as f:
            path = image_file(f, True)
            for layer in range(3):
                recs = sites(L, layer)
                t = {"0": [], "1": []}
                dev = {"0": [], "1": []}
                ref = None
                for sw in ("0", "1"):  # (warm-up of both routes: buffers grown, kernels loaded)
                    os.environ["BNN_MI355X_ACT_WINDOW"] = sw
                    sweep(L, path, recs[:64])
                for _ in range(reps):
                    for sw in ("0", "1"):
                        os.environ["BNN_MI355X_ACT_WINDOW"] = sw
                        wall, d, st, changed = sweep(L, path, recs)
                        t[sw].append(wall)
                        dev[sw].append(d)
                        if ref is None:
                            ref = (st, changed.copy())
                        assert st == ref[0] and (changed == ref[1]).all(), "the routes disagree"
                md, mw = float(np.median(t["0"])), float(np.median(t["1"]))
                spread = max(max(t["0"]) - min(t["0"]), max(t["1"]) - min(t["1"]))
                verdict = "windowed faster" if md - mw > spread else "NOT faster beyond the spread: stays dense by policy"
                print("%s L%d %7d sites x shifts: dense %s | windowed %s" % (
                    net, layer, len(recs), " ".join("%.1f" % x for x in t["0"]), " ".join("%.1f" % x for x in t["1"])))
                print("    medians %.1f / %.1f ms = x%.2f (device %.1f / %.1f), spread %.1f ms: %s; %.1f -> %.1f M pairs/s" % (
                    md, mw, md / mw, float(np.median(dev["0"])), float(np.median(dev["1"])), spread, verdict,
                    len(recs) * n / md / 1e3, len(recs) * n / mw / 1e3))
                sys.stdout.flush()
        os.environ.pop("BNN_MI355X_ACT_WINDOW", None)


rng = np.random.default_rng(0)
if window_ab:
    window_ab_mode()
    sys.exit(0)
print("activation-fault sweeps on %d random images: every site x shift of the layer's output in one call; ms" % n)
for net in NETS:
    cnv = net.startswith("cnv")
    L = gl.load(net)
    L.load_parameters(gl.param_dir("cifar10" if cnv else "mnist", net).encode())
    with tempfile.NamedTemporaryFile(dir="/tmp", suffix=".bin") as f:
        path = image_file(f, cnv)
        sweep(L, path, sites(L, 0)[:64])  # (warm-up: buffers grown, kernels loaded)
        all_wall = all_dev = all_pairs = 0.0
        for layer in range(8 if cnv else 3):
            recs = sites(L, layer)
            wall, dev, st, changed = sweep(L, path, recs)
            pairs = len(recs) * n
            all_wall, all_dev, all_pairs = all_wall + wall, all_dev + dev, all_pairs + pairs
            print("%s L%d %8d sites x shifts: %9.1f ms wall (device %9.1f)  %6.1f M pairs/s  %5.1f%% change an image" % (
                net, layer, len(recs), wall, dev, pairs / wall / 1e3, 100.0 * (changed > 0).mean()))
            print("    pairs per layer: " + " ".join("%d" % x for x in st))
            sys.stdout.flush()
        print("%s all layers: %.1f ms wall (device %.1f), %.1f M pairs/s" % (net, all_wall, all_dev, all_pairs / all_wall / 1e3))
