#!/usr/bin/env python3
"""tools/lfc_mfma_rate.py [NETWORK ...]: the LFC nets' matrix-core form (BNN_MI355X_LFC=mfma, k_lfc_mfma) against the default
route of the same build, in ONE process: the python_sw library is loaded as shipped, the python_hw library (the same object
under its second name: a runtime of its own) with the switch and BNN_MI355X_LFC_MFMA_MIN=1.  Resident images through
bnn_mi355x_inference_device; per size seven rounds that alternate the two routes, each a window of back-to-back calls of
about 0.1 s closed by a device synchronise (wall time per call, launch gaps included); medians, best of seven, and the
default route's own spread (max - min over its rounds).  The two routes' words are compared at every size first.  Then the
per-stage HIP-event times at 10 000 and 131 072 images (profiling on: the default route's staged kernels at every size).
This is what profiles/r38_lfc_mfma_rate.txt records."""
import ctypes as C
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import gpu_lib as gl  # noqa: E402

SIZES = (1024, 4096, 10000, 32768, 131072)
ROUNDS = 7


def window(call, reps):
    t0 = time.perf_counter()
    for _ in range(reps):
        call()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e6


def stages(L, call, reps):
    L.bnn_mi355x_profile(1)
    for _ in range(reps):
        call()
    torch.cuda.synchronize()
    ms, nc = (C.c_float * 16)(), C.c_int(0)
    k = L.bnn_mi355x_profile_read(ms, 16, C.byref(nc))
    L.bnn_mi355x_profile(0)
    return " ".join("%s=%.1f" % (L.bnn_mi355x_stage_name(i).decode().replace(" ", "_"), ms[i] / reps * 1e3) for i in range(k))


for net in sys.argv[1:] or ("lfcW1A1", "lfcW1A2"):
    pdir = gl.param_dir("mnist", net).encode()
    libs = {"default": gl.load(net), "matrix": gl.load(net, "python_hw")}
    libs["default"].load_parameters(pdir)
    os.environ["BNN_MI355X_LFC"], os.environ["BNN_MI355X_LFC_MFMA_MIN"] = "mfma", "1"
    libs["matrix"].load_parameters(pdir)
    del os.environ["BNN_MI355X_LFC"], os.environ["BNN_MI355X_LFC_MFMA_MIN"]
    for n in SIZES:
        assert libs["default"].bnn_mi355x_matrix_stages(n) == 0 and libs["matrix"].bnn_mi355x_matrix_stages(n) == 0x1E
        imgs = torch.randint(0, 256, (n, 784), dtype=torch.uint8, device="cuda")
        out = {k: (torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(n, dtype=torch.int64, device="cuda")) for k in libs}
        s = torch.cuda.current_stream().cuda_stream

        def caller(k):
            L, (cls, words) = libs[k], out[k]
            def call():
                assert L.bnn_mi355x_inference_device(imgs.data_ptr(), n, 10, cls.data_ptr(), None, words.data_ptr(), s) == 0
            return call
        calls = {k: caller(k) for k in libs}
        for k in libs:  # warm-up, and the calibration of the window
            for _ in range(5):
                calls[k]()
        torch.cuda.synchronize()
        assert bool((out["default"][1] == out["matrix"][1]).all()) and bool((out["default"][0] == out["matrix"][0]).all()), (net, n, "routes differ")
        reps = {k: max(10, min(5000, int(1e5 / window(calls[k], 10)))) for k in libs}
        t = {k: [] for k in libs}
        for _ in range(ROUNDS):
            for k in libs:
                t[k].append(window(calls[k], reps[k]))
        med = {k: statistics.median(t[k]) for k in libs}
        print("%s n=%d us/call: default median %.1f best %.1f spread %.1f | matrix median %.1f best %.1f | default / matrix %.3f (median) %.3f (best)"
              % (net, n, med["default"], min(t["default"]), max(t["default"]) - min(t["default"]), med["matrix"], min(t["matrix"]),
                 med["default"] / med["matrix"], min(t["default"]) / min(t["matrix"])), flush=True)
        if n in (10000, 131072):
            for k in libs:
                print("%s n=%d stage events, %s, us: %s" % (net, n, k, stages(libs[k], calls[k], 20)), flush=True)
