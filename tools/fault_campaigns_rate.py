#!/usr/bin/env python3
"""Wall time of a fault study of R runs: sequential (load_parameters + one inference_multiple_with_faults per run, the
Fault Testing notebook's loop) against batched (ONE bnn_mi355x_fault_campaigns call: the runs side by side on the GPU).
Both compute the same classes (checked here on the first configuration).  Median of `reps` repetitions.
usage: fault_campaigns_rate.py [runs [n_images [reps]]]"""
import ctypes as C, os, sys, tempfile, time
import numpy as np
import torch  # noqa: F401
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gpu_lib as gl
R = int(sys.argv[1]) if len(sys.argv) > 1 else 100
n = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
rng = np.random.default_rng(0)
print("fault study: %d runs x %d images, seeds 1000 + r, any target, bit flips; wall ms, median of %d" % (R, n, reps))
for net in ("cnvW1A1", "lfcW1A1"):
    cnv = net.startswith("cnv")
    L = gl.load(net)
    pdir = gl.param_dir("cifar10" if cnv else "mnist", net).encode()
    with tempfile.NamedTemporaryFile(dir="/tmp", suffix=".bin") as f:
        if cnv:
            f.write(rng.integers(0, 256, (n, 3073), dtype=np.uint8).tobytes())
        else:
            f.write((0x803).to_bytes(4, "big") + n.to_bytes(4, "big") + (28).to_bytes(4, "big") * 2)
            f.write(rng.integers(0, 256, (n, 784), dtype=np.uint8).tobytes())
        f.flush()
        path = f.name.encode()
        for flips in (10, 100):
            cnt, usec = C.c_int(0), C.c_float(0)
            seq_t, bat_t, seq_res, bat_res, dev_us = [], [], None, None, []
            for rep in range(reps):
                rows = []
                t0 = time.perf_counter()
                for r in range(R):
                    L.load_parameters(pdir)
                    L.bnn_mi355x_set_fault_seed(1000 + r)
                    p = L.inference_multiple_with_faults(path, 10, C.byref(cnt), None, flips, 1, -1, None, 0)
                    assert p and cnt.value == n
                    rows.append(np.ctypeslib.as_array(p, shape=(n,)).copy())
                    L.free_results(p)
                seq_t.append(time.perf_counter() - t0)
                seq_res = np.stack(rows)
                L.load_parameters(pdir)
                L.bnn_mi355x_set_fault_seed(0)
                t0 = time.perf_counter()
                p = L.bnn_mi355x_fault_campaigns(path, 10, R, 1000, flips, 1, -1, None, 0, C.byref(cnt), C.byref(usec))
                bat_t.append(time.perf_counter() - t0)
                assert p and cnt.value == n, L.bnn_mi355x_last_error()
                bat_res = np.ctypeslib.as_array(p, shape=(R * n,)).copy().reshape(R, n)
                L.free_results(p)
                dev_us.append(usec.value * R * n)
            assert (seq_res == bat_res).all(), "batched and sequential results differ"
            s, b = np.median(seq_t) * 1e3, np.median(bat_t) * 1e3
            print("%s %3d flips: sequential %8.1f ms  batched %7.1f ms (device %6.1f ms)  x%.1f" % (net, flips, s, b, np.median(dev_us) / 1e3, s / b))
            sys.stdout.flush()
