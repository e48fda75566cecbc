#!/usr/bin/env python3
"""The two forms of the single-fault sweeps (bnn_mi355x_campaign_form): 0, every stage on the integer pipe by segment
record, and 1, every stage of layers 1-7 that reads the loaded parameters on the matrix cores from the list of its alive
slots (csrc/list_mfma_kernels.hip).  IMAGES seeded random images (default 1 000) per call, for cnvW1A1 and cnvW2A2:
  act_fault_sweep on ALL sites of layer 0, of layer 1, of layer 3 and of layer 6 (one call each);
  fault_sweep on a whole layer 1 (every weight bit and every threshold bit, word size 1).
The forms alternate in one process, the order swapping every round; each call reports the device time the entry point
returns (usecPerImage x faults x images: the bursts of device work between the call's host waits -- broadcasts, seeds,
stages, marking, counting) and the wall time, which adds the host's share (cutting the survivors into records, and under
form 1 listing them); medians and ranges of ROUNDS rounds after one untimed call each, `changed` and the pairs per stage
asserted equal in every call.  Form 0 is the yardstick.  The record is profiles/r40_sweep_form_rate.txt.
usage: sweep_form_rate.py [rounds [images [network ...]]]"""
import ctypes as C
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch  # noqa: F401  (HIP runtime order)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bnn-pynq_amd"))
from bnn import abi  # noqa: E402

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
IMAGES = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
NETS = tuple(sys.argv[3:]) or ("cnvW1A1", "cnvW2A2")
ip = C.POINTER(C.c_int)


def act_sites(L, layer):
    k = L.bnn_mi355x_enumerate_act_faults(layer, 0, None, 0)
    assert k > 0, L.bnn_mi355x_last_error()
    rec = np.zeros((k, 5), np.int32)
    L.bnn_mi355x_enumerate_act_faults(layer, 0, rec.ctypes.data_as(ip), k)
    return rec


def layer_faults(L, layer):
    out = []
    for target in (0, 1):
        k = L.bnn_mi355x_enumerate_faults(layer, target, 1, 0, None, 0)
        rec = np.zeros((max(k, 1), 8), np.int32)
        L.bnn_mi355x_enumerate_faults(layer, target, 1, 0, rec.ctypes.data_as(ip), k)
        out.append(rec[:k])
    return np.concatenate(out)


def sweep_call(L, entry, stages, path, recs):
    """-> call() -> (changed, pairs per stage, device ms); no diffs kept (cap 0)"""
    changed, diffs = np.zeros(len(recs), np.int32), np.zeros((1, 3), np.int32)

    def call():
        cnt, usec = C.c_int(0), C.c_float(0)
        total = entry(path, 10, recs.ctypes.data_as(ip), len(recs), changed.ctypes.data_as(ip), diffs.ctypes.data_as(ip), 0, C.byref(cnt),
                      C.byref(usec))
        assert total >= 0 and cnt.value == IMAGES, L.bnn_mi355x_last_error().decode()
        s = stages(None, 0)
        pairs = (C.c_long * s)()
        assert stages(pairs, s) == s
        return changed.copy(), list(pairs), usec.value * len(recs) * cnt.value / 1e3
    return call


def spread(v):
    return "median %10.3f  range %10.3f .. %10.3f  (%s)" % (statistics.median(v), min(v), max(v), " ".join("%.3f" % x for x in v))


print("%d seeded random images a call; ms per call, %d rounds of the two forms in one process after one untimed call each; "
      "changed and pairs per stage equal in every call" % (IMAGES, rounds))
with tempfile.TemporaryDirectory() as tmp:
    imgs = np.random.default_rng(2026).integers(0, 256, (IMAGES, 3072), dtype=np.uint8)
    path = os.path.join(tmp, "imgs.bin")
    np.concatenate([np.ones((IMAGES, 1), np.uint8), imgs], axis=1).tofile(path)
    for network in NETS:
        L = abi.load(network)
        L.load_parameters(os.path.join(abi.PARAM_ROOT, "cifar10", network).encode())
        assert L.bnn_mi355x_last_error() == b"", L.bnn_mi355x_last_error()
        was = L.bnn_mi355x_campaign_form(7)
        cases = [("act_fault_sweep, all sites of layer %d" % l, L.bnn_mi355x_act_fault_sweep, L.bnn_mi355x_last_act_sweep_stages,
                  act_sites(L, l)) for l in (0, 1, 3, 6)]
        cases.append(("fault_sweep, all of layer 1", L.bnn_mi355x_fault_sweep, L.bnn_mi355x_last_sweep_stages, layer_faults(L, 1)))
        for name, entry, stages, recs in cases:
            call = sweep_call(L, entry, stages, path.encode(), np.ascontiguousarray(recs))

            def route(form):
                L.bnn_mi355x_campaign_form(form)
                t0 = time.perf_counter()
                changed, pairs, dev = call()
                return changed, pairs, 1e3 * (time.perf_counter() - t0), dev
            ref = route(0)  # once each, untimed
            one = route(1)
            assert (one[0] == ref[0]).all() and one[1] == ref[1], name
            wall, dev = {0: [], 1: []}, {0: [], 1: []}
            for r in range(rounds):
                for form in ((0, 1), (1, 0))[r % 2]:
                    changed, pairs, w, d = route(form)
                    assert (changed == ref[0]).all() and pairs == ref[1], (name, form)
                    wall[form].append(w); dev[form].append(d)
                print("  ... %s %s: round %d of %d" % (network, name, r + 1, rounds), file=sys.stderr, flush=True)
            print("%s %s: %d faults, %d changed classes, pairs per stage %s" % (network, name, len(recs), int(ref[0].sum()), ref[1]))
            for form, label in ((0, "form 0, integer pipe:"), (1, "form 1, matrix cores:")):
                print("  %-22s device %s" % (label, spread(dev[form])))
                print("  %-22s wall   %s" % ("", spread(wall[form])))
            for what, v in (("device", dev), ("wall", wall)):
                print("  %s, medians: form 1 x%.3f of form 0; form 0's own spread x%.3f (max / min of its %d repeats)"
                      % (what, statistics.median(v[1]) / statistics.median(v[0]), max(v[0]) / min(v[0]), rounds))
            sys.stdout.flush()
        L.bnn_mi355x_campaign_form(was)
