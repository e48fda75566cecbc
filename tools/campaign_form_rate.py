#!/usr/bin/env python3
"""The two forms of the campaign launches (bnn_mi355x_campaign_form): 0, layers 1-7 on the integer pipe, and 1, on the
matrix cores from every run's own operand tables (csrc/multi_mfma_kernels.hip).  RUNS runs x IMAGES seeded random images
(defaults 100 x 1 000) per call, per CNV network:
  mem_noise_campaigns at rate 0 (every run on the loaded tables) and 2^-6 (every run on its own);
  fault_campaigns with 1 and 10 flips (the tables remade behind every wave of patches);
  act_noise_campaigns at 2^-6 (a launch per layer, the loaded tables);
  exposure_campaigns with 1, 10 and 100 epochs at 2^-9 per epoch (the tables remade behind every epoch; segments of
  IMAGES / epochs images: where the form is expected to lose).
The forms alternate in one process, the order swapping every round; each call reports the device time the entry point
returns (usecPerImage x runs x images: everything the call enqueues between its two events -- copies, upsets, table
launches, stages) and the wall time; medians and ranges of ROUNDS rounds after one untimed call each, classes and counters
asserted equal in every round.  Form 0 is the yardstick.  The record is profiles/r39_campaign_form_rate.txt.
usage: campaign_form_rate.py [rounds [runs [images]]]"""
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
from bnn import abi, params_io  # noqa: E402

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
RUNS = int(sys.argv[2]) if len(sys.argv) > 2 else 100
IMAGES = int(sys.argv[3]) if len(sys.argv) > 3 else 1000
NETS = ("cnvW1A1", "cnvW1A2", "cnvW2A2")


def q32(p):
    return int(np.floor(p * 4294967296.0))


def result(L, p, cnt, counts, k):
    assert p, L.bnn_mi355x_last_error().decode()
    got = np.ctypeslib.as_array(p, shape=(RUNS * cnt.value,)).copy()
    L.free_results(p)
    c = (C.c_long * max(k, 1))()
    if counts is not None:
        assert counts(c, k) == k
    return got, np.array(c[:k], np.int64)


def cases(L, network, path):
    """-> [(name, call)]; call() -> (classes, counters, device ms)"""
    lay = params_io.layout(network)
    S = len(lay)
    up = C.c_uint * S

    def rates(p):
        return up(*([q32(p)] * S)), up(*[q32(p) if F["nthr"] else 0 for F in lay])

    def timed(fn):
        def call():
            cnt, usec = C.c_int(0), C.c_float(0)
            got, counts = fn(cnt, usec)
            return got, counts, usec.value * RUNS * cnt.value / 1e3
        return call

    def mem(p):
        rw, rt = rates(p)
        return timed(lambda cnt, usec: result(L, L.bnn_mi355x_mem_noise_campaigns(path, 10, RUNS, 11, rw, rt, S, C.byref(cnt), C.byref(usec)), cnt,
                                              L.bnn_mi355x_last_mem_noise_counts, RUNS * S * 2))

    def fault(flips):
        return timed(lambda cnt, usec: result(L, L.bnn_mi355x_fault_campaigns(path, 10, RUNS, 22, flips, 1, -1, None, 0, C.byref(cnt), C.byref(usec)),
                                              cnt, None, 0))

    def act(p):
        rq = (C.c_uint * (S - 1))(*([q32(p)] * (S - 1)))
        return timed(lambda cnt, usec: result(L, L.bnn_mi355x_act_noise_campaigns(path, 10, RUNS, 33, rq, S - 1, C.byref(cnt), C.byref(usec)), cnt,
                                              L.bnn_mi355x_last_act_noise_counts, RUNS * (S - 1)))

    def exposure(epochs):
        rw, rt = rates(2.0 ** -9)
        ei = -(-IMAGES // epochs)
        return timed(lambda cnt, usec: result(L, L.bnn_mi355x_exposure_campaigns(path, 10, 0, 1, RUNS, 44, rw, rt, S, ei, 0, C.byref(cnt), C.byref(usec)),
                                              cnt, L.bnn_mi355x_last_exposure_counts, RUNS * -(-IMAGES // ei) * S * 4))

    return [("mem_noise rate 0", mem(0.0)), ("mem_noise rate 2^-6", mem(2.0 ** -6)), ("fault 1 flip", fault(1)), ("fault 10 flips", fault(10)),
            ("act_noise 2^-6", act(2.0 ** -6)), ("exposure 1 epoch", exposure(1)), ("exposure 10 epochs", exposure(10)),
            ("exposure 100 epochs", exposure(100))]


def spread(v):
    return "median %9.3f  range %9.3f .. %9.3f  (%s)" % (statistics.median(v), min(v), max(v), " ".join("%.3f" % x for x in v))


print("%d runs x %d seeded random images a call; ms per call, %d rounds of the two forms in one process after one untimed call each; "
      "classes and counters equal in every call" % (RUNS, IMAGES, rounds))
with tempfile.TemporaryDirectory() as tmp:
    imgs = np.random.default_rng(2026).integers(0, 256, (IMAGES, 3072), dtype=np.uint8)
    path = os.path.join(tmp, "imgs.bin")
    np.concatenate([np.ones((IMAGES, 1), np.uint8), imgs], axis=1).tofile(path)
    for network in NETS:
        L = abi.load(network)
        L.load_parameters(os.path.join(abi.PARAM_ROOT, "cifar10", network).encode())
        assert L.bnn_mi355x_last_error() == b"", L.bnn_mi355x_last_error()
        was = L.bnn_mi355x_campaign_form(7)
        for name, call in cases(L, network, path.encode()):
            def route(form):
                L.bnn_mi355x_campaign_form(form)
                assert L.bnn_mi355x_campaign_matrix_stages(RUNS) == (0xFE if form else 0)
                t0 = time.perf_counter()
                got, counts, dev = call()
                return got, counts, 1e3 * (time.perf_counter() - t0), dev
            ref = route(0)  # once each, untimed
            one = route(1)
            assert (one[0] == ref[0]).all() and (one[1] == ref[1]).all(), name
            wall, dev = {0: [], 1: []}, {0: [], 1: []}
            for r in range(rounds):
                for form in ((0, 1), (1, 0))[r % 2]:
                    got, counts, w, d = route(form)
                    assert (got == ref[0]).all() and (counts == ref[1]).all(), (name, form)
                    wall[form].append(w); dev[form].append(d)
            print("%s %s" % (network, name))
            for form, label in ((0, "form 0, integer pipe:"), (1, "form 1, matrix cores:")):
                print("  %-22s device %s" % (label, spread(dev[form])))
                print("  %-22s wall   %s" % ("", spread(wall[form])))
            for what, v in (("device", dev), ("wall", wall)):
                print("  %s, medians: form 1 x%.3f of form 0; form 0's own spread x%.3f (max / min of its %d repeats)"
                      % (what, statistics.median(v[1]) / statistics.median(v[0]), max(v[0]) / min(v[0]), rounds))
            sys.stdout.flush()
        L.bnn_mi355x_campaign_form(was)
