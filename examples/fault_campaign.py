#!/usr/bin/env python3
"""A fault-injection campaign with the reference's `bnn.faults` drivers (the flow of the fork's fault
notebooks) on an MI355X: 2 000 synthetic CIFAR-10-shaped images whose "labels" are the fault-free
classes (control accuracy 100 %), three runs for each of {50, 500} upsets x {weight bit, threshold word}, then the
datapath's accuracy-versus-upset-rate curve: every activation upset with probability 2^-14 ... 2^-6, ten runs each; the
same curve for the parameter memories (every weight / threshold bit upset with that probability, per memory kind);
what TMR and threshold interleaving buy at the three highest rates, for single bits and bursts of four; and
the same two questions of the image buffer: the curve for input-bit upsets, and which bit positions of a pixel matter
(every bit of the image flipped alone, on the first 200 images).

    python examples/fault_campaign.py [output_dir]
"""
import json
import os
import sys
import tempfile

import numpy as np
import torch  # noqa: F401  first: one HIP runtime per process

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bnn-pynq_amd"))
import bnn  # noqa: E402

out = sys.argv[1] if len(sys.argv) > 1 else tempfile.mkdtemp(prefix="bnn_faults_")
rng = np.random.default_rng(0)
rec = rng.integers(0, 256, (2000, 3073), dtype=np.uint8)
path = os.path.join(out, "set.bin")
os.makedirs(out, exist_ok=True)
rec.tofile(path)
labels = bnn.CnvClassifier(bnn.NETWORK_CNVW1A1, "cifar10").classify_cifars(path).tolist()

test = bnn.faults.CNVFaultTest.CIFARTest(bnn.NETWORK_CNVW1A1, path, labels)
T = bnn.faults.NetworkTest.TestType
bnn.faults.NetworkTest(test).test_network(out, 3, [50, 500], [T.weight_bit(), T.threshold_word()])
for flips in (50, 500):
    stats = json.load(open(os.path.join(out, "cnvW1A1", "cifar10", "%dflips" % flips, "cnvW1A1_cifar10_stats.json")))
    for name, e in stats["results"].items():
        print("%4d x %-14s accuracy min %.2f avg %.2f max %.2f (%d of 3 runs changed something)"
              % (flips, name, e["min accuracy"], e["avg accuracy"], e["max accuracy"], e["effective count"]))

net = bnn.faults.NetworkTest(test)
rates = [2.0 ** -e for e in (14, 12, 10, 8, 6)]
net.upset_rate_curve(out, 10, rates, seed=1)
for p in rates:
    stats = json.load(open(os.path.join(out, "cnvW1A1", "cifar10", "upsets", "cnvW1A1_cifar10_rate%g_stats.json" % p)))
    e = stats["results"]["upset rate %g" % p]
    print("upset rate %-12g (effective %.3g) accuracy min %.2f avg %.2f max %.2f stddev %.2f"
          % (p, e["effective rate"], e["min accuracy"], e["avg accuracy"], e["max accuracy"], e["stddev accuracy"]))

# the parameter memories: every bit of the weight (then: threshold) memories upset with probability p, in place from image 0
net.memory_upset_rate_curve(out, 10, rates, seed=1)
for target in ("weights", "thresholds"):
    stats = json.load(open(os.path.join(out, "cnvW1A1", "cifar10", "memory-upsets", "cnvW1A1_cifar10_%s_stats.json" % target)))
    for p in rates:
        e = stats["results"]["%s upset rate %g" % (target, p)]
        print("%-10s upset rate %-12g (effective %.3g) accuracy min %.2f avg %.2f max %.2f stddev %.2f"
              % (target, p, e["effective rate"], e["min accuracy"], e["avg accuracy"], e["max accuracy"], e["stddev accuracy"]))

# what hardening buys: the same upsets on the PHYSICAL memories of the fork's hardened overlays (three voted modules under
# TMR, bit-interleaved threshold lines), single bits and bursts of four, the same seeds for every scheme
schemes = [0, 1, 2, 3]
net.hardening_curve(out, 10, rates[-3:], schemes, bursts=(1, 4), seed=1)
stats = json.load(open(os.path.join(out, "cnvW1A1", "cifar10", "hardening", "cnvW1A1_cifar10_hardening_stats.json")))
for scheme in schemes:
    for burst in (1, 4):
        for p in rates[-3:]:
            e = stats["results"]["%s burst %d upset rate %g" % (bnn.faults.HARDENING_SCHEMES[scheme], burst, p)]
            print("%-22s burst %d upset rate %-10g accuracy min %.2f avg %.2f max %.2f  (%d physical bits, %d logical)"
                  % (bnn.faults.HARDENING_SCHEMES[scheme], burst, p, e["min accuracy"], e["avg accuracy"], e["max accuracy"],
                     e["physical bits"], e["logical bits"]))

# how often the memories must be rewritten: the same upsets ACCUMULATE over 8 epochs of 250 images at a rate per epoch,
# never scrubbed, scrubbed every other epoch and every epoch; unhardened and TMR
net.scrubbing_curve(out, 10, [2.0 ** -10], [0, 2, 1], [0, 1], 250, seed=1)
stats = json.load(open(os.path.join(out, "cnvW1A1", "cifar10", "scrubbing", "cnvW1A1_cifar10_scrubbing_stats.json")))
for scheme in (0, 1):
    for every in (0, 2, 1):
        e = stats["results"]["%s burst 1 upset rate %g scrub every %d" % (bnn.faults.HARDENING_SCHEMES[scheme], 2.0 ** -10, every)]
        print("%-6s scrub every %d: mean accuracy per epoch %s" % (bnn.faults.HARDENING_SCHEMES[scheme], every,
                                                                  np.round(e["mean accuracy per epoch"], 2).tolist()))
net.scrubbing_curve(os.path.join(out, "ecc"), 10, [2.0 ** -10], [0, 1], [(0, 1), (2, 1)], 250, bursts=(1, 2), seed=1)  # (scheme, code): SEC-DED coded thresholds

# the scrub such memories really have: a REPAIR reads a word, votes or decodes it and writes it back -- it fixes only what the
# redundancy covers and locks in what it gets wrong.  (scrub_every, repair_every): rewrite every epoch / repair every epoch /
# repair every epoch + rewrite every 10 / never; 20 epochs of 100 images, TMR and interleaved + SEC-DED
intervals = [(1, 0), (0, 1), (10, 1), (0, 0)]
net.scrubbing_curve(os.path.join(out, "repair"), 10, [2.0 ** -10], intervals, [1, (2, 1)], 100, seed=1)
stats = json.load(open(os.path.join(out, "repair", "cnvW1A1", "cifar10", "scrubbing", "cnvW1A1_cifar10_scrubbing_stats.json")))
for name in ("TMR", "interleaved + SEC-DED"):
    for every, repair in intervals:
        e = stats["results"]["%s burst 1 upset rate %g scrub every %d" % (name, 2.0 ** -10, every) + (" repair every %d" % repair if repair else "")]
        print("%-21s rewrite every %2d repair every %d: avg accuracy %.2f, last epoch %.2f, words repaired %d"
              % (name, every, repair, e["avg accuracy"], e["mean accuracy per epoch"][-1], sum(e.get("repaired words per epoch", [0]))))

# the last unprotected memories: SEC-DED (72,64) over the weights of the layers >= 1, a (scheme, code, weight_code) triple.  TMR
# plus coded weights is the first organisation in which every memory has redundancy; the same four schedules
net.scrubbing_curve(os.path.join(out, "wecc"), 10, [2.0 ** -10], intervals, [(1, 0, 1), (0, 1, 1)], 100, seed=1)
stats = json.load(open(os.path.join(out, "wecc", "cnvW1A1", "cifar10", "scrubbing", "cnvW1A1_cifar10_scrubbing_stats.json")))
for name in ("TMR + SEC-DED weights", "none + SEC-DED + SEC-DED weights"):
    for every, repair in intervals:
        e = stats["results"]["%s burst 1 upset rate %g scrub every %d" % (name, 2.0 ** -10, every) + (" repair every %d" % repair if repair else "")]
        print("%-32s rewrite every %2d repair every %d: avg accuracy %.2f, last epoch %.2f, weight code words repaired %d"
              % (name, every, repair, e["avg accuracy"], e["mean accuracy per epoch"][-1], sum(e["repaired weight words per epoch"])))

# bursts: with the coded weights alone an aligned burst of 2 is a double error of one code word and nothing is corrected;
# column-interleaved (a (scheme, code, weight_code, weight_interleave) 4-tuple) its two bits lie in two code words, both corrected
net.scrubbing_curve(os.path.join(out, "iwecc"), 10, [2.0 ** -10], [(0, 1)], [(1, 0, 1), (1, 0, 1, 1)], 100, bursts=(2,), seed=1)
stats = json.load(open(os.path.join(out, "iwecc", "cnvW1A1", "cifar10", "scrubbing", "cnvW1A1_cifar10_scrubbing_stats.json")))
for name in ("TMR + SEC-DED weights", "TMR + SEC-DED weights column-interleaved"):
    e = stats["results"]["%s burst 2 upset rate %g scrub every 0 repair every 1" % (name, 2.0 ** -10)]
    print("%-42s burst 2, repair every epoch: avg accuracy %.2f, last epoch %.2f, weight code words corrected %d, detected %d"
          % (name, e["avg accuracy"], e["mean accuracy per epoch"][-1], sum(e["corrected weight words per epoch"]),
             sum(e["detected weight words per epoch"])))

# the image buffer: upset-rate curve, then the per-bit sensitivity map (24 576 sites x 200 images)
net.input_upset_rate_curve(out, 10, rates, seed=1)
for p in rates:
    stats = json.load(open(os.path.join(out, "cnvW1A1", "cifar10", "input-upsets", "cnvW1A1_cifar10_rate%g_stats.json" % p)))
    e = stats["results"]["input upset rate %g" % p]
    print("input upset rate %-6g (effective %.3g) accuracy min %.2f avg %.2f max %.2f stddev %.2f"
          % (p, e["effective rate"], e["min accuracy"], e["avg accuracy"], e["max accuracy"], e["stddev accuracy"]))
small = os.path.join(out, "set200.bin")
rec[:200].tofile(small)
cm = bnn.faults.NetworkTest(bnn.faults.CNVFaultTest.CIFARTest(bnn.NETWORK_CNVW1A1, small, labels[:200])).input_sensitivity_map(out)
print("images (of 200) whose class one flipped input bit changes, mean per bit position 0..7:",
      np.round(cm.reshape(-1, 8).mean(axis=0), 3).tolist())

# where faults are masked: the propagation of every activation site of layers 0 and 4, and of every input bit, on the 200 images
small_net = bnn.faults.NetworkTest(bnn.faults.CNVFaultTest.CIFARTest(bnn.NETWORK_CNVW1A1, small, labels[:200]))
for layer, doc in list(small_net.propagation_map(out, "activation", [0, 4]).items()) + list(small_net.propagation_map(out, "input").items()):
    print("sites of %s: share of (fault, image) pairs still alive after layers %s: %s; activations wrong per live image: %s"
          % ("layer %d" % layer if layer != "input" else "the image", doc["downstream layers"],
             np.round(doc["share alive"], 4).tolist(), np.round(doc["mean error size"], 1).tolist()))
print("results under", out)
