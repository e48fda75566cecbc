"""Hardened memory schemes in the memory upset campaigns on the GPU (bnn_mi355x_hardened_mem_noise_campaigns): upsets of
the PHYSICAL parameter memories -- three modules under TMR, bit-interleaved threshold lines -- in bursts of b bits, seen
through the voter and the de-interleaver.  All checks are exact.

The model is pinned on the host by tests/test_hardened_mem_noise.py: bnn_mi355x_hardened_mem_noise_mask lists a run's
events, bnn_mi355x_pack_params_hardened applies such records (checked there against a route of its own).  Here the
device's work is compared with it byte for byte -- bnn_mi355x_hardened_mem_noise_params reads back the very blob a run
classifies with -- and the classes with import_params(that blob) + inference_buffer in a second library handle.

3 runs x 48 images, rates 2^-3 and 2^-8.  At 2^-3 the inputs exercise the voter and the partner-line path BY
CONSTRUCTION: the tests first assert, from the plain-Python restatement of the draw, that every replicated memory has a
bit hit in exactly one module and one hit in two or more, and that every interleaved layer has an event that reaches
both lines' elements."""
import ctypes as C
import struct

import numpy as np
import pytest

import gpu_lib as gl
import hardened_ref as hr
import test_gpu_act_fault_sweep as sw
import test_gpu_mem_noise as gm
import test_mem_noise_mask as mm

pytestmark = pytest.mark.gpu
q32 = hr.q32
RUNS, N, SEED = 3, 48, 20261018
PAIRS = [(n, s) for n in ("cnvW1A1", "cnvW1A2", "cnvW2A2") for s in hr.SUPPORTED[n]]
RATES = (2.0 ** -3, 2.0 ** -8)


def hcampaign(L, path, scheme, burst, runs, seed, rw, rt, ncls=10):
    """-> (classes [runs, n], counts [runs, layers, 2: weights, thresholds, 2: physical, logical], seeds [runs])"""
    up = C.c_uint * len(rw)
    cnt, usec = C.c_int(0), C.c_float(0)
    p = L.bnn_mi355x_hardened_mem_noise_campaigns(path.encode(), ncls, scheme, burst, runs, seed, up(*rw), up(*rt), len(rw), C.byref(cnt),
                                                  C.byref(usec))
    assert p, L.bnn_mi355x_last_error().decode()
    n = cnt.value
    got = np.ctypeslib.as_array(p, shape=(max(runs * n, 1),))[: runs * n].copy().reshape(runs, n)
    L.free_results(p)
    k = L.bnn_mi355x_last_hardened_mem_noise_counts(None, 0)
    assert k == runs * len(rw) * 4
    c = (C.c_long * k)()
    assert L.bnn_mi355x_last_hardened_mem_noise_counts(c, k) == k
    s = (C.c_ulonglong * runs)()
    assert L.bnn_mi355x_last_hardened_mem_noise_seeds(s, runs) == runs
    return got, np.array(c[:], np.int64).reshape(runs, len(rw), 2, 2), list(s)


def hdevice_blob(L, scheme, burst, seed, rw, rt):
    up = C.c_uint * len(rw)
    size = L.bnn_mi355x_hardened_mem_noise_params(scheme, burst, seed, up(*rw), up(*rt), len(rw), None, 0)
    assert size > 0, L.bnn_mi355x_last_error().decode()
    blob = np.zeros(size, np.uint8)
    assert L.bnn_mi355x_hardened_mem_noise_params(scheme, burst, seed, up(*rw), up(*rt), len(rw), blob.ctypes.data, size) == size
    return blob


def module_bits(network, recs, layer, target):
    """-> one set per module of the physical bits (mem, ind, thresh, bit) the records flip in that (small) memory"""
    eb = hr.ebits(network, layer, target)
    out = [set(), set(), set()]
    for _, t, l, mem, ind, thresh, bit, ws, module in recs[(recs[:, 2] == layer) & (recs[:, 1] == target)].tolist():
        out[module].update((mem, ind, thresh, b) for b in range(bit, min(bit + ws, eb)))
    return out


def assert_preconditions(network, scheme, burst, recs):
    """at 2^-3, from the restatement's events alone"""
    lay = hr.params_io.layout(network)
    for layer in range(len(lay)):
        for target in (0, 1):
            if hr.org(network, scheme, layer)[target] == 3:
                a, b, c = module_bits(network, recs, layer, target)
                twice = (a & b) | (a & c) | (b & c)
                assert len((a | b | c) - twice) >= 1 and len(twice) >= 1, (layer, target)
        il = hr.org(network, scheme, layer)[2]
        if il:
            T, F = hr.ebits(network, layer, 1), lay[layer]
            tab = hr.pair_table(il, T)
            reach = False
            for _, t, l, mem, ind, thresh, bit, ws, module in recs.tolist():
                if (l, t) != (layer, 1):
                    continue
                q0 = bit + (T if ind % 2 == 0 else 0)
                lines = {tab[q][0] for q in range(q0, min(q0 + ws, (q0 // T + 1) * T))}
                # burst 1: a physical bit of one line that belongs to the other line's element
                reach = reach or (lines == {0, 1} if burst > 1 else lines == {1 - ind % 2})
            assert reach, layer


def implied_counts(network, scheme, pdir, recs):
    """[layer][target][physical, logical] from the events: physical, the bits flipped (a burst clipped to its element);
    logical: one module and no interleave, the same; interleave alone permutes bits, the same; three modules, the bits
    hit in two or more.  Layer 0 (24-bit thresholds read back as their integer part) through hardened_ref's own route."""
    lay = hr.params_io.layout(network)
    out = np.zeros((len(lay), 2, 2), np.int64)
    for layer in range(1, len(lay)):
        for target in (0, 1):
            mine = recs[(recs[:, 2] == layer) & (recs[:, 1] == target)]
            width = np.minimum(mine[:, 7], hr.ebits(network, layer, target) - mine[:, 6])
            out[layer, target] = width.sum()  # (events of one module never overlap: distinct aligned groups)
            if hr.org(network, scheme, layer)[target] == 3:
                a, b, c = module_bits(network, mine, layer, target)
                assert len(a) + len(b) + len(c) == out[layer, target, 0]
                out[layer, target, 1] = len((a & b) | (a & c) | (b & c))
    _, _, physical, logical = hr.logical_after(network, scheme, pdir, recs[recs[:, 2] == 0], only=(0,))
    out[0, :, 0], out[0, :, 1] = physical[0], logical[0]
    return out


def weight_bits_differing(network, blob, clean, layer):
    """1-bit weights: the differing bits of the layer's rows behind the two threshold dwords"""
    off, rd, rows, kw = struct.unpack_from("<4I", clean, 32 + 16 * layer)
    a = blob[off: off + rows * rd * 4].reshape(rows, rd * 4)[:, 8: 8 + 8 * kw]
    b = clean[off: off + rows * rd * 4].reshape(rows, rd * 4)[:, 8: 8 + 8 * kw]
    return int(np.unpackbits(a ^ b).sum())


def rates_of(network, p):
    return gm.rates(network, p, p)


@pytest.mark.parametrize("network,dataset", mm.NETS, ids=lambda x: x)
def test_scheme_0_burst_1_is_mem_noise_campaigns(network, dataset, tmp_path, monkeypatch):
    """the exposure path at epoch 0 (k_xmem_noise_w / _t, which the hardened entry point runs) against the plain route's own
    kernels, all five nets, both rates: classes, blob and counts are equal (the logical count equals the physical one
    wherever a bit is a bit: every memory but layer 0's thresholds of a CNV net)"""
    L, pdir = gm.load(network, dataset)
    path = sw.write_images(network, sw.images(network, N, seed=17), tmp_path)
    monkeypatch.setenv("BNN_MI355X_NOISE_GROUP", "37")
    for p in RATES:
        rw, rt = rates_of(network, p)
        want, wcounts, wseeds = gm.campaign(L, path, RUNS, SEED, rw, rt)
        got, counts, seeds = hcampaign(L, path, 0, 1, RUNS, SEED, rw, rt)
        assert seeds == wseeds and got.tolist() == want.tolist()
        assert counts[:, :, :, 0].tolist() == wcounts.tolist() and wcounts[:, :, 0].sum() > 0
        same = np.ones(counts.shape[1:3], bool)
        same[0, 1] = not network.startswith("cnv")
        assert (counts[:, :, :, 1] == counts[:, :, :, 0])[:, same].all()
        for r in range(RUNS):
            gm.assert_same_bytes(hdevice_blob(L, 0, 1, SEED + r, rw, rt), gm.device_blob(L, SEED + r, rw, rt), "%s run %d rate %g" % (network, r, p))
    assert (got != gm.clean_classes(L, path)[None]).any()


@pytest.mark.parametrize("network,scheme", PAIRS, ids=str)
def test_every_supported_scheme(network, scheme, tmp_path, monkeypatch):
    """bursts 1 and 4, rates 2^-3 and 2^-8 on every memory: the blob each run classifies with is pack_params_hardened of
    its concatenated masks, byte for byte; the classes are those of that blob imported into a second library handle; both
    counts are what the masks imply; another grouping of the pairs changes nothing"""
    L, pdir = gm.load(network, "cifar10")
    L2 = gl.load(network, "python_hw")  # a second handle: importing a blob drops the raw memories the campaign draws in
    imgs = sw.images(network, N, seed=23)
    path = sw.write_images(network, imgs, tmp_path)
    clean = gl.pack_params(network, pdir)
    clean_cls = gm.clean_classes(L, path)
    crc = L.bnn_mi355x_params_crc()
    changed = 0
    for burst in (1, 4):
        for p in RATES:
            rw, rt = rates_of(network, p)
            what = "%s scheme %d burst %d rate %g" % (network, scheme, burst, p)
            blobs, want_counts = [], []
            for r in range(RUNS):
                recs = hr.lib_run_events(L, network, scheme, burst, SEED + r, rw, rt)
                if p == RATES[0]:
                    small = recs[(recs[:, 2] <= 4) | (recs[:, 1] == 1)]  # (the replicated and the interleaved memories)
                    ref_small = np.concatenate([hr.events(network, burst, SEED + r, l, t, m, (rw, rt)[t][l]) for l in range(9) for t in (0, 1)
                                                for m in range(hr.org(network, scheme, l)[t]) if l <= 4 or t == 1])
                    assert (small == ref_small).all()
                    assert_preconditions(network, scheme, burst, ref_small[(ref_small[:, 2] == 0) | (ref_small[:, 1] == 1)])
                blob = hr.pack_hardened(L, pdir, scheme, recs)
                gm.assert_same_bytes(hdevice_blob(L, scheme, burst, SEED + r, rw, rt), blob, what + " run %d" % r)
                blobs.append(blob)
                want_counts.append(implied_counts(network, scheme, pdir, recs))
                if "W1" in network:
                    for layer in (1, 5, 8):
                        assert weight_bits_differing(network, blob, clean, layer) == want_counts[-1][layer, 0, 1] > 0
            monkeypatch.setenv("BNN_MI355X_NOISE_GROUP", "37")
            got, counts, seeds = hcampaign(L, path, scheme, burst, RUNS, SEED, rw, rt)
            assert seeds == [SEED + r for r in range(RUNS)]
            assert counts.tolist() == np.array(want_counts).tolist(), what
            monkeypatch.setenv("BNN_MI355X_NOISE_GROUP", "1000")
            g2, c2, _ = hcampaign(L, path, scheme, burst, RUNS, SEED, rw, rt)
            assert g2.tolist() == got.tolist() and c2.tolist() == counts.tolist(), what
            for r in range(RUNS):
                want = gm.classify_with_blob(L2, blobs[r], imgs)
                assert got[r].tolist() == want.tolist(), what + " run %d" % r
                changed += int((want != clean_cls).sum())
            if scheme == 1:  # the voter at work: far fewer logical than physical bits in the replicated thresholds
                assert 0 < counts[:, 1:5, 1, 1].sum() < counts[:, 1:5, 1, 0].sum() / 3 or p == RATES[1]
    assert changed > 0 and L.bnn_mi355x_params_crc() == crc
    assert gm.clean_classes(L, path).tolist() == clean_cls.tolist()


def test_rate_0_and_refusals_on_loaded_parameters(tmp_path):
    """all rates 0: the fault-free classes once per run, all counts 0, the parameters read back are the loaded ones (no
    copy is made and no upset kernel launched: the runs read the loaded blob).  An imported blob has no raw memories to
    draw in: refused like mem_noise_campaigns refuses it."""
    network = "cnvW1A2"
    L, pdir = gm.load(network, "cifar10")
    path = sw.write_images(network, sw.images(network, N, seed=4), tmp_path)
    clean = gm.clean_classes(L, path)
    z = [0] * 9
    for scheme, burst in ((1, 1), (3, 4), (0, 16)):
        got, counts, _ = hcampaign(L, path, scheme, burst, RUNS, 5, z, z)
        assert (got == clean[None]).all() and (counts == 0).all()
        assert (hdevice_blob(L, scheme, burst, 5, z, z) == gl.pack_params(network, pdir)).all()
    blob = gl.pack_params(network, pdir)
    assert L.bnn_mi355x_import_params(blob.ctypes.data, len(blob)) == 0
    up = C.c_uint * 9
    w = [1 << 24] * 9
    assert not L.bnn_mi355x_hardened_mem_noise_campaigns(path.encode(), 10, 1, 1, 1, 1, up(*w), up(*z), 9, None, None)
    assert b"imported blob" in L.bnn_mi355x_last_error()
    assert L.bnn_mi355x_hardened_mem_noise_params(1, 1, 1, up(*w), up(*z), 9, None, 0) == 0
    assert b"imported blob" in L.bnn_mi355x_last_error()
    L.load_parameters(pdir.encode())


def test_variant_library_runs_the_same_campaign(variant_libs, tmp_path):
    """cnvW1A1-TMR's library: the entry points it shares with the base network still refuse; the hardened campaign gives the
    classes and counts of the base network's library for the scheme its name implies"""
    network = "cnvW1A1"
    L, pdir = gm.load(network, "cifar10")
    V = gl.load("cnvW1A1-TMR")
    V.load_parameters(pdir.encode())
    assert V.bnn_mi355x_last_error() == b""
    path = sw.write_images(network, sw.images(network, N, seed=6), tmp_path)
    rw, rt = rates_of(network, 2.0 ** -3)
    up = C.c_uint * 9
    assert not V.bnn_mi355x_mem_noise_campaigns(path.encode(), 10, 1, 1, up(*rw), up(*rt), 9, None, None)
    assert b"not modelled" in V.bnn_mi355x_last_error()
    scheme = V.bnn_mi355x_hardening_scheme()
    assert scheme == 1
    a = hcampaign(V, path, scheme, 4, RUNS, 9, rw, rt)
    b = hcampaign(L, path, scheme, 4, RUNS, 9, rw, rt)
    assert a[0].tolist() == b[0].tolist() and a[1].tolist() == b[1].tolist()


def test_python_interface(tmp_path):
    """FaultTest.run_memory_noise_test(scheme=, burst=) and NetworkTest.hardening_curve on 40 images: the accuracies follow
    from the C call's classes, the counts are the C call's; the curve has one entry per (scheme, burst, rate)"""
    import json
    from bnn.faults import faults
    network, dataset = "cnvW1A1", "cifar10"
    L, pdir = gm.load(network, dataset)
    n, runs, seed = 40, 3, 77
    imgs = sw.images(network, n, seed=21)
    path = sw.write_images(network, imgs, tmp_path, network)
    labels = gm.clean_classes(L, path).tolist()
    labels[0] = (labels[0] + 1) % 10
    ft = faults.CNVFaultTest(network, dataset, path, labels)
    assert faults.hardening_of("cnvW1A1-resilient-interleaved") == ("cnvW1A1", 3) and faults.hardening_of("lfcW1A1") == ("lfcW1A1", 0)
    acc, cnts = ft.run_memory_noise_test(runs, 2.0 ** -7, 2.0 ** -3, seed=seed, scheme=1, burst=4)
    rw, rt = gm.rates(network, 2.0 ** -7, 2.0 ** -3)
    got, counts, _ = hcampaign(L, path, 1, 4, runs, seed, rw, rt)
    assert ft.mem_noise_results.tolist() == got.tolist() and cnts.tolist() == counts.tolist()
    assert acc == [100.0 * (row == np.array(labels)).sum() / n for row in got]
    acc0, cnts0 = ft.run_memory_noise_test(runs, 2.0 ** -7, 2.0 ** -3, seed=seed)  # (today's path: [run][layer][2])
    assert cnts0.shape == (runs, 9, 2)
    nt = faults.NetworkTest(ft)
    nt.hardening_curve(str(tmp_path / "out"), 2, [0.0, 2.0 ** -3], [0, 1, 3], [1, 4], seed=5)
    with open(tmp_path / "out" / network / dataset / "hardening" / ("%s_%s_hardening_stats.json" % (network, dataset))) as f:
        doc = json.load(f)
    assert len(doc["results"]) == 3 * 2 * 2
    for scheme in ("none", "TMR", "resilient-interleaved"):
        for burst in (1, 4):
            zero = doc["results"]["%s burst %d upset rate 0" % (scheme, burst)]
            some = doc["results"]["%s burst %d upset rate %g" % (scheme, burst, 2.0 ** -3)]
            assert zero["runs"]["all"] == [nt.control] * 2 and zero["physical bits"] == 0
            assert some["physical bits"] > 0 and some["logical bits"] > 0
