"""Input-buffer faults on the GPU: bnn_mi355x_input_fault_sweep (one bit of one input byte flipped while an image is
classified) and bnn_mi355x_input_noise_campaigns (every bit flipped with probability p).  A faulted image is just
another image, so the expectation of every check is what the fault-free entry point bnn_mi355x_inference_buffer
returns for the bytes with those bits XORed on the host.  All checks are exact."""
import ctypes as C

import numpy as np
import pytest

import gpu_lib as gl
from test_gpu_act_fault_sweep import write_images

pytestmark = pytest.mark.gpu
ip = C.POINTER(C.c_int)
NETS = [("cnvW1A1", "cifar10"), ("cnvW2A2", "cifar10"), ("lfcW1A1", "mnist")]
N_IMAGES = 16
POOL = 384


def edge_bytes(network):
    """the bytes a 16-byte lane or a plane boundary can get wrong"""
    if network.startswith("cnv"):
        return [0, 15, 16, 1023, 1024, 2047, 2048, 3071]
    return [0, 15, 16, 783, 768]  # (768 ... 783: the last full 16-byte lane)


def records_of(network, seed=3):
    """the edge bytes x bits 0 and 7, and a dozen seeded random sites"""
    isz = 3072 if network.startswith("cnv") else 784
    rec = [(b, bit) for b in edge_bytes(network) for bit in (0, 7)]
    rng = np.random.default_rng(seed)
    rec += [(int(b), int(bit)) for b, bit in zip(rng.integers(0, isz, 12), rng.integers(0, 8, 12))]
    return np.array(rec, np.int32)


def flipped(imgs, recs):
    """[k, n, bytes]: every image with each record's bit XORed on the host"""
    out = np.repeat(imgs[None], len(recs), axis=0)
    for f, (b, bit) in enumerate(recs):
        out[f, :, b] ^= np.uint8(1 << bit)
    return out


def expect_sweep(net, imgs, recs, clean, ncls=10):
    """-> (classes [k, n] of the host-perturbed images, changed [k], diffs [m, 3])"""
    cls = net.classify(flipped(imgs, recs), ncls).reshape(len(recs), len(imgs))
    f, i = np.nonzero(cls != clean[None])
    return cls, (cls != clean[None]).sum(axis=1), np.stack([f, i, cls[f, i]], axis=1).astype(np.int32)


def sweep(L, path, recs, cap=None, ncls=10):
    """-> (changed [k], diffs [m, 3], total, n)"""
    recs = np.ascontiguousarray(recs, np.int32)
    k = len(recs)
    changed = np.full(max(k, 1), -7, np.int32)
    cap = k * 1000 if cap is None else cap
    diffs = np.zeros((max(cap, 1), 3), np.int32)
    cnt, usec = C.c_int(0), C.c_float(0)
    total = L.bnn_mi355x_input_fault_sweep(path.encode(), ncls, recs.ctypes.data_as(ip), k, changed.ctypes.data_as(ip),
                                           diffs.ctypes.data_as(ip), cap, C.byref(cnt), C.byref(usec))
    assert total >= 0, L.bnn_mi355x_last_error().decode()
    return changed[:k], diffs[:min(cap, total)], total, cnt.value


def stages(L):
    s = L.bnn_mi355x_last_input_sweep_stages(None, 0)
    out = (C.c_long * max(s, 1))()
    assert L.bnn_mi355x_last_input_sweep_stages(out, s) == s
    return np.array(out[:s], np.int64)


def campaign(L, path, runs, seed, rate, ncls=10):
    """-> (classes [runs, n], counts [runs], seeds [runs])"""
    cnt, usec = C.c_int(0), C.c_float(0)
    p = L.bnn_mi355x_input_noise_campaigns(path.encode(), ncls, runs, seed, rate, C.byref(cnt), C.byref(usec))
    assert p, L.bnn_mi355x_last_error().decode()
    n = cnt.value
    got = np.ctypeslib.as_array(p, shape=(max(runs * n, 1),))[: runs * n].copy().reshape(runs, n)
    L.free_results(p)
    assert L.bnn_mi355x_last_input_noise_counts(None, 0) == runs
    c = (C.c_long * runs)()
    assert L.bnn_mi355x_last_input_noise_counts(c, runs) == runs
    s = (C.c_ulonglong * runs)()
    assert L.bnn_mi355x_last_input_noise_seeds(s, runs) == runs
    return got, np.array(c[:], np.int64), list(s)


def lib_mask(L, seed, image, rate):
    total = L.bnn_mi355x_input_noise_mask(seed, image, rate, 0, None, 0)
    assert total >= 0
    rec = np.zeros((max(total, 1), 2), np.int32)
    assert L.bnn_mi355x_input_noise_mask(seed, image, rate, 0, rec.ctypes.data_as(ip), total) == total
    return rec[:total]


def noisy(L, imgs, indices, seeds, rate):
    """-> (images [runs, len(indices), bytes] with the library's masks XORed on the host, flips [runs])"""
    out = np.repeat(imgs[indices][None], len(seeds), axis=0)
    flips = np.zeros(len(seeds), np.int64)
    for r, seed in enumerate(seeds):
        for j, i in enumerate(indices):
            rec = lib_mask(L, seed, int(i), rate)
            flips[r] += len(rec)
            np.bitwise_xor.at(out[r, j], rec[:, 0], (1 << rec[:, 1]).astype(np.uint8))
    return out, flips


class Case:
    """a loaded network, N_IMAGES images in a file, the fault-free classes and the sweep's host expectation, made once"""

    def __init__(self, network, dataset, tmp):
        self.network, self.net = network, gl.Net(network, dataset)
        self.L = self.net.L
        self.recs = records_of(network)
        # Candidate images: uniform bytes, every record's byte at 127 or 128 (bit 7 of either crosses the LFC binariser's
        # threshold and the sign of layer 0's int8 input; bit 0 of 127 / 128 moves that input by one step).  The test set
        # is the candidates on which most records change the class, then the first of the others: some record changes
        # a class, and with the whole set drawn the same way some record changes none (both asserted by the tests).
        pool = np.random.default_rng(31).integers(0, 256, (POOL, self.net.isz), dtype=np.uint8)
        for j, b in enumerate(sorted(set(self.recs[:, 0].tolist()))):
            pool[:, b] = np.where((np.arange(POOL) + j) % 2, 127, 128).astype(np.uint8)
        clean = self.net.classify(pool, 10)
        _, changed, diffs = expect_sweep(self.net, pool, self.recs, clean)
        per_image = np.bincount(diffs[:, 1], minlength=POOL)
        order = np.argsort(-per_image, kind="stable")
        pick = np.sort(np.concatenate([order[:4], np.setdiff1d(np.arange(POOL), order[:4])[:N_IMAGES - 4]]))
        self.imgs = np.ascontiguousarray(pool[pick])
        self.path = write_images(network, self.imgs, tmp, network)
        self.clean = clean[pick]
        self.cls, self.changed, self.diffs = expect_sweep(self.net, self.imgs, self.recs, self.clean)


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    made = {}

    def get(network, dataset):
        if network not in made:
            made[network] = Case(network, dataset, tmp_path_factory.mktemp("in_" + network))
        return made[network]
    return get


@pytest.mark.parametrize("network,dataset", NETS, ids=lambda x: x)
def test_sweep_equals_host_perturbed_images(network, dataset, cases, monkeypatch):
    """changed, diffs and the return value are what inference_buffer gives for every image with the record's bit XORed
    on the host; again in groups of a few dozen pairs (several groups and image windows); the first stage runs every
    pair and the counts never grow"""
    c = cases(network, dataset)
    k, n = len(c.recs), N_IMAGES
    assert (c.changed > 0).any(), "no record changes a class: the test would pass vacuously"
    assert (c.changed == 0).any(), "every record changes a class: the pruned pairs are not covered"
    assert 127 in c.imgs[:, c.recs[0, 0]] and 128 in c.imgs[:, c.recs[0, 0]]
    for group in (None, 40, 9):  # (9 < n: image windows of one record)
        if group:
            monkeypatch.setenv("BNN_MI355X_SWEEP_GROUP", str(group))
        changed, diffs, total, cnt = sweep(c.L, c.path, c.recs)
        assert cnt == n and total == c.changed.sum() == len(diffs), group
        assert changed.tolist() == c.changed.tolist(), group
        assert diffs.tolist() == c.diffs.tolist(), group
        st = stages(c.L)
        assert len(st) == (9 if network.startswith("cnv") else 4)
        assert st[0] == k * n and (np.diff(st) <= 0).all(), st
    monkeypatch.delenv("BNN_MI355X_SWEEP_GROUP")
    # the first cap_diffs diffs only; no diffs at all; no records
    changed, diffs, total, _ = sweep(c.L, c.path, c.recs, cap=1)
    assert total == c.changed.sum() and diffs.tolist() == c.diffs[:1].tolist() and changed.tolist() == c.changed.tolist()
    changed, diffs, total, _ = sweep(c.L, c.path, c.recs, cap=0)
    assert total == c.changed.sum() and changed.tolist() == c.changed.tolist()
    assert sweep(c.L, c.path, c.recs[:0])[2] == 0
    # ... and the loaded parameters still classify as before
    assert (c.net.classify(c.imgs, 10) == c.clean).all()


def test_lfc_bits_below_the_msb_change_nothing(cases):
    """binarisation reads bit 7 only: every bit 0 ... 6 record reports 0 changed images and is pruned after layer 0;
    bit 7 of the 127 / 128 pixels changes some class"""
    c = cases("lfcW1A1", "mnist")
    low = np.array([(b, bit) for b in edge_bytes("lfcW1A1") + [400, 511] for bit in range(7)], np.int32)
    changed, diffs, total, n = sweep(c.L, c.path, low)
    assert total == 0 and len(diffs) == 0 and (changed == 0).all()
    st = stages(c.L)
    assert st[0] == len(low) * n and (st[1:] == 0).all()
    assert c.changed[c.recs[:, 1] == 7].sum() > 0
    assert (c.changed[c.recs[:, 1] != 7] == 0).all()


@pytest.mark.parametrize("network,dataset", NETS, ids=lambda x: x)
def test_campaign_equals_host_perturbed_images(network, dataset, cases, monkeypatch):
    """3 runs at 2^-6 with a fixed seed: the classes, run-major, are inference_buffer's for each pair's image with
    input_noise_mask XORed on the host, the device's counts the mask totals exactly; rate 0; rate 2^32 - 1; small groups"""
    c = cases(network, dataset)
    runs, seed, n = 3, 1234567, N_IMAGES
    idx = np.arange(n)
    for rate in (1 << 26, 0xFFFFFFFF):
        imgs, flips = noisy(c.L, c.imgs, idx, [seed + r for r in range(runs)], rate)
        want = c.net.classify(imgs, 10).reshape(runs, n)
        got, counts, seeds = campaign(c.L, c.path, runs, seed, rate)
        assert seeds == [seed + r for r in range(runs)]
        assert counts.tolist() == flips.tolist(), rate
        assert (got == want).all(), rate
        if rate == 1 << 26:
            bits = n * c.net.isz * 8
            assert (np.abs(flips - bits / 64) <= 6 * np.sqrt(bits * 63 / 4096)).all()  # (binomial, p = 2^-6)
            for group in (7, 23):  # (not multiples of n: groups that end inside a run)
                monkeypatch.setenv("BNN_MI355X_NOISE_GROUP", str(group))
                g2, c2, _ = campaign(c.L, c.path, runs, seed, rate)
                assert (g2 == got).all() and c2.tolist() == counts.tolist(), group
            monkeypatch.delenv("BNN_MI355X_NOISE_GROUP")
        else:
            assert (flips >= n * c.net.isz * 8 - 2 * n).all()  # (u = 2^32 - 1 is the only draw this rate misses)
            assert (got != c.clean[None]).any()  # (nearly every bit flipped: the check above is not one of equal classes)
    for group in (None, 7):
        if group:
            monkeypatch.setenv("BNN_MI355X_NOISE_GROUP", str(group))
        got, counts, _ = campaign(c.L, c.path, runs, seed, 0)
        assert (got == c.clean[None]).all() and (counts == 0).all()
    monkeypatch.delenv("BNN_MI355X_NOISE_GROUP")
    # seed 0: every run's seed from std::random_device, never 0, and the results follow them
    got, counts, seeds = campaign(c.L, c.path, 2, 0, 1 << 26)
    assert all(seeds) and seeds[0] != seeds[1]
    imgs, flips = noisy(c.L, c.imgs, idx, seeds, 1 << 26)
    assert counts.tolist() == flips.tolist() and (got == c.net.classify(imgs, 10).reshape(2, n)).all()
    assert (c.net.classify(c.imgs, 10) == c.clean).all()


def test_campaign_group_on_the_matrix_cores(cases, tmp_path):
    """cnvW1A1, runs x 8 images sized so that the call's one group takes the matrix-core conv stages: a seeded sample
    of 64 pairs against the same host expectation, the counts of their runs' other pairs included in the total"""
    c = cases("cnvW1A1", "cifar10")
    L = c.L
    assert L.bnn_mi355x_matrix_stages(1) >= 0  # (-1: nothing loaded)
    size = next(m for m in range(1, 1 << 15) if (L.bnn_mi355x_matrix_stages(m) & 0xE) == 0xE)  # (layers 1-3 as MFMA kernels)
    n = 8
    runs = -(-size // n)
    assert runs * n >= size and runs <= 4096
    path = write_images("cnvW1A1", c.imgs[:n], tmp_path, "mx")
    seed, rate = 99, 1 << 26
    got, counts, seeds = campaign(L, path, runs, seed, rate)
    assert got.shape == (runs, n) and seeds[-1] == seed + runs - 1
    rng = np.random.default_rng(8)
    sample = sorted(set(map(tuple, np.stack([rng.integers(0, runs, 64), rng.integers(0, n, 64)], axis=1).tolist())))
    imgs = np.stack([noisy(L, c.imgs[:n], [i], [seed + r], rate)[0][0, 0] for r, i in sample])
    want = c.net.classify(imgs, 10)
    assert [int(got[r, i]) for r, i in sample] == want.tolist()
    for r in sorted({r for r, _ in sample})[:8]:
        assert counts[r] == noisy(L, c.imgs[:n], np.arange(n), [seed + r], rate)[1][0]


def test_variant_and_bad_records_refused(variant_libs, cases):
    c = cases("cnvW1A1", "cifar10")
    ch = (C.c_int * 2)()
    bad = (C.c_int * 4)(0, 0, 3072, 1)
    assert c.L.bnn_mi355x_input_fault_sweep(c.path.encode(), 10, bad, 2, ch, None, 0, None, None) == -1
    assert b"record 1 {3072, 1}" in c.L.bnn_mi355x_last_error()
    assert c.L.bnn_mi355x_last_input_sweep_stages(None, 0) == 0
    V = gl.load("cnvW1A1-TMR")
    ok = (C.c_int * 2)(0, 0)
    assert V.bnn_mi355x_input_fault_sweep(c.path.encode(), 10, ok, 1, ch, None, 0, None, None) == -1
    assert b"not modelled" in V.bnn_mi355x_last_error()
    cnt = C.c_int(0)
    assert not V.bnn_mi355x_input_noise_campaigns(c.path.encode(), 10, 2, 5, 1 << 20, C.byref(cnt), None)
    assert b"not modelled" in V.bnn_mi355x_last_error()


@pytest.mark.parametrize("network,dataset,shape", [("cnvW1A1", "cifar10", (3, 32, 32, 8)), ("lfcW1A1", "mnist", (28, 28, 8))],
                         ids=lambda x: str(x))
def test_input_sensitivity_map(network, dataset, shape, cases, tmp_path):
    """NetworkTest.input_sensitivity_map on 8 images: the documented shape, site order, the sweep's total; the curve's
    statistics files"""
    import json
    from bnn.faults import faults
    c = cases(network, dataset)
    path = write_images(network, c.imgs[:8], tmp_path, network)
    labels = c.clean[:8].tolist()
    ft = (faults.CNVFaultTest if network.startswith("cnv") else faults.LFCFaultTest)(network, dataset, path, labels)
    cm = faults.NetworkTest(ft).input_sensitivity_map(str(tmp_path / "out"))
    assert cm.shape == shape
    k = c.net.isz * 8
    all_sites = np.stack([np.arange(k) >> 3, np.arange(k) & 7], axis=1).astype(np.int32)
    changed, _, total, n = sweep(c.L, path, all_sites, cap=0)
    assert n == 8 and cm.sum() == total and cm.ravel().tolist() == changed.tolist()
    for f, (b, bit) in enumerate(c.recs):  # (the map's axes: the byte in the image's own layout, then the bit)
        assert cm.reshape(-1, 8)[b, bit] == (c.cls[f, :8] != c.clean[:8]).sum()
    assert ft.control_accuracy == 100.0
    with open(tmp_path / "out" / network / dataset / "sensitivity" / (network + "_input.json")) as f:
        doc = json.load(f)
    assert doc["map"] == list(shape) and doc["totals"]["sites"] == k and sum(doc["changed"]) == total
    if network.startswith("lfc"):
        assert cm[..., :7].sum() == 0
    # the upset-rate curve: rate 0 is the control, the effective rate is what the device counted
    net = faults.NetworkTest(ft)
    net.input_upset_rate_curve(str(tmp_path / "out"), 2, [2.0 ** -6], seed=5)
    assert net.control == 100.0
    with open(tmp_path / "out" / network / dataset / "input-upsets" / ("%s_%s_rate%g_stats.json" % (network, dataset, 2.0 ** -6))) as f:
        e = json.load(f)["results"]["input upset rate %g" % 2.0 ** -6]
    assert e["flips"] == int(ft.input_noise_counts.sum()) and abs(e["effective rate"] - 2.0 ** -6) < 2.0 ** -8
    assert ft.input_noise_results.shape == (2, 8)
