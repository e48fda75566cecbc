"""Memory upset-rate campaigns on the GPU (bnn_mi355x_mem_noise_campaigns): every bit of the weight / threshold memories
flipped with a per-layer probability, independently per run, in place on the run's copy of the parameters from the first
image on.  All checks are exact.

The model is pinned to host functions the CPU suite walks (tests/test_mem_noise_mask.py): bnn_mi355x_mem_noise_mask says
which sites a run flips, bnn_mi355x_pack_params_faulty applies such records to the parameter files.  So the device's work
is checked byte for byte -- bnn_mi355x_mem_noise_params reads back the very blob a run classifies with -- and the classes
against the host route: import the host-built blob, classify the same images with bnn_mi355x_inference_buffer."""
import ctypes as C
import struct

import numpy as np
import pytest

import gpu_lib as gl
import test_gpu_act_fault_sweep as sw
import test_mem_noise_mask as mm

NETS = mm.NETS
ip = C.POINTER(C.c_int)
q32 = mm.q32
pytestmark = pytest.mark.gpu


def layout(network):
    return mm.params_io.layout(network)


def rates(network, w=0.0, t=0.0):
    """-> (rate_w_q32, rate_t_q32): w on every layer's weights, t on the thresholds of every layer that has any"""
    lay = layout(network)
    return [q32(w)] * len(lay), [q32(t) if F["nthr"] else 0 for F in lay]


def campaign(L, path, runs, seed, rw, rt, ncls=10):
    """-> (classes [runs, n], counts [runs, layers, 2], seeds [runs])"""
    up = C.c_uint * len(rw)
    cnt, usec = C.c_int(0), C.c_float(0)
    p = L.bnn_mi355x_mem_noise_campaigns(path.encode(), ncls, runs, seed, up(*rw), up(*rt), len(rw), C.byref(cnt), C.byref(usec))
    assert p, L.bnn_mi355x_last_error().decode()
    n = cnt.value
    got = np.ctypeslib.as_array(p, shape=(max(runs * n, 1),))[: runs * n].copy().reshape(runs, n)
    L.free_results(p)
    assert n == 0 or usec.value > 0
    k = L.bnn_mi355x_last_mem_noise_counts(None, 0)
    assert k == runs * len(rw) * 2
    c = (C.c_long * k)()
    assert L.bnn_mi355x_last_mem_noise_counts(c, k) == k
    s = (C.c_ulonglong * runs)()
    assert L.bnn_mi355x_last_mem_noise_seeds(s, runs) == runs
    return got, np.array(c[:], np.int64).reshape(runs, len(rw), 2), list(s)


def device_blob(L, seed, rw, rt):
    up = C.c_uint * len(rw)
    size = L.bnn_mi355x_mem_noise_params(seed, up(*rw), up(*rt), len(rw), None, 0)
    assert size > 0, L.bnn_mi355x_last_error().decode()
    blob = np.zeros(size, np.uint8)
    assert L.bnn_mi355x_mem_noise_params(seed, up(*rw), up(*rt), len(rw), blob.ctypes.data, size) == size, L.bnn_mi355x_last_error()
    return blob


def host_blob(L, network, pdir, seed, rw, rt, before=None):
    """the oracle: the records of `before` (faults already in the loaded parameters), then the run's masks, through
    pack_params_faulty"""
    recs = mm.all_masks(L, network, seed, rw, rt)
    if before is not None and len(before):
        recs = np.concatenate([np.asarray(before, np.int32).reshape(-1, 8), recs])
    return mm.pack_faulty(L, pdir, recs), recs


def assert_same_bytes(got, want, what):
    if (got == want).all():
        return
    assert len(got) == len(want), what
    d = int(np.nonzero(got.view(np.uint32) != want.view(np.uint32))[0][0])
    where = "outside the layers' rows"
    for l in range(struct.unpack_from("<I", want, 16)[0]):
        off, rd, rows, kw = struct.unpack_from("<4I", want, 32 + 16 * l)
        if off <= 4 * d < off + rows * rd * 4:
            where = "layer %d row %d dword %d of %d" % (l, (4 * d - off) // (rd * 4), (4 * d - off) // 4 % rd, rd)
    l0m = struct.unpack_from("<I", want, 24)[0]
    if l0m and 4 * d >= l0m:
        where = "layer 0's matrix-pipe tables, byte %d" % (4 * d - l0m)
    raise AssertionError("%s: first differing dword %d (%s): device %08x, host %08x; %d dwords differ" % (
        what, d, where, got.view(np.uint32)[d], want.view(np.uint32)[d], int((got.view(np.uint32) != want.view(np.uint32)).sum())))


def clean_classes(L, path, ncls=10):
    cnt = C.c_int(0)
    p = L.inference_multiple(path.encode(), ncls, C.byref(cnt), None, 0)
    assert p, L.bnn_mi355x_last_error().decode()
    out = np.ctypeslib.as_array(p, shape=(cnt.value,)).copy()
    L.free_results(p)
    return out


def classify_with_blob(L, blob, imgs, ncls=10):
    """the host route: import the blob, classify the images from a host buffer"""
    assert L.bnn_mi355x_import_params(blob.ctypes.data, len(blob)) == 0, L.bnn_mi355x_last_error()
    imgs = np.ascontiguousarray(imgs, np.uint8)
    p = L.bnn_mi355x_inference_buffer(imgs.ctypes.data, len(imgs), ncls, None, 0)
    assert p, L.bnn_mi355x_last_error().decode()
    out = np.ctypeslib.as_array(p, shape=(len(imgs),)).copy()
    L.free_results(p)
    return out


def load(network, dataset):
    L = gl.load(network)
    pdir = gl.param_dir(dataset, network)
    L.load_parameters(pdir.encode())
    assert L.bnn_mi355x_last_error() == b"", L.bnn_mi355x_last_error()
    return L, pdir


RATE_SETS = {"w8": (2.0 ** -8, 0.0), "w3": (2.0 ** -3, 0.0), "t5": (0.0, 2.0 ** -5), "both": (2.0 ** -3, 2.0 ** -5)}


@pytest.mark.parametrize("network,dataset", NETS, ids=lambda x: x)
def test_bytes(network, dataset):
    """two seeds x {weights 2^-8, weights 2^-3 (several flips per word, -2 fields in cnvW2A2), thresholds 2^-5 (both
    thresholds of a 2-bit neuron), both}: the blob the device made equals pack_params_faulty of the masks, all bytes"""
    L, pdir = load(network, dataset)
    clean = gl.pack_params(network, pdir)
    crc = L.bnn_mi355x_params_crc()
    for seed in (20261018, (0xABCD << 32) | 7):
        for name, (w, t) in RATE_SETS.items():
            rw, rt = rates(network, w, t)
            want, recs = host_blob(L, network, pdir, seed, rw, rt)
            assert len(recs) > 0 and (want != clean).any()
            assert_same_bytes(device_blob(L, seed, rw, rt), want, "%s seed %d %s" % (network, seed, name))
    rw, rt = rates(network)
    assert_same_bytes(device_blob(L, 5, rw, rt), clean, network + " all rates 0")
    assert L.bnn_mi355x_params_crc() == crc


PRE_SEED, PRE_FLIPS = 424242, 1500


def prefault(L, path):
    """-2 weights into layer 6 of the loaded cnvW2A2 parameters: inference_multiple_with_faults under a fixed seed,
    weight bits only; -> its records (last_faults)"""
    L.bnn_mi355x_set_fault_seed(PRE_SEED)
    cnt = C.c_int(0)
    layers = (C.c_int * 1)(6)
    p = L.inference_multiple_with_faults(path.encode(), 10, C.byref(cnt), None, PRE_FLIPS, 1, 0, layers, 1)
    assert p, L.bnn_mi355x_last_error().decode()
    L.free_results(p)
    L.bnn_mi355x_set_fault_seed(0)
    k = L.bnn_mi355x_last_faults(None, 0)
    assert k == PRE_FLIPS
    rec = (C.c_int * (8 * k))()
    L.bnn_mi355x_last_faults(rec, k)
    return np.array(rec[:], np.int32).reshape(k, 8)


def flags(blob, layer):
    off, rd, rows, kw = struct.unpack_from("<4I", blob, 32 + 16 * layer)
    return blob[off: off + rows * rd * 4].view(np.uint32).reshape(rows, rd)[:, 2 + 6 * kw]


def test_bytes_and_classes_from_prefaulted_parameters(tmp_path):
    """cnvW2A2 starting from parameters that already hold -2 rows: the expected blob is last_faults followed by the mask.
    Layer 6 at 2^-8 over eight seeds: rows lose their only -2 (the flag must go back to 0) and others gain one; layer 1 at
    2^-3 on top.  The host route itself must show both directions, or the check would be vacuous.  A campaign on these
    parameters classifies with exactly these blobs: it starts from the faulted parameters, not from the files."""
    network, dataset = "cnvW2A2", "cifar10"
    L, pdir = load(network, dataset)
    n = 24
    imgs = sw.images(network, n, seed=12)
    path = sw.write_images(network, imgs, tmp_path)
    before = prefault(L, path)
    start = mm.pack_faulty(L, pdir, before)
    assert flags(start, 6).sum() > 200
    crc = L.bnn_mi355x_params_crc()
    rw, rt = rates(network)
    rw[6], rw[1] = q32(2.0 ** -8), q32(2.0 ** -3)
    seed, runs = 7000, 8
    cleared = gained = 0
    blobs = []
    for r in range(runs):
        want, _ = host_blob(L, network, pdir, seed + r, rw, rt, before)
        cleared += int(((flags(start, 6) == 1) & (flags(want, 6) == 0)).sum())
        gained += int(((flags(start, 6) == 0) & (flags(want, 6) == 1)).sum())
        assert_same_bytes(device_blob(L, seed + r, rw, rt), want, "prefaulted cnvW2A2 seed %d" % (seed + r))
        blobs.append(want)
    print("flags cleared", cleared, "gained", gained)
    assert cleared >= 1 and gained >= 1
    got, counts, seeds = campaign(L, path, runs, seed, rw, rt)
    assert L.bnn_mi355x_params_crc() == crc and L.bnn_mi355x_last_faults(None, 0) == PRE_FLIPS
    assert counts[:, 6, 0].min() > 0 and counts[:, 1, 0].min() > 0 and counts[:, :, 1].sum() == 0
    for r in range(runs):
        assert got[r].tolist() == classify_with_blob(L, blobs[r], imgs).tolist(), r
    L.load_parameters(pdir.encode())


# the rate of test_campaign_equals_the_host_route, on all weights and all thresholds: 2^-9 was the starting guess
ROUTE_RATE = {"cnvW1A1": 2.0 ** -9, "cnvW1A2": 2.0 ** -9, "cnvW2A2": 2.0 ** -9, "lfcW1A1": 2.0 ** -9, "lfcW1A2": 2.0 ** -9}


@pytest.mark.parametrize("network,dataset", NETS, ids=lambda x: x)
def test_campaign_equals_the_host_route(network, dataset, tmp_path):
    """5 runs x 60 images (LFC: 200), a non-zero rate in every layer's weights and thresholds (ROUTE_RATE: 2^-9 for all
    five nets): the classes of run r are those of import_params(host-built blob of seed + r) + inference_buffer on the
    same images.  Not vacuous: the host route itself changes the class of at least one image in at least two runs."""
    L, pdir = load(network, dataset)
    n, runs, seed = (60 if network.startswith("cnv") else 200), 5, 1234
    imgs = sw.images(network, n, seed=44)
    path = sw.write_images(network, imgs, tmp_path)
    p = ROUTE_RATE[network]
    rw, rt = rates(network, p, p)
    clean = clean_classes(L, path)
    got, counts, seeds = campaign(L, path, runs, seed, rw, rt)
    assert seeds == [seed + r for r in range(runs)]
    want = []
    for r in range(runs):
        blob, recs = host_blob(L, network, pdir, seed + r, rw, rt)
        want.append(classify_with_blob(L, blob, imgs))
    # (the library now holds an imported blob: no raw memories to draw in -- refused as fault_campaigns refuses it)
    up = C.c_uint * len(rw)
    assert not L.bnn_mi355x_mem_noise_campaigns(path.encode(), 10, 1, 1, up(*rw), up(*rt), len(rw), None, None)
    assert b"imported blob" in L.bnn_mi355x_last_error()
    assert L.bnn_mi355x_mem_noise_params(1, up(*rw), up(*rt), len(rw), None, 0) == 0
    L.load_parameters(pdir.encode())
    changed = [int((w != clean).sum()) for w in want]
    print(network, "rate", p, "images whose class the host route changes, per run:", changed)
    assert sum(c >= 1 for c in changed) >= 2
    for r in range(runs):
        assert got[r].tolist() == want[r].tolist(), r
    assert clean_classes(L, path).tolist() == clean.tolist()


@pytest.mark.parametrize("network,dataset", NETS, ids=lambda x: x)
def test_zero_rates_groups_and_counts(network, dataset, tmp_path, monkeypatch):
    """all rates 0: the clean classes once per run, counts 0.  5 runs x 260 images in groups of 37 and of 1 000 pairs
    (groups end inside runs, a run spans several groups): classes and counts as in the ungrouped call.  The counts are the
    lengths of the masks of the seeds the call reports -- also for a seed-0 call, whose seeds replay it."""
    L, pdir = load(network, dataset)
    n, runs, seed = 260, 5, 31337
    path = sw.write_images(network, sw.images(network, n, seed=3), tmp_path)
    clean = clean_classes(L, path)
    rw0, rt0 = rates(network)
    got0, counts0, _ = campaign(L, path, runs, seed, rw0, rt0)
    assert (got0 == clean[None]).all() and (counts0 == 0).all()
    rw, rt = rates(network, 2.0 ** -9, 2.0 ** -7)
    got, counts, seeds = campaign(L, path, runs, seed, rw, rt)
    assert (got != clean[None]).any()

    def mask_counts(ss):
        return [[[L.bnn_mi355x_mem_noise_mask(s, l, t, (rw, rt)[t][l], 0, None, 0) for t in (0, 1)] for l in range(len(rw))] for s in ss]

    assert counts.tolist() == mask_counts(seeds)
    assert (counts[:, :, 0] > 0).all()
    for group in (37, 1000):
        monkeypatch.setenv("BNN_MI355X_NOISE_GROUP", str(group))
        g2, c2, _ = campaign(L, path, runs, seed, rw, rt)
        assert g2.tolist() == got.tolist() and c2.tolist() == counts.tolist(), group
        z2, zc2, _ = campaign(L, path, runs, seed, rw0, rt0)
        assert (z2 == clean[None]).all() and (zc2 == 0).all()
    monkeypatch.delenv("BNN_MI355X_NOISE_GROUP")
    ga, ca, sa = campaign(L, path, 2, 0, rw, rt)
    assert all(s != 0 for s in sa) and sa[0] != sa[1]
    assert ca.tolist() == mask_counts(sa)
    for r in range(2):
        one, c1, s1 = campaign(L, path, 1, sa[r], rw, rt)
        assert s1 == [sa[r]] and one[0].tolist() == ga[r].tolist() and c1[0].tolist() == ca[r].tolist()


def test_more_pairs_than_one_workspace(tmp_path):
    """lfcW1A1, 300 runs x 500 images = 150 000 pairs at 2^-12: two groups of the activation workspace, run 262 cut in the
    middle.  The first, the last and a middle run (the cut one) against the host route."""
    network, dataset = "lfcW1A1", "mnist"
    L, pdir = load(network, dataset)
    n, runs, seed = 500, 300, 5150
    imgs = sw.images(network, n, seed=8)
    path = sw.write_images(network, imgs, tmp_path)
    rw, rt = rates(network, 2.0 ** -12, 2.0 ** -12)
    got, counts, seeds = campaign(L, path, runs, seed, rw, rt)
    sites = np.array([F["pe"] * F["wmem"] * F["simd"] for F in layout(network)], np.float64)
    mean = sites * runs * 2.0 ** -12
    assert (abs(counts[:, :, 0].sum(axis=0) - mean) < 6 * np.sqrt(mean)).all(), (counts[:, :, 0].sum(axis=0), mean)
    want = {}
    for r in (0, 131072 // n, runs - 1):
        blob, _ = host_blob(L, network, pdir, seeds[r], rw, rt)
        want[r] = classify_with_blob(L, blob, imgs)
    L.load_parameters(pdir.encode())
    for r, w in want.items():
        assert got[r].tolist() == w.tolist(), r
    assert (got != clean_classes(L, path)[None]).any()


def test_state_untouched(tmp_path):
    """params_crc, last_faults, last_campaign_faults, the sweeps' stage counts and a following plain inference_multiple
    are the same before and after a campaign and a mem_noise_params call"""
    network, dataset = "cnvW1A2", "cifar10"
    L, pdir = load(network, dataset)
    imgs = sw.images(network, 48)
    path = sw.write_images(network, imgs, tmp_path)
    rec8 = np.array([[0, 0, 2, 0, 0, 0, 3, 1]], np.int32)
    ch = np.zeros(1, np.int32)
    assert L.bnn_mi355x_fault_sweep(path.encode(), 10, rec8.ctypes.data_as(ip), 1, ch.ctypes.data_as(ip), None, 0, None, None) >= 0
    sw.sweep(L, path, sw.enumerate_act(L, 6)[::53])
    cnt = C.c_int(0)
    p = L.bnn_mi355x_fault_campaigns(path.encode(), 10, 2, 5, 3, 1, -1, None, 0, C.byref(cnt), None)
    assert p
    L.free_results(p)

    def state():
        a, b, c = (C.c_long * 9)(), (C.c_long * 9)(), (C.c_long * 10)()
        na, nb = L.bnn_mi355x_last_sweep_stages(a, 9), L.bnn_mi355x_last_act_sweep_stages(b, 9)
        nc = L.bnn_mi355x_last_input_sweep_stages(c, 10)
        k = L.bnn_mi355x_last_campaign_faults(None, 0)
        rec = (C.c_int * (9 * k))()
        L.bnn_mi355x_last_campaign_faults(rec, k)
        return (clean_classes(L, path).tolist(), L.bnn_mi355x_params_crc(), L.bnn_mi355x_last_faults(None, 0), na, list(a), nb, list(b),
                nc, list(c), list(rec))

    before = state()
    rw, rt = rates(network, 2.0 ** -6, 2.0 ** -5)
    got, counts, _ = campaign(L, path, 3, 11, rw, rt)
    assert (got != np.array(before[0])[None]).any() and counts.sum() > 0
    device_blob(L, 11, rw, rt)
    assert state() == before


def test_python_interface(tmp_path):
    """FaultTest.run_memory_noise_test on 40 images, 3 runs: the accuracies follow from the C call's classes and the
    labels, the counts are the C call's; memory_upset_rate_curve writes one file per target"""
    import json
    from bnn.faults import faults
    for network, dataset, cls_ in (("cnvW1A1", "cifar10", faults.CNVFaultTest), ("lfcW1A2", "mnist", faults.LFCFaultTest)):
        L, pdir = load(network, dataset)
        n, runs, seed = 40, 3, 77
        imgs = sw.images(network, n, seed=21)
        path = sw.write_images(network, imgs, tmp_path, network)
        labels = clean_classes(L, path).tolist()
        labels[0] = (labels[0] + 1) % 10
        ft = cls_(network, dataset, path, labels)
        acc, cnts = ft.run_memory_noise_test(runs, 2.0 ** -7, 2.0 ** -6, seed=seed)
        rw, rt = rates(network, 2.0 ** -7, 2.0 ** -6)
        got, counts, _ = campaign(L, path, runs, seed, rw, rt)
        assert ft.mem_noise_results.tolist() == got.tolist() and cnts.tolist() == counts.tolist()
        assert acc == [100.0 * (row == np.array(labels)).sum() / n for row in got]
        nt = faults.NetworkTest(ft)
        nt.memory_upset_rate_curve(str(tmp_path / "out"), 3, [0.0, 2.0 ** -5], layers=([1, 2],), seed=5)
        assert nt.control == pytest.approx(100.0 * (n - 1) / n)
        for target in ("weights", "thresholds"):
            with open(tmp_path / "out" / network / dataset / "memory-upsets" / ("%s_%s_%s_stats.json" % (network, dataset, target))) as f:
                doc = json.load(f)
            zero = doc["results"]["%s upset rate 0 layer[1, 2]" % target]
            some = doc["results"]["%s upset rate %g layer[1, 2]" % (target, 2.0 ** -5)]
            assert zero["runs"]["all"] == [nt.control] * 3 and zero["effective rate"] == 0
            t = 0 if target == "weights" else 1
            bits = sum(L.bnn_mi355x_enumerate_faults(l, t, 1, 0, None, 0) for l in (1, 2))
            assert abs(some["effective rate"] - 2.0 ** -5) < 6 * np.sqrt(2.0 ** -5 / (bits * 3))
            assert sum(some["flips per layer"]) == sum(some["flips per layer"][1:3]) > 0
