"""Datapath upset-rate campaigns on the GPU (bnn_mi355x_act_noise_campaigns): every activation of every layer's
output upset with a per-layer probability, independently per run, image and site.  All checks are exact.

The draw keys on the image's INDEX IN THE FILE (and the run's seed, the layer and the site) and on nothing else of the
call: the same (seed, image index) gives the same upsets whatever the batch, the grouping of the runs or the kernel
form -- which is what lets these tests compare a call against calls cut differently.

The classes must be what the per-layer numpy restatement of tests/test_gpu_act_fault_sweep.py gives (its helpers are
imported; its self-check against the oracle's layer_ref is repeated here) with the mask of bnn_mi355x_act_noise_mask
applied to every layer's output before the next layer reads it, and what bnn_mi355x_act_fault_sweep reports for the
pairs that have exactly one upset in the whole network."""
import ctypes as C
import os

import numpy as np
import pytest

import act_noise_ref as ref
import gpu_lib as gl
import test_gpu_act_fault_sweep as sw

NETS = sw.NETS
ip = C.POINTER(C.c_int)
pytestmark = pytest.mark.gpu


def q32(p):
    return int(np.floor(p * 4294967296.0))


def campaign(L, path, runs, seed, rates, ncls=10):
    """-> (classes [runs, n], counts [runs, layers - 1], seeds [runs])"""
    rq = (C.c_uint * len(rates))(*rates)
    cnt, usec = C.c_int(0), C.c_float(0)
    p = L.bnn_mi355x_act_noise_campaigns(path.encode(), ncls, runs, seed, rq, len(rates), C.byref(cnt), C.byref(usec))
    assert p, L.bnn_mi355x_last_error().decode()
    n = cnt.value
    got = np.ctypeslib.as_array(p, shape=(max(runs * n, 1),))[: runs * n].copy().reshape(runs, n)
    L.free_results(p)
    assert n == 0 or usec.value > 0
    k = L.bnn_mi355x_last_act_noise_counts(None, 0)
    assert k == runs * len(rates)
    c = (C.c_long * k)()
    assert L.bnn_mi355x_last_act_noise_counts(c, k) == k
    s = (C.c_ulonglong * runs)()
    assert L.bnn_mi355x_last_act_noise_seeds(s, runs) == runs
    return got, np.array(c[:], np.int64).reshape(runs, len(rates)), list(s)


def lib_mask(L, seed, image, layer, rate):
    total = L.bnn_mi355x_act_noise_mask(seed, image, layer, rate, 0, None, 0)
    assert total >= 0
    rec = np.zeros((max(total, 1), 5), np.int32)
    assert L.bnn_mi355x_act_noise_mask(seed, image, layer, rate, 0, rec.ctypes.data_as(ip), total) == total
    return rec[:total]


def clean_classes(L, path, ncls=10):
    cnt = C.c_int(0)
    p = L.inference_multiple(path.encode(), ncls, C.byref(cnt), None, 0)
    assert p, L.bnn_mi355x_last_error().decode()
    out = np.ctypeslib.as_array(p, shape=(cnt.value,)).copy()
    L.free_results(p)
    return out


def restate_noise(L, rs, network, imgs, indices, seeds, rates, ncls=10):
    """the restatement: for every run seed and every image (imgs[j] has file index indices[j]) the network layer by
    layer with the library's mask applied to each layer's output -> (classes [runs, len(imgs)], upsets [runs, layers - 1])"""
    nl = len(rates)
    x0 = np.stack([rs.o.layer_ref(i, 0) for i in imgs])
    x = np.repeat(x0[None], len(seeds), axis=0).reshape(len(seeds) * len(imgs), -1)
    counts = np.zeros((len(seeds), nl), np.int64)
    for l in range(nl):
        for r, seed in enumerate(seeds):
            for j, idx in enumerate(indices):
                recs = lib_mask(L, seed, int(idx), l, rates[l])
                counts[r, l] += len(recs)
                x[r * len(imgs) + j] = ref.apply(network, x[r * len(imgs) + j], recs)
        if l + 1 < nl:
            x = np.concatenate([rs.layer(l + 1, x[i:i + 64]) for i in range(0, len(x), 64)])
    return sw.classes_of(rs, nl - 1, x, ncls).reshape(len(seeds), len(imgs)), counts


@pytest.fixture(scope="module")
def shipped_and_random(tmp_path_factory):
    import random_params
    sets = {}
    for k, (network, dataset) in enumerate(NETS):
        d = tmp_path_factory.mktemp("rpn_" + network)
        random_params.make(str(d), network, 171 + k)
        sets[network] = [gl.param_dir(dataset, network), str(d)]
    return sets


def test_restatement_self_check(shipped_and_random):
    """with no fault the restatement reproduces layer_ref at every layer and the oracle's scores / words at the end
    (the check of tests/test_gpu_act_fault_sweep.py, on this file's parameter sets)"""
    for network, _ in NETS:
        for pdir in shipped_and_random[network]:
            rs = sw.Restatement(network, pdir)
            imgs = sw.images(network, 6, seed=15)
            base = sw.fault_free(rs, imgs[:1])
            for l, x in enumerate(base):
                assert (x[0] == rs.o.layer_ref(imgs[0], l)).all(), (network, pdir, l)
            x = np.stack([rs.o.layer_ref(i, 0) for i in imgs])
            for l in range(1, len(rs.W)):
                x = rs.layer(l, x)
            if rs.cnv:
                assert ((x & 0xFFFF).astype(np.uint16).view(np.int16) == rs.o.scores_fast(imgs)).all(), (network, pdir)
            else:
                bits = sw.lfc_last(rs, x)[:, :64] > 0
                words = (bits.astype(np.uint64) << np.arange(64, dtype=np.uint64)).sum(axis=1, dtype=np.uint64)
                assert (words == rs.o.words_fast(imgs)).all(), (network, pdir)
            # ... and ref.apply moves one site the way the sweep's restatement does
            rec = np.array([[0, 0, 0, 5, 1]], np.int32)
            lv = ref.levels(network)
            i = (int(base[0][0, 5]) + 1) // (2 if lv == 2 else 1)
            k = (i + 1) % lv
            assert ref.apply(network, base[0][0], rec)[5] == ((2 * k - 1) if lv == 2 else (k - 1))
            rs.o.close()


@pytest.mark.parametrize("network,dataset", NETS, ids=lambda x: x)
def test_campaign_equals_restatement(network, dataset, shipped_and_random, tmp_path):
    """3 runs x 24 images, rates 2^-8 ... 2^-3 over the layers with one layer at 0, shipped and random parameters: the
    classes as restated with the library's masks, the device's upset counts equal to the mask sizes, and the library's
    masks equal to the numpy draw"""
    L = gl.load(network)
    nl = len(ref.maps(network))
    for p, pdir in enumerate(shipped_and_random[network]):
        L.load_parameters(pdir.encode())
        assert L.bnn_mi355x_last_error() == b"", L.bnn_mi355x_last_error()
        rs = sw.Restatement(network, pdir)
        rates = [q32(2.0 ** -(8 - (5 * l) // max(nl - 1, 1))) for l in range(nl)]  # 2^-8 (layer 0) ... 2^-3 (last hidden)
        rates[(1 + p) % nl] = 0
        n, runs, seed = 24, 3, 900 + 17 * p
        imgs = sw.images(network, n, seed=60 + p)
        path = sw.write_images(network, imgs, tmp_path, "n%d" % p)
        got, counts, seeds = campaign(L, path, runs, seed, rates)
        assert seeds == [seed + r for r in range(runs)]
        want, want_counts = restate_noise(L, rs, network, imgs, range(n), seeds, rates)
        print(network, pdir, "upsets per run and layer:", counts.tolist(), "classes changed:",
              int((got != clean_classes(L, path)[None]).sum()), "of", got.size)
        assert counts.tolist() == want_counts.tolist(), (network, pdir)
        assert (counts[:, (1 + p) % nl] == 0).all() and counts.sum() > 0
        assert got.tolist() == want.tolist(), (network, pdir)
        for l in range(nl):  # the library's masks are the numpy draw (the CPU suite walks this far wider)
            assert (lib_mask(L, seeds[1], 7, l, rates[l]) == ref.mask(network, seeds[1], 7, l, rates[l])).all()
        rs.o.close()
    L.load_parameters(shipped_and_random[network][0].encode())


@pytest.mark.parametrize("network,dataset,rate", [("cnvW1A1", "cifar10", 2.0 ** -17), ("cnvW2A2", "cifar10", 2.0 ** -17),
                                                  ("lfcW1A2", "mnist", 2.0 ** -12)], ids=lambda x: str(x))
def test_single_upsets_agree_with_the_sweep(network, dataset, rate, tmp_path):
    """a rate so low that many (run, image) pairs have exactly one upset in the whole network: each such pair's class
    is what bnn_mi355x_act_fault_sweep reports for that record and image.  No restatement involved."""
    L = gl.load(network)
    L.load_parameters(gl.param_dir(dataset, network).encode())
    nl = len(ref.maps(network))
    n, runs, seed = 32, 4, 4242
    imgs = sw.images(network, n, seed=77)
    path = sw.write_images(network, imgs, tmp_path)
    rates = [q32(rate)] * nl
    got, counts, seeds = campaign(L, path, runs, seed, rates)
    clean = clean_classes(L, path)
    singles = []  # (run, image, record)
    for r in range(runs):
        for i in range(n):
            recs = [lib_mask(L, seeds[r], i, l, rates[l]) for l in range(nl)]
            if sum(len(x) for x in recs) == 1:
                singles.append((r, i, np.concatenate(recs)[0]))
    assert len(singles) >= 10, len(singles)
    recs = np.array([s[2] for s in singles], np.int32)
    changed, diffs, total, got_n = sw.sweep(L, path, recs)
    assert got_n == n
    cls = {(int(f), int(i)): int(c) for f, i, c in diffs}
    differing = 0
    for f, (r, i, _) in enumerate(singles):
        assert got[r, i] == cls.get((f, i), clean[i]), (f, r, i)
        differing += got[r, i] != clean[i]
    print(network, len(singles), "pairs with exactly one upset,", differing, "of them change the class")
    none = [(r, i) for r in range(runs) for i in range(n) if all(len(lib_mask(L, seeds[r], i, l, rates[l])) == 0 for l in range(nl))]
    assert none and all(got[r, i] == clean[i] for r, i in none)


@pytest.mark.parametrize("network,dataset", NETS, ids=lambda x: x)
def test_zero_rates_runs_and_groups(network, dataset, tmp_path, monkeypatch):
    """all rates 0: the classes of inference_multiple once per run, counts 0.  One call of R runs equals R calls with
    seeds seed + r.  The same call cut into many small groups of (run, image) pairs gives the same classes and counts."""
    L = gl.load(network)
    L.load_parameters(gl.param_dir(dataset, network).encode())
    nl = len(ref.maps(network))
    n, runs, seed = 50, 5, 31337
    path = sw.write_images(network, sw.images(network, n, seed=3), tmp_path)
    clean = clean_classes(L, path)
    got0, counts0, _ = campaign(L, path, runs, seed, [0] * nl)
    assert (got0 == clean[None]).all() and (counts0 == 0).all()
    rates = [q32(2.0 ** -7)] * nl
    got, counts, seeds = campaign(L, path, runs, seed, rates)
    assert (got != clean[None]).any() and (counts > 0).all()
    for r in range(runs):
        one, c1, s1 = campaign(L, path, 1, seed + r, rates)
        assert s1 == [seeds[r]] and one[0].tolist() == got[r].tolist() and c1[0].tolist() == counts[r].tolist(), r
    for group in (7, 50, 64, 101):
        monkeypatch.setenv("BNN_MI355X_NOISE_GROUP", str(group))
        g2, c2, _ = campaign(L, path, runs, seed, rates)
        assert g2.tolist() == got.tolist() and c2.tolist() == counts.tolist(), group
    monkeypatch.delenv("BNN_MI355X_NOISE_GROUP")
    # seed 0: the seeds come from std::random_device, are reported, and replay the call
    ga, ca, sa = campaign(L, path, 2, 0, rates)
    assert all(s != 0 for s in sa) and sa[0] != sa[1]
    for r in range(2):
        one, c1, _ = campaign(L, path, 1, sa[r], rates)
        assert one[0].tolist() == ga[r].tolist() and c1[0].tolist() == ca[r].tolist()


def test_more_pairs_than_one_workspace(tmp_path):
    """133 072 MNIST images x 2 runs: three groups of the activation workspace, a run cut in the middle; the same as
    the call in smaller groups, and images of the second window as restated with their index in the file"""
    network, dataset = "lfcW1A1", "mnist"
    L = gl.load(network)
    pdir = gl.param_dir(dataset, network)
    L.load_parameters(pdir.encode())
    n, runs, seed = 133072, 2, 99
    imgs = sw.images(network, n, seed=8)
    path = sw.write_images(network, imgs, tmp_path, "all")
    rates = [q32(2.0 ** -6), 0, q32(2.0 ** -4)]
    got, counts, seeds = campaign(L, path, runs, seed, rates)
    os.environ["BNN_MI355X_NOISE_GROUP"] = "50000"
    try:
        g2, c2, _ = campaign(L, path, runs, seed, rates)
    finally:
        del os.environ["BNN_MI355X_NOISE_GROUP"]
    assert (g2 == got).all() and c2.tolist() == counts.tolist()
    idx = [0, 1, 131071, 131072, 131073, 133071] + list(range(132000, 132026))
    rs = sw.Restatement(network, pdir)
    want, _ = restate_noise(L, rs, network, imgs[idx], idx, seeds, rates)
    assert got[:, idx].tolist() == want.tolist()
    # the expected number of upsets: 1024 sites x n images x rate, within 6 standard deviations
    for l, p in ((0, 2.0 ** -6), (2, 2.0 ** -4)):
        mean = 1024.0 * n * p
        assert (abs(counts[:, l] - mean) < 6 * np.sqrt(mean)).all(), (l, counts[:, l].tolist(), mean)
    assert (counts[:, 1] == 0).all()
    rs.o.close()


def test_loaded_parameters_untouched(tmp_path):
    """classes, the parameter CRC, last_faults, last_campaign_faults and both sweeps' stage counts are the same before
    and after a campaign"""
    network, dataset = "cnvW2A2", "cifar10"
    L = gl.load(network)
    L.load_parameters(gl.param_dir(dataset, network).encode())
    imgs = sw.images(network, 64)
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
        a, b = (C.c_long * 9)(), (C.c_long * 9)()
        na, nb = L.bnn_mi355x_last_sweep_stages(a, 9), L.bnn_mi355x_last_act_sweep_stages(b, 9)
        k = L.bnn_mi355x_last_campaign_faults(None, 0)
        rec = (C.c_int * (9 * k))()
        L.bnn_mi355x_last_campaign_faults(rec, k)
        return (clean_classes(L, path).tolist(), L.bnn_mi355x_params_crc(), L.bnn_mi355x_last_faults(None, 0), na, list(a), nb, list(b), list(rec))

    before = state()
    got, counts, _ = campaign(L, path, 3, 11, [q32(2.0 ** -5)] * 8)
    assert (got != np.array(before[0])[None]).any() and counts.sum() > 0
    assert state() == before


def test_imported_blob_is_fine(tmp_path):
    """no parameter is patched: a library that holds an imported blob (no parameter files) runs the campaign, with the
    results of the loaded directory"""
    network, dataset = "lfcW1A2", "mnist"
    L = gl.load(network)
    pdir = gl.param_dir(dataset, network)
    L.load_parameters(pdir.encode())
    path = sw.write_images(network, sw.images(network, 40), tmp_path)
    rates = [q32(2.0 ** -5)] * 3
    want = campaign(L, path, 2, 8, rates)
    blob = gl.pack_params(network, pdir)
    assert L.bnn_mi355x_import_params(blob.ctypes.data, len(blob)) == 0
    got = campaign(L, path, 2, 8, rates)
    assert got[0].tolist() == want[0].tolist() and got[1].tolist() == want[1].tolist()
    L.load_parameters(pdir.encode())


def test_upset_rate_curve(tmp_path):
    """NetworkTest.upset_rate_curve writes one statistics file per (layer set, rate); rate 0 reproduces the control run,
    the effective rate is near the nominal one, and run_noise_test's accuracies follow from its classes"""
    import json
    from bnn.faults import faults
    for network, dataset, layer_sets in (("lfcW1A1", "mnist", ()), ("cnvW1A2", "cifar10", ([6, 7], 4))):
        n = 80
        imgs = sw.images(network, n, seed=21)
        path = sw.write_images(network, imgs, tmp_path, network)
        cls_ = faults.CNVFaultTest if network.startswith("cnv") else faults.LFCFaultTest
        L = gl.load(network)
        L.load_parameters(gl.param_dir(dataset, network).encode())
        labels = clean_classes(L, path).tolist()  # (so that the control accuracy is 100 % and upsets can only lower it)
        labels[0] = (labels[0] + 1) % 10
        ft = cls_(network, dataset, path, labels)
        nt = faults.NetworkTest(ft)
        nt.upset_rate_curve(str(tmp_path / "out"), 6, [0.0, 2.0 ** -6, 0.25], layers=layer_sets, seed=5)
        assert nt.control == pytest.approx(100.0 * (n - 1) / n)
        folder = tmp_path / "out" / network / dataset / "upsets"
        sets = [list(range(3))] if not layer_sets else [[6, 7], [4]]
        sites = np.array([h * w * c for h, w, c in ref.maps(network)])
        for which in sets:
            suffix = "" if not layer_sets else "_layer%s" % which
            accs = []
            for p in (0.0, 2.0 ** -6, 0.25):
                with open(folder / ("%s_%s_rate%g_stats%s.json" % (network, dataset, p, suffix))) as f:
                    doc = json.load(f)
                assert doc["control"] == nt.control and doc["layers"] == which and doc["run count"] == 6
                e = doc["results"]["upset rate %g" % p]
                assert len(e["runs"]["all"]) == 6 and e["min accuracy"] <= e["avg accuracy"] <= e["max accuracy"]
                ups = np.array(e["upsets per layer"])
                assert (ups[[l for l in range(len(sites)) if l not in which]] == 0).all()
                exposed = sites[which].sum() * 6 * n
                assert e["effective rate"] == pytest.approx(ups.sum() / exposed)
                if p == 0.0:
                    assert e["runs"]["all"] == [nt.control] * 6 and e["effective rate"] == 0 and e["stddev accuracy"] == 0
                else:
                    assert abs(e["effective rate"] - p) < 6 * np.sqrt(p / exposed)
                accs.append(e["avg accuracy"])
            assert accs[2] < accs[0]
        acc = ft.run_noise_test(3, 2.0 ** -5, seed=9)
        assert ft.noise_results.shape == (3, n) and ft.noise_counts.shape == (3, len(sites))
        assert acc == [100.0 * (row == np.array(labels)).sum() / n for row in ft.noise_results]
