"""Repair scrubs in the exposure campaigns, on the GPU (bnn_mi355x_repair_exposure_campaigns; the model: csrc/mem_org.h
"repair scrubs", csrc/ecc.h).  All checks are exact.

The model is pinned on the host: bnn_mi355x_pack_params_repair applies an ordered list of physical records with repair
and rewrite markers (tests/test_repair_pack.py, against the plain-Python route of tests/repair_ref.py).  The blob of (run,
epoch t) must be pack_params_repair of the marker-and-mask stream of epochs 0 ... t; bnn_mi355x_repair_exposure_params
reads back the very blob the device classifies that epoch with, and the epoch's classes are compared with
import_params(blob) + inference_buffer in a second library handle.  The eight counts are what repair_ref's stepped
physical state gives.

The exposure tests' shape: 3 runs x 48 images, rates 2^-3 and 2^-8 per epoch, epochs of 12 images (4 epochs) and of 10
(5, the last one short), two groupings of the pairs.  The masks of the small memories (every threshold memory, check
memories included, and layer 0) are restated in plain Python at 2^-3; the weights of layers >= 1 are the library's."""
import ctypes as C
import faulthandler
import json

import numpy as np
import pytest

import ecc_ref as er
import gpu_lib as gl
import hardened_ref as hr
import repair_ref as rr
import test_gpu_act_fault_sweep as sw
import test_gpu_ecc_exposure as ge
import test_gpu_exposure as gx
import test_gpu_mem_noise as gm
import test_mem_noise_mask as mm

pytestmark = pytest.mark.gpu
q32 = hr.q32
RUNS, N, SEED = 3, 48, 20261119
RATES = (2.0 ** -3, 2.0 ** -8)
EPOCH_IMAGES = (12, 10)
T_MAX = 5
DATASET = dict(mm.NETS)
# (network, scheme, code, burst, layer 0's rates zero)
CASES = [("cnvW1A1", 1, 0, 1, False), ("cnvW1A1", 1, 0, 4, False), ("cnvW1A1", 0, 1, 1, True), ("cnvW1A1", 2, 1, 1, False),
         ("cnvW1A1", 2, 1, 4, False), ("cnvW1A2", 1, 0, 1, False), ("cnvW2A2", 1, 0, 4, False), ("lfcW1A1", 0, 1, 1, False)]
# (scrub_every, repair_every): a repair every epoch, every other epoch, and every epoch with a rewrite before epoch 3 in its place
SCHEDULES = [(0, 1), (0, 2), (3, 1)]


@pytest.fixture(autouse=True)
def _time_limit():
    """every test runs in this process under a limit of its own (a case takes a few seconds): a device call that hangs
    ends the process with a traceback, and nothing more is started on the card"""
    faulthandler.dump_traceback_later(180, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def rcampaign(L, path, scheme, code, burst, runs, seed, rw, rt, epoch_images, scrub_every=0, repair_every=0, ncls=10):
    """-> (classes [runs, n], counts [runs, epochs, layers, 8], seeds [runs])"""
    up = C.c_uint * len(rw)
    cnt, usec = C.c_int(0), C.c_float(0)
    p = L.bnn_mi355x_repair_exposure_campaigns(path.encode(), ncls, scheme, code, burst, runs, seed, up(*rw), up(*rt), len(rw), epoch_images,
                                               scrub_every, repair_every, C.byref(cnt), C.byref(usec))
    assert p, L.bnn_mi355x_last_error().decode()
    n = cnt.value
    got = np.ctypeslib.as_array(p, shape=(max(runs * n, 1),))[: runs * n].copy().reshape(runs, n)
    L.free_results(p)
    epochs = -(-n // epoch_images)
    k = L.bnn_mi355x_last_repair_exposure_counts(None, 0)
    assert k == runs * epochs * len(rw) * 8
    c = (C.c_long * k)()
    assert L.bnn_mi355x_last_repair_exposure_counts(c, k) == k
    s = (C.c_ulonglong * runs)()
    assert L.bnn_mi355x_last_repair_exposure_seeds(s, runs) == runs
    return got, np.array(c[:], np.int64).reshape(runs, epochs, len(rw), 8), list(s)


def rdevice_blob(L, scheme, code, burst, seed, rw, rt, epoch, scrub_every=0, repair_every=0):
    up = C.c_uint * len(rw)
    size = L.bnn_mi355x_repair_exposure_params(scheme, code, burst, seed, up(*rw), up(*rt), len(rw), epoch, scrub_every, repair_every, None, 0)
    assert size > 0, L.bnn_mi355x_last_error().decode()
    blob = np.zeros(size, np.uint8)
    assert L.bnn_mi355x_repair_exposure_params(scheme, code, burst, seed, up(*rw), up(*rt), len(rw), epoch, scrub_every, repair_every,
                                               blob.ctypes.data, size) == size
    return blob


def rates_of(network, p, zero_layer_0=False):
    rw, rt = gm.rates(network, p, p)
    if zero_layer_0:
        rw, rt = [0] + list(rw[1:]), [0] + list(rt[1:])
    return list(rw), list(rt)


def drawn_epochs(L, network, scheme, code, burst, seed, rw, rt, restate, epochs=T_MAX):
    out = []
    for t in range(epochs):
        recs = er.lib_epoch_events(L, network, scheme, code, burst, seed, t, rw, rt)
        if restate:
            for key, mine in er.epoch_events(network, scheme, code, burst, seed, t, rw, rt, ge.small).items():
                assert mine.shape == recs[key].shape and (mine == recs[key]).all(), (t, key)
                recs[key] = mine
        out.append(recs)
    return out


def redundant_layers(network, scheme, code):
    return [l for l in range(len(hr.params_io.layout(network))) if er.org(network, scheme, code, l)[0] == 3 or er.org(network, scheme, code, l)[1] > 1]


@pytest.mark.parametrize("network,scheme,code", [("cnvW1A1", 1, 0), ("cnvW1A1", 2, 1), ("cnvW1A2", 0, 1), ("lfcW1A1", 0, 1)], ids=str)
def test_repair_every_0_is_the_coded_exposure_campaign(network, scheme, code, tmp_path, monkeypatch):
    """2^-5, burst 2, epochs of 12, scrub_every 2: classes, seeds, the six counts and the blob of every epoch equal
    ecc_exposure_campaigns' / ecc_exposure_params' bit for bit; the two repair counts are 0; the coded entry point's last_*
    state is not this one's"""
    L, pdir = gm.load(network, DATASET[network])
    path = sw.write_images(network, sw.images(network, N, seed=17), tmp_path)
    monkeypatch.setenv("BNN_MI355X_NOISE_GROUP", "37")
    rw, rt = rates_of(network, 2.0 ** -5)
    want, wcounts, wseeds = ge.ecampaign(L, path, scheme, code, 2, RUNS, SEED, rw, rt, 12, 2)
    got, counts, seeds = rcampaign(L, path, scheme, code, 2, RUNS, SEED + 1, rw, rt, 12, 2, 0)  # (another seed: the states are apart)
    s = (C.c_ulonglong * RUNS)()
    L.bnn_mi355x_last_ecc_exposure_seeds(s, RUNS)
    assert list(s) == wseeds and seeds == [SEED + 1 + r for r in range(RUNS)]
    got, counts, seeds = rcampaign(L, path, scheme, code, 2, RUNS, SEED, rw, rt, 12, 2, 0)
    assert seeds == wseeds and got.tolist() == want.tolist()
    assert counts[..., :6].tolist() == wcounts.tolist() and (counts[..., 6:] == 0).all()
    assert wcounts[..., 0].sum() > 0 and (want != gm.clean_classes(L, path)[None]).any()
    for r in range(RUNS):
        for t in range(4):
            gm.assert_same_bytes(rdevice_blob(L, scheme, code, 2, SEED + r, rw, rt, t, 2, 0), ge.edevice_blob(L, scheme, code, 2, SEED + r, rw, rt, t, 2),
                                 "%s scheme %d code %d run %d epoch %d" % (network, scheme, code, r, t))


@pytest.mark.parametrize("network,scheme,code", [("cnvW1A1", 0, 0), ("cnvW1A1", 3, 0), ("cnvW1A2", 2, 0), ("lfcW1A1", 0, 0)], ids=str)
def test_without_redundancy_a_repair_is_a_no_op(network, scheme, code, tmp_path, monkeypatch):
    """a (scheme, code) without redundancy at 2^-3: repair_every 1 gives repair_every 0's classes, counts and blobs, the
    two repair counts all zero"""
    L, pdir = gm.load(network, DATASET[network])
    path = sw.write_images(network, sw.images(network, N, seed=18), tmp_path)
    monkeypatch.setenv("BNN_MI355X_NOISE_GROUP", "37")
    rw, rt = rates_of(network, 2.0 ** -3)
    assert redundant_layers(network, scheme, code) == []
    a = rcampaign(L, path, scheme, code, 1, RUNS, SEED, rw, rt, 10, 0, 0)
    b = rcampaign(L, path, scheme, code, 1, RUNS, SEED, rw, rt, 10, 0, 1)
    assert a[0].tolist() == b[0].tolist() and a[1].tolist() == b[1].tolist() and (b[1][..., 6:] == 0).all() and b[1][..., 1].sum() > 0
    for t in (1, 4):
        gm.assert_same_bytes(rdevice_blob(L, scheme, code, 1, SEED, rw, rt, t, 0, 1), rdevice_blob(L, scheme, code, 1, SEED, rw, rt, t, 0, 0), str(t))


@pytest.mark.parametrize("network,scheme,code,burst,zero0", CASES, ids=str)
def test_repairs(network, scheme, code, burst, zero0, tmp_path, monkeypatch):
    """both rates, the three schedules, epochs of 12 and of 10 images: for every run and epoch the device's blob is
    pack_params_repair of the marker-and-mask stream of epochs 0 ... t, byte for byte; the epoch's classes are those of
    that blob in a second library handle; the eight counts are repair_ref's; another grouping of the pairs changes
    nothing.  Before any device result is looked at, the cases only a correct repair gets right are asserted present at
    2^-3 from the plain-Python restatement alone"""
    L, pdir = gm.load(network, DATASET[network])
    L2 = gl.load(network, "python_hw")  # a second handle: importing a blob drops the raw memories the campaign draws in
    imgs = sw.images(network, N, seed=23)
    path = sw.write_images(network, imgs, tmp_path)
    clean_cls = gm.clean_classes(L, path)
    crc = L.bnn_mi355x_params_crc()
    red = redundant_layers(network, scheme, code)
    assert red and (0 in red) == (scheme == 1 or network.startswith("lfc"))
    changed = 0
    for p in RATES:
        rw, rt = rates_of(network, p, zero0)
        runs_epochs = [drawn_epochs(L, network, scheme, code, burst, SEED + r, rw, rt, p == RATES[0]) for r in range(RUNS)]
        base = {}
        for every, repair in SCHEDULES:
            what = "%s scheme %d code %d burst %d rate %g scrub every %d repair every %d" % (network, scheme, code, burst, p, every, repair)
            for r in range(RUNS):  # (the counts of the memories a repair never touches: once per rewrite interval)
                if (r, every) not in base and every and (r, 0) in base:  # (one rewrite, before epoch `every`: from there on a fresh start)
                    assert every < T_MAX <= 2 * every
                    base[(r, every)] = np.concatenate([base[(r, 0)][:every], rr.base_counts(network, scheme, code, pdir, runs_epochs[r][every:], 0)])
                if (r, every) not in base:
                    base[(r, every)] = rr.base_counts(network, scheme, code, pdir, runs_epochs[r], every)
            ref = [rr.campaign_counts(network, scheme, code, pdir, runs_epochs[r], every, repair, base[(r, every)]) for r in range(RUNS)]
            want_counts = np.array([c for c, _ in ref])
            if p == RATES[0] and (every, repair) == (0, 1):  # what the chosen seeds hold, from the plain-Python draw alone
                flags = {k: any(f.get(k, False) for _, f in ref) for k in ("tmr_cleared", "tmr_locked", "coded_cleared", "coded_locked", "status2_hit_again")}
                if scheme == 1:
                    assert flags["tmr_cleared"] and flags["tmr_locked"], flags
                if code == 1:
                    assert flags["status2_hit_again"], flags
                    # (a burst of 4 too: under scheme 2 the check memory's clipped last group, 2 bits wide, is one bit of each of
                    # two code words)
                    assert flags["coded_cleared"] and flags["coded_locked"], flags
                if scheme == 2:  # a pair whose partner line takes events in a later epoch
                    assert all(any(er.reaches_partner(scheme, e[(l, 1, m)]) for pe in runs_epochs for e in pe[1:4] for m in (0, 1)) for l in red)
                assert (want_counts[..., 6].sum(axis=(0, 1))[red] > 0).all() and (want_counts[..., 7].sum(axis=(0, 1))[red] > 0).all()
                assert (want_counts[:, 0, :, 6:] == 0).all()
            not_red = [l for l in range(want_counts.shape[2]) if l not in red]
            assert (want_counts[:, :, not_red, 6:] == 0).all()
            classes = []
            for r in range(RUNS):
                classes.append([])
                for t in range(T_MAX):
                    blob = rr.lib_pack(L, pdir, scheme, code, rr.stream(runs_epochs[r], t, every, repair))
                    gm.assert_same_bytes(rdevice_blob(L, scheme, code, burst, SEED + r, rw, rt, t, every, repair), blob, what + " run %d epoch %d" % (r, t))
                    classes[-1].append(gm.classify_with_blob(L2, blob, imgs))
            for ei in EPOCH_IMAGES:
                E = -(-N // ei)
                monkeypatch.setenv("BNN_MI355X_NOISE_GROUP", "37")
                got, counts, seeds = rcampaign(L, path, scheme, code, burst, RUNS, SEED, rw, rt, ei, every, repair)
                assert seeds == [SEED + r for r in range(RUNS)]
                assert counts.tolist() == want_counts[:, :E].tolist(), what
                if (every, repair) == (0, 1):
                    monkeypatch.setenv("BNN_MI355X_NOISE_GROUP", "1000")
                    g2, c2, _ = rcampaign(L, path, scheme, code, burst, RUNS, SEED, rw, rt, ei, every, repair)
                    assert g2.tolist() == got.tolist() and c2.tolist() == counts.tolist(), what
                for r in range(RUNS):
                    for t in range(E):
                        want = classes[r][t][t * ei: (t + 1) * ei]
                        assert got[r, t * ei: (t + 1) * ei].tolist() == want.tolist(), what + " run %d epoch %d of %d images" % (r, t, ei)
                        changed += int((want != clean_cls[t * ei: (t + 1) * ei]).sum())
    assert changed > 0 and L.bnn_mi355x_params_crc() == crc
    assert gm.clean_classes(L, path).tolist() == clean_cls.tolist()


def test_rate_0_refusals_and_side_effects(tmp_path):
    """all rates 0: the fault-free classes once per run, all counts 0, the parameters read back are the loaded ones (no
    kernel has anything to do); the loaded parameters (params_crc, the classes they give) and the last_* state of the
    exposure and coded entry points are unchanged after every call.  Refusals, with a device present, return NULL / 0 with
    a reason and leave no counts"""
    network = "cnvW1A2"
    L, pdir = gm.load(network, "cifar10")
    path = sw.write_images(network, sw.images(network, N, seed=4), tmp_path)
    clean = gm.clean_classes(L, path)
    crc = L.bnn_mi355x_params_crc()
    z = [0] * 9
    rw, rt = rates_of(network, 2.0 ** -8)
    exposure = gx.xcampaign(L, path, 1, 1, 2, 11, rw, rt, 12, 0)[1:]
    coded = ge.ecampaign(L, path, 2, 1, 1, 2, 12, rw, rt, 12, 0)[1:]

    def untouched():
        assert L.bnn_mi355x_params_crc() == crc and gm.clean_classes(L, path).tolist() == clean.tolist()
        for counts, seeds, want in ((L.bnn_mi355x_last_exposure_counts, L.bnn_mi355x_last_exposure_seeds, exposure),
                                    (L.bnn_mi355x_last_ecc_exposure_counts, L.bnn_mi355x_last_ecc_exposure_seeds, coded)):
            k = counts(None, 0)
            c = (C.c_long * k)()
            counts(c, k)
            s = (C.c_ulonglong * 2)()
            assert seeds(s, 2) == 2
            assert list(c) == want[0].reshape(-1).tolist() and list(s) == want[1]

    for scheme, code, burst, ei, every, repair in ((1, 0, 1, 12, 0, 1), (2, 1, 4, 10, 3, 1), (0, 1, 16, 100, 0, 2), (3, 0, 2, 12, 0, 1)):
        got, counts, _ = rcampaign(L, path, scheme, code, burst, RUNS, 5, z, z, ei, every, repair)
        assert (got == clean[None]).all() and (counts == 0).all() and counts.shape[1] == -(-N // ei)
        assert (rdevice_blob(L, scheme, code, burst, 5, z, z, 3, every, repair) == gl.pack_params(network, pdir)).all()
        untouched()
    got, counts, _ = rcampaign(L, path, 1, 0, 4, RUNS, 5, rw, rt, 12, 0, 1)
    assert counts[..., 2].sum() > 0
    untouched()
    up = C.c_uint * 9
    call = lambda scheme, code, burst, ei, every, repair: L.bnn_mi355x_repair_exposure_campaigns(path.encode(), 10, scheme, code, burst, 1, 1, up(*rw),
                                                                                                up(*rt), 9, ei, every, repair, None, None)
    for scheme, code, reason in ((1, 1, b"TMR plus a code is not modelled"), (3, 1, b"resilient patterns are defined for 32 and 48 positions only"),
                                 (0, 2, b"code must be 0 (none) or 1 (SEC-DED)"), (4, 1, b"scheme must be")):
        assert not call(scheme, code, 1, 12, 0, 1)
        assert reason in L.bnn_mi355x_last_error()
        assert L.bnn_mi355x_last_repair_exposure_counts(None, 0) == 0 and L.bnn_mi355x_last_repair_exposure_seeds(None, 0) == 0
        assert L.bnn_mi355x_repair_exposure_params(scheme, code, 1, 1, up(*rw), up(*rt), 9, 1, 0, 1, None, 0) == 0
        assert reason in L.bnn_mi355x_last_error()
    assert not call(1, 0, 1, 12, 0, -1)
    assert b"repair_every must not be negative" in L.bnn_mi355x_last_error()
    assert L.bnn_mi355x_repair_exposure_params(1, 0, 1, 1, up(*rw), up(*rt), 9, 1, 0, -1, None, 0) == 0
    assert b"repair_every must not be negative" in L.bnn_mi355x_last_error()
    for ei, every in ((0, 0), (-1, 0), (12, -1)):
        assert not call(2, 1, 1, ei, every, 1)
        assert b"epoch_images must be at least 1" in L.bnn_mi355x_last_error()
    assert not call(2, 1, 17, 12, 0, 1)
    assert b"burst" in L.bnn_mi355x_last_error()
    big = tmp_path / "sparse.bin"  # 2^15 epochs x 1024 runs x 9 layers x 8 counters: refused from the file's size alone (a sparse file)
    with open(big, "wb") as f:
        f.truncate((1 << 15) * 3073)
    assert not L.bnn_mi355x_repair_exposure_campaigns(str(big).encode(), 10, 1, 0, 1, 1024, 1, up(*rw), up(*rt), 9, 1, 0, 1, None, None)
    assert b"layers * 8 counters must stay below 2^31" in L.bnn_mi355x_last_error()
    untouched()
    W = gm.load("cnvW2A2", "cifar10")[0]
    assert not W.bnn_mi355x_repair_exposure_campaigns(path.encode(), 10, 2, 1, 1, 1, 1, up(*rw), up(*rt), 9, 12, 0, 1, None, None)
    assert b"cnvW2A2 with scheme 2" in W.bnn_mi355x_last_error()
    blob = gl.pack_params(network, pdir)
    assert L.bnn_mi355x_import_params(blob.ctypes.data, len(blob)) == 0
    assert not call(1, 0, 1, 12, 0, 1)
    assert b"imported blob" in L.bnn_mi355x_last_error()
    L.load_parameters(pdir.encode())


def test_variant_library_runs_the_same_campaign(variant_libs, tmp_path):
    """cnvW1A1-TMR's library gives the classes, counts and blobs of the base network's library for the scheme its name
    implies, with a repair every epoch"""
    network = "cnvW1A1"
    L, pdir = gm.load(network, "cifar10")
    V = gl.load("cnvW1A1-TMR")
    V.load_parameters(pdir.encode())
    assert V.bnn_mi355x_last_error() == b""
    path = sw.write_images(network, sw.images(network, N, seed=6), tmp_path)
    rw, rt = rates_of(network, 2.0 ** -3)
    scheme = V.bnn_mi355x_hardening_scheme()
    assert scheme == 1
    a = rcampaign(V, path, scheme, 0, 1, RUNS, 9, rw, rt, 10, 3, 1)
    b = rcampaign(L, path, scheme, 0, 1, RUNS, 9, rw, rt, 10, 3, 1)
    assert a[0].tolist() == b[0].tolist() and a[1].tolist() == b[1].tolist() and a[1][..., 6].sum() > 0 and a[1][..., 7].sum() > 0
    assert (rdevice_blob(V, scheme, 0, 1, 9, rw, rt, 4, 3, 1) == rdevice_blob(L, scheme, 0, 1, 9, rw, rt, 4, 3, 1)).all()


def test_python_interface(tmp_path):
    """FaultTest.run_exposure_test(..., repair_every=1) on 40 images in epochs of 16 (the last one short) returns what the
    C call returns; with repair_every 0 it keeps its entry points; NetworkTest.scrubbing_curve accepts (scrub_every,
    repair_every) pairs next to plain intervals, and only a non-zero repair_every changes a result's name ((1, 0) is
    "scrub every 1")"""
    from bnn.faults import faults
    network, dataset = "cnvW1A1", "cifar10"
    L, pdir = gm.load(network, dataset)
    n, runs, seed, ei = 40, 3, 77, 16
    imgs = sw.images(network, n, seed=21)
    path = sw.write_images(network, imgs, tmp_path, network)
    labels = gm.clean_classes(L, path).tolist()
    labels[0] = (labels[0] + 1) % 10
    ft = faults.CNVFaultTest(network, dataset, path, labels)
    rw, rt = gm.rates(network, 2.0 ** -7, 2.0 ** -3)
    lab = np.array(labels)
    for scheme, code in ((1, 0), (2, 1)):
        acc, cnts = ft.run_exposure_test(runs, 2.0 ** -7, 2.0 ** -3, ei, scrub_every=2, scheme=scheme, burst=1, seed=seed, code=code, repair_every=1)
        got, counts, _ = rcampaign(L, path, scheme, code, 1, runs, seed, rw, rt, ei, 2, 1)
        assert ft.exposure_results.tolist() == got.tolist() and cnts.tolist() == counts.tolist() and cnts.shape == (runs, 3, 9, 8)
        assert cnts[:, 1, :, 6].sum() > 0 and (cnts[:, (0, 2), :, 6:] == 0).all()  # (epoch 1 is repaired, epoch 2 rewritten)
        assert acc == [[100.0 * (row[i: i + ei] == lab[i: i + ei]).sum() / len(lab[i: i + ei]) for i in range(0, n, ei)] for row in got]
    _, coded = ft.run_exposure_test(runs, 2.0 ** -7, 2.0 ** -3, ei, scrub_every=2, scheme=2, burst=1, seed=seed, code=1)
    assert coded.shape == (runs, 3, 9, 6) and coded.tolist() == ge.ecampaign(L, path, 2, 1, 1, runs, seed, rw, rt, ei, 2)[1].tolist()
    _, plain = ft.run_exposure_test(runs, 2.0 ** -7, 2.0 ** -3, ei, scrub_every=2, scheme=1, burst=1, seed=seed, repair_every=0)
    assert plain.shape == (runs, 3, 9, 2, 2) and plain.tolist() == gx.xcampaign(L, path, 1, 1, runs, seed, rw, rt, ei, 2)[1].tolist()
    nt = faults.NetworkTest(ft)
    nt.scrubbing_curve(str(tmp_path / "out"), 2, [2.0 ** -3], [0, (1, 0), (0, 1), (2, 1)], [1, (2, 1)], ei, bursts=[1], seed=5)
    with open(tmp_path / "out" / network / dataset / "scrubbing" / ("%s_%s_scrubbing_stats.json" % (network, dataset))) as f:
        doc = json.load(f)
    assert len(doc["results"]) == 2 * 4
    for name in ("TMR", "interleaved + SEC-DED"):
        never = doc["results"]["%s burst 1 upset rate %g scrub every 0" % (name, 2.0 ** -3)]
        rewrite = doc["results"]["%s burst 1 upset rate %g scrub every 1" % (name, 2.0 ** -3)]
        repair = doc["results"]["%s burst 1 upset rate %g scrub every 0 repair every 1" % (name, 2.0 ** -3)]
        both = doc["results"]["%s burst 1 upset rate %g scrub every 2 repair every 1" % (name, 2.0 ** -3)]
        assert "repair every" not in never and "repair every" not in rewrite and repair["repair every"] == 1 and both["scrub every"] == 2
        assert len(repair["repaired words per epoch"]) == 3 and repair["repaired words per epoch"][0] == 0 and repair["repaired words per epoch"][1] > 0
        assert both["repaired words per epoch"][2] == 0 and len(repair["logical bits per epoch"]) == 3
        assert ("code" in repair) == (name != "TMR") and repair["physical bits"] == never["physical bits"]
        # a repair repairs less than a rewrite (the weights keep their upsets); under TMR it repairs more than nothing (a word
        # is lost where two modules are hit between two repairs, not over the whole run; with the code, at this rate, most
        # words hold more errors than it corrects either way): the logical bits after the last epoch
        assert rewrite["logical bits per epoch"][2] < min(repair["logical bits per epoch"][2], never["logical bits per epoch"][2])
        if name == "TMR":
            assert repair["logical bits per epoch"][2] < never["logical bits per epoch"][2]
