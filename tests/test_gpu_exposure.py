"""Exposure campaigns on the GPU (bnn_mi355x_exposure_campaigns): memory upsets that accumulate over epochs of images on
the PHYSICAL state of a hardened memory organisation, with scrubbing.  All checks are exact.

The model is pinned on the host: bnn_mi355x_exposure_mask lists an epoch's events (tests/test_exposure_mask.py),
bnn_mi355x_pack_params_hardened applies any ordered list of physical records (tests/test_hardened_mem_noise.py).  The
blob of (run, epoch t) must be pack_params_hardened of the masks of the epochs since the last scrub, concatenated;
bnn_mi355x_exposure_params reads back the very blob the device classifies that epoch with, and the epoch's classes are
compared with import_params(blob) + inference_buffer in a second library handle.

3 runs x 48 images, rates 2^-3 and 2^-8 per epoch on every memory, epochs of 12 images (4 epochs) and of 10 (5, the last
one short).  At 2^-3 the cases only accumulation gets right are there BY CONSTRUCTION: the tests first assert them from
the plain-Python restatement of the draw (tests/exposure_ref.py), before any device result is looked at -- for run 0
of every memory, for runs 1 and 2 (to keep the tests quick) of layer 0 and the threshold memories, which are the ones a
scheme replicates or interleaves; the other memories' masks are the library's there."""
import ctypes as C
import faulthandler
import json
import os
import struct

import numpy as np
import pytest

import exposure_ref as xr
import gpu_lib as gl
import hardened_ref as hr
import test_gpu_act_fault_sweep as sw
import test_gpu_hardened_mem_noise as gh
import test_gpu_mem_noise as gm
import test_mem_noise_mask as mm

pytestmark = pytest.mark.gpu
q32 = hr.q32
RUNS, N, SEED = 3, 48, 20261018
RATES = (2.0 ** -3, 2.0 ** -8)
EPOCH_IMAGES = (12, 10)
T_MAX = 5  # epochs of the longer configuration: ceil(48 / 10)
PAIRS = gh.PAIRS
DATASET = dict(mm.NETS)


@pytest.fixture(autouse=True)
def _time_limit():
    """every test runs in this process under a limit of its own (a case takes a few seconds): a device call that hangs
    ends the process with a traceback, and nothing more is started on the card"""
    faulthandler.dump_traceback_later(180, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def xcampaign(L, path, scheme, burst, runs, seed, rw, rt, epoch_images, scrub_every=0, ncls=10):
    """-> (classes [runs, n], counts [runs, epochs, layers, 2: weights, thresholds, 2: physical, logical], seeds [runs])"""
    up = C.c_uint * len(rw)
    cnt, usec = C.c_int(0), C.c_float(0)
    p = L.bnn_mi355x_exposure_campaigns(path.encode(), ncls, scheme, burst, runs, seed, up(*rw), up(*rt), len(rw), epoch_images, scrub_every,
                                        C.byref(cnt), C.byref(usec))
    assert p, L.bnn_mi355x_last_error().decode()
    n = cnt.value
    got = np.ctypeslib.as_array(p, shape=(max(runs * n, 1),))[: runs * n].copy().reshape(runs, n)
    L.free_results(p)
    epochs = -(-n // epoch_images)
    k = L.bnn_mi355x_last_exposure_counts(None, 0)
    assert k == runs * epochs * len(rw) * 4
    c = (C.c_long * k)()
    assert L.bnn_mi355x_last_exposure_counts(c, k) == k
    s = (C.c_ulonglong * runs)()
    assert L.bnn_mi355x_last_exposure_seeds(s, runs) == runs
    return got, np.array(c[:], np.int64).reshape(runs, epochs, len(rw), 2, 2), list(s)


def xdevice_blob(L, scheme, burst, seed, rw, rt, epoch, scrub_every=0):
    up = C.c_uint * len(rw)
    size = L.bnn_mi355x_exposure_params(scheme, burst, seed, up(*rw), up(*rt), len(rw), epoch, scrub_every, None, 0)
    assert size > 0, L.bnn_mi355x_last_error().decode()
    blob = np.zeros(size, np.uint8)
    assert L.bnn_mi355x_exposure_params(scheme, burst, seed, up(*rw), up(*rt), len(rw), epoch, scrub_every, blob.ctypes.data, size) == size
    return blob


def rates_of(network, p):
    return gm.rates(network, p, p)


def drawn_epochs(L, network, scheme, burst, seed, rw, rt, restate):
    """a run's masks of epochs 0 ... T_MAX - 1, each {(layer, target, module): records} in the in-epoch order, from the
    library.  restate "all" / "small": the plain-Python draw of all memories / of the replicated and interleaved ones and
    layer 0 (exposure_ref.small) takes their place, after the library's were found equal"""
    out = []
    for t in range(T_MAX):
        recs = xr.lib_epoch_events(L, network, scheme, burst, seed, t, rw, rt)
        if restate:
            for key, mine in xr.epoch_events(network, scheme, burst, seed, t, rw, rt, None if restate == "all" else xr.small).items():
                assert mine.shape == recs[key].shape and (mine == recs[key]).all(), (t, key)
                recs[key] = mine
        out.append(recs)
    return out


def assert_accumulation_preconditions(network, scheme, burst, per_epoch, epochs, only=None):
    """at 2^-3, from the restatement's events of epochs 0 ... epochs - 1 alone (only: the memories restated):
    - every replicated memory has a bit that ends up set in two modules' states which were hit in different epochs and in
      no single epoch together: a draw that starts every epoch from the loaded words never outvotes it;
    - every memory (of those restated: `only`) has a bit hit twice in one module: the XOR cancels it;
    - every interleaved layer has an event that reaches the partner line's element in an epoch later than 0."""
    lay = hr.params_io.layout(network)
    for layer in range(len(lay)):
        for target in (0, 1):
            if hr.ebits(network, layer, target) == 0 or (only and not only(layer, target)):
                continue
            mods = hr.org(network, scheme, layer)[target]
            assert any((xr.hit_counts(network, per_epoch[:epochs], layer, target, m) >= 2).any() for m in range(mods)), (layer, target)
            if mods == 3:
                voted = xr.state(network, per_epoch[:epochs], layer, target, 3)
                together = sum(sum((xr.hit_counts(network, [e], layer, target, m) > 0).astype(np.int64) for m in range(3)) >= 2 for e in per_epoch[:epochs])
                assert ((voted > 0) & (together == 0)).any(), (layer, target)
        il = hr.org(network, scheme, layer)[2]
        if il:
            T = hr.ebits(network, layer, 1)
            tab = hr.pair_table(il, T)
            reach = False
            for e in per_epoch[1:epochs]:
                for _, t, l, mem, ind, thresh, bit, ws, module in e[(layer, 1, 0)].tolist():
                    q0 = bit + (T if ind % 2 == 0 else 0)
                    lines = {tab[q][0] for q in range(q0, min(q0 + ws, (q0 // T + 1) * T))}
                    reach = reach or (lines == {0, 1} if burst > 1 else lines == {1 - ind % 2})
            assert reach, layer


@pytest.mark.parametrize("network,scheme", [(n, 0) for n, _ in mm.NETS] + PAIRS, ids=str)
def test_one_epoch_is_the_hardened_campaign(network, scheme, tmp_path, monkeypatch):
    """epoch_images >= n, bursts 1 and 4, both rates: classes, seeds, counts and the blob of epoch 0 equal
    hardened_mem_noise_campaigns / _params bit for bit (scrub_every has nothing to act on).  Both entry points run the same
    device path: this pins the hardened entry point's argument mapping (the whole file as one epoch, never scrubbed)"""
    L, pdir = gm.load(network, DATASET[network])
    path = sw.write_images(network, sw.images(network, N, seed=17), tmp_path)
    monkeypatch.setenv("BNN_MI355X_NOISE_GROUP", "37")
    changed = 0
    for burst in (1, 4):
        for p in RATES:
            rw, rt = rates_of(network, p)
            what = "%s scheme %d burst %d rate %g" % (network, scheme, burst, p)
            want, wcounts, wseeds = gh.hcampaign(L, path, scheme, burst, RUNS, SEED, rw, rt)
            for ei, every in ((N, 0), (N + 100, 1)):
                got, counts, seeds = xcampaign(L, path, scheme, burst, RUNS, SEED, rw, rt, ei, every)
                assert seeds == wseeds and got.tolist() == want.tolist(), what
                assert counts.shape[1] == 1 and counts[:, 0].tolist() == wcounts.tolist(), what
            assert wcounts[..., 0].sum() > 0
            for r in range(RUNS):
                gm.assert_same_bytes(xdevice_blob(L, scheme, burst, SEED + r, rw, rt, 0), gh.hdevice_blob(L, scheme, burst, SEED + r, rw, rt),
                                     what + " run %d" % r)
            changed += int((want != gm.clean_classes(L, path)[None]).sum())
    assert changed > 0


@pytest.mark.parametrize("network,scheme,burst", [(n, s, b) for n, s in PAIRS + [("lfcW1A1", 0)] for b in (1, 4)], ids=str)
def test_accumulation(network, scheme, burst, tmp_path, monkeypatch):
    """scrub_every 0, both rates, epochs of 12 and of 10 images: for every run and epoch the device's blob is
    pack_params_hardened of the masks of epochs 0 ... t concatenated, byte for byte; the epoch's classes are those of that
    blob in a second library handle; both counts are what the masks imply; another grouping of the pairs changes nothing"""
    L, pdir = gm.load(network, DATASET[network])
    L2 = gl.load(network, "python_hw")  # a second handle: importing a blob drops the raw memories the campaign draws in
    imgs = sw.images(network, N, seed=23)
    path = sw.write_images(network, imgs, tmp_path)
    clean_cls = gm.clean_classes(L, path)
    crc = L.bnn_mi355x_params_crc()
    changed = 0
    for p in RATES:
        rw, rt = rates_of(network, p)
        what = "%s scheme %d burst %d rate %g" % (network, scheme, burst, p)
        classes, want_counts = [], []
        for r in range(RUNS):
            # (2^-3: every memory restated for run 0; for the other runs the replicated and interleaved ones and layer 0)
            restate = ("all" if r == 0 else "small") if p == RATES[0] else None
            per_epoch = drawn_epochs(L, network, scheme, burst, SEED + r, rw, rt, restate)
            if restate:
                for ei in EPOCH_IMAGES:
                    assert_accumulation_preconditions(network, scheme, burst, per_epoch, -(-N // ei), None if r == 0 else xr.small)
            classes.append([])
            want_counts.append([])
            for t in range(T_MAX):
                blob = hr.pack_hardened(L, pdir, scheme, xr.since_scrub(per_epoch, t, 0))
                gm.assert_same_bytes(xdevice_blob(L, scheme, burst, SEED + r, rw, rt, t), blob, what + " run %d epoch %d" % (r, t))
                classes[-1].append(gm.classify_with_blob(L2, blob, imgs))
                want_counts[-1].append(xr.implied_counts(network, scheme, pdir, per_epoch, t, 0))
        want_counts = np.array(want_counts)
        for ei in EPOCH_IMAGES:
            E = -(-N // ei)
            monkeypatch.setenv("BNN_MI355X_NOISE_GROUP", "37")
            got, counts, seeds = xcampaign(L, path, scheme, burst, RUNS, SEED, rw, rt, ei)
            assert seeds == [SEED + r for r in range(RUNS)]
            assert counts.tolist() == want_counts[:, :E].tolist(), what
            monkeypatch.setenv("BNN_MI355X_NOISE_GROUP", "1000")
            g2, c2, _ = xcampaign(L, path, scheme, burst, RUNS, SEED, rw, rt, ei)
            assert g2.tolist() == got.tolist() and c2.tolist() == counts.tolist(), what
            for r in range(RUNS):
                for t in range(E):
                    want = classes[r][t][t * ei: (t + 1) * ei]
                    assert got[r, t * ei: (t + 1) * ei].tolist() == want.tolist(), what + " run %d epoch %d of %d images" % (r, t, ei)
                    changed += int((want != clean_cls[t * ei: (t + 1) * ei]).sum())
        # the state grows: more logical bits differ after the last epoch than after the first
        assert (want_counts[:, T_MAX - 1, :, :, 1].sum(axis=(1, 2)) > want_counts[:, 0, :, :, 1].sum(axis=(1, 2))).all()
    assert changed > 0 and L.bnn_mi355x_params_crc() == crc
    assert gm.clean_classes(L, path).tolist() == clean_cls.tolist()


@pytest.mark.parametrize("network,scheme,burst", [("cnvW1A1", 1, 1), ("cnvW1A1", 2, 4), ("cnvW1A2", 3, 1), ("cnvW2A2", 1, 4), ("lfcW1A1", 0, 1)], ids=str)
def test_scrubbing(network, scheme, burst, tmp_path, monkeypatch):
    """4 epochs of 12 images at 2^-3.  scrub_every 1: every epoch's blob is pack_params_hardened of that epoch's masks
    alone.  scrub_every 2: epochs 0-1 are the unscrubbed run's, epoch 2 a fresh exposure with epoch 2's draw, epoch 3
    epochs 2 + 3 accumulated; fewer logical bits differ after epoch 2 than without the scrub.  The campaign's classes and
    counts follow the same blobs and masks."""
    L, pdir = gm.load(network, DATASET[network])
    L2 = gl.load(network, "python_hw")
    imgs = sw.images(network, N, seed=29)
    path = sw.write_images(network, imgs, tmp_path)
    ei, E = 12, 4
    rw, rt = rates_of(network, RATES[0])
    monkeypatch.setenv("BNN_MI355X_NOISE_GROUP", "37")
    per_epoch = [[xr.lib_epoch_events(L, network, scheme, burst, SEED + r, t, rw, rt) for t in range(E)] for r in range(RUNS)]
    implied = {every: np.array([[xr.implied_counts(network, scheme, pdir, per_epoch[r], t, every) for t in range(E)] for r in range(RUNS)])
               for every in (0, 1, 2)}
    # (from the masks) the scrub before epoch 2 takes logical bits away, in every run
    assert (implied[2][:, 2, :, :, 1].sum(axis=(1, 2)) < implied[0][:, 2, :, :, 1].sum(axis=(1, 2))).all()
    for every in (1, 2):
        what = "%s scheme %d burst %d scrub every %d" % (network, scheme, burst, every)
        got, counts, _ = xcampaign(L, path, scheme, burst, RUNS, SEED, rw, rt, ei, every)
        assert counts.tolist() == implied[every].tolist(), what
        for r in range(RUNS):
            for t in range(E):
                first = xr.first_epoch(t, every)
                assert first == (t if every == 1 else (0, 0, 2, 2)[t])
                blob = hr.pack_hardened(L, pdir, scheme, xr.since_scrub(per_epoch[r], t, every))
                dev = xdevice_blob(L, scheme, burst, SEED + r, rw, rt, t, every)
                gm.assert_same_bytes(dev, blob, what + " run %d epoch %d" % (r, t))
                if every == 2 and t < 2:
                    assert (dev == xdevice_blob(L, scheme, burst, SEED + r, rw, rt, t, 0)).all()
                want = gm.classify_with_blob(L2, blob, imgs)[t * ei: (t + 1) * ei]
                assert got[r, t * ei: (t + 1) * ei].tolist() == want.tolist(), what + " run %d epoch %d" % (r, t)
    unscrubbed = xcampaign(L, path, scheme, burst, RUNS, SEED, rw, rt, ei, 0)[1]
    scrubbed = xcampaign(L, path, scheme, burst, RUNS, SEED, rw, rt, ei, 2)[1]
    assert (scrubbed[:, 2, :, :, 1].sum(axis=(1, 2)) < unscrubbed[:, 2, :, :, 1].sum(axis=(1, 2))).all()
    assert scrubbed[:, :2].tolist() == unscrubbed[:, :2].tolist()


@pytest.mark.parametrize("scheme", [0, 1])
def test_sparse_layer_0_events_with_scrubbing(scheme, tmp_path):
    """layer 0 of cnvW1A1 alone at 2^-12 per epoch (the host's part: a handful of events per epoch, some epochs none), 8
    epochs of 6 images, scrub_every 0, 2 and 3: blobs, classes and counts as elsewhere.  This is where a row RETURNS to the
    loaded words and must be patched back, where an epoch without events carries the logical counts over, and where a
    scrub meets an epoch without events.  Scheme 0: asserted first from the masks and the host's blobs, for the seed chosen
    on the CPU for it."""
    network, seed, runs, ei, E = "cnvW1A1", 234, 2, 6, 8
    L, pdir = gm.load(network, "cifar10")
    L2 = gl.load(network, "python_hw")
    imgs = sw.images(network, N, seed=31)
    path = sw.write_images(network, imgs, tmp_path)
    clean = gl.pack_params(network, pdir)
    off, rd, rows, kw = struct.unpack_from("<4I", clean, 32)
    differs = lambda blob: (blob[off: off + rows * rd * 4].reshape(rows, -1) != clean[off: off + rows * rd * 4].reshape(rows, -1)).any(axis=1)
    rate = q32(2.0 ** -12)
    rw, rt = [rate] + [0] * 8, [rate] + [0] * 8
    per_epoch = []
    for r in range(runs):
        per_epoch.append([xr.lib_epoch_events(L, network, scheme, 1, seed + r, t, rw, rt) for t in range(E)])
        for t in range(E):  # (the restatement of layer 0's draw)
            for key, mine in xr.epoch_events(network, scheme, 1, seed + r, t, rw, rt, lambda l, target: l == 0).items():
                assert (mine == per_epoch[r][t][key]).all()
    host = {every: [[hr.pack_hardened(L, pdir, scheme, xr.since_scrub(per_epoch[r], t, every)) for t in range(E)] for r in range(runs)]
            for every in (0, 2, 3)}
    if scheme == 0:
        events = [len(xr.flat(e)) for e in per_epoch[0]]
        rows_of = [differs(b) for b in host[0][0]]
        assert any((rows_of[t - 1] & ~rows_of[t]).any() for t in range(1, E)), "no row returns to the loaded words"
        assert any(events[t] == 0 and rows_of[t - 1].any() for t in range(1, E)), "no epoch without events behind a changed state"
        assert any(events[t] == 0 and differs(host[every][0][t - 1]).any() for every in (2, 3) for t in range(every, E, every)), \
            "no scrub that meets an epoch without events"
    for every in (0, 2, 3):
        what = "scheme %d scrub every %d" % (scheme, every)
        got, counts, _ = xcampaign(L, path, scheme, 1, runs, seed, rw, rt, ei, every)
        want_counts = [[xr.implied_counts(network, scheme, pdir, per_epoch[r], t, every) for t in range(E)] for r in range(runs)]
        assert counts.tolist() == np.array(want_counts).tolist(), what
        for r in range(runs):
            for t in range(E):
                gm.assert_same_bytes(xdevice_blob(L, scheme, 1, seed + r, rw, rt, t, every), host[every][r][t], what + " run %d epoch %d" % (r, t))
                want = gm.classify_with_blob(L2, host[every][r][t], imgs)[t * ei: (t + 1) * ei]
                assert got[r, t * ei: (t + 1) * ei].tolist() == want.tolist(), what + " run %d epoch %d" % (r, t)


def test_rate_0_refusals_and_side_effects(tmp_path):
    """all rates 0: the fault-free classes once per run, all counts 0, the parameters read back are the loaded ones; the
    loaded parameters (params_crc, the classes they give) and the last_* state of the hardened entry point are unchanged
    after every call.  Refusals return NULL / 0 with a reason: a bad epoch length or scrub interval, too many epochs or
    counters, an imported blob."""
    network = "cnvW1A2"
    L, pdir = gm.load(network, "cifar10")
    path = sw.write_images(network, sw.images(network, N, seed=4), tmp_path)
    clean = gm.clean_classes(L, path)
    crc = L.bnn_mi355x_params_crc()
    z = [0] * 9
    rw, rt = rates_of(network, 2.0 ** -8)
    hardened = gh.hcampaign(L, path, 1, 1, 2, 11, rw, rt)[1:]

    def untouched():
        assert L.bnn_mi355x_params_crc() == crc and gm.clean_classes(L, path).tolist() == clean.tolist()
        k = L.bnn_mi355x_last_hardened_mem_noise_counts(None, 0)
        c = (C.c_long * k)()
        L.bnn_mi355x_last_hardened_mem_noise_counts(c, k)
        s = (C.c_ulonglong * 2)()
        assert L.bnn_mi355x_last_hardened_mem_noise_seeds(s, 2) == 2
        assert list(c) == hardened[0].reshape(-1).tolist() and list(s) == hardened[1]

    for scheme, burst, ei, every in ((1, 1, 12, 0), (3, 4, 10, 2), (0, 16, 100, 1)):
        got, counts, _ = xcampaign(L, path, scheme, burst, RUNS, 5, z, z, ei, every)
        assert (got == clean[None]).all() and (counts == 0).all() and counts.shape[1] == -(-N // ei)
        assert (xdevice_blob(L, scheme, burst, 5, z, z, 3, every) == gl.pack_params(network, pdir)).all()
        untouched()
    got, counts, _ = xcampaign(L, path, 1, 4, RUNS, 5, rw, rt, 12, 2)
    assert counts[..., 0].sum() > 0
    untouched()
    up = C.c_uint * 9
    for ei, every in ((0, 0), (-1, 0), (12, -1)):
        assert not L.bnn_mi355x_exposure_campaigns(path.encode(), 10, 1, 1, 1, 1, up(*rw), up(*rt), 9, ei, every, None, None)
        assert b"epoch_images must be at least 1" in L.bnn_mi355x_last_error()
    assert not L.bnn_mi355x_exposure_campaigns(path.encode(), 10, 1, 17, 1, 1, up(*rw), up(*rt), 9, 12, 0, None, None)
    assert b"burst" in L.bnn_mi355x_last_error()
    assert L.bnn_mi355x_exposure_params(1, 1, 1, up(*rw), up(*rt), 9, xr.MAX_EPOCHS, 0, None, 0) == 0
    assert b"epoch must be" in L.bnn_mi355x_last_error()
    # too many epochs, or too many (run, epoch) counters: refused from the file's size alone (sparse files: nothing is read)
    for records, runs in ((xr.MAX_EPOCHS + 1, 1), ((1 << 31) // (4096 * 9 * 4) + 1, 4096)):
        big = tmp_path / ("sparse_%d.bin" % records)
        with open(big, "wb") as f:
            f.truncate(records * 3073)
        assert not L.bnn_mi355x_exposure_campaigns(str(big).encode(), 10, 1, 1, runs, 1, up(*rw), up(*rt), 9, 1, 0, None, None)
        assert b"epochs: at most 65536" in L.bnn_mi355x_last_error()
        assert L.bnn_mi355x_last_exposure_counts(None, 0) == 0
    untouched()
    blob = gl.pack_params(network, pdir)
    assert L.bnn_mi355x_import_params(blob.ctypes.data, len(blob)) == 0
    assert not L.bnn_mi355x_exposure_campaigns(path.encode(), 10, 1, 1, 1, 1, up(*rw), up(*rt), 9, 12, 0, None, None)
    assert b"imported blob" in L.bnn_mi355x_last_error()
    assert L.bnn_mi355x_exposure_params(1, 1, 1, up(*rw), up(*rt), 9, 1, 0, None, 0) == 0
    assert b"imported blob" in L.bnn_mi355x_last_error()
    L.load_parameters(pdir.encode())


def test_l1_comparison_forms_are_refused(tmp_path):
    """the BNN_MI355X_L1 comparison forms (cnvW1A1; read at load_parameters) are not wired to fault injection: both device
    entry points refuse them with the reason, as every parameter-fault entry point does"""
    network = "cnvW1A1"
    L, pdir = gm.load(network, "cifar10")
    path = sw.write_images(network, sw.images(network, 16, seed=8), tmp_path)
    rw, rt = rates_of(network, 2.0 ** -8)
    up = C.c_uint * 9
    try:
        for form in ("mfma", "lds"):
            os.environ["BNN_MI355X_L1"] = form
            L.load_parameters(pdir.encode())
            assert L.bnn_mi355x_last_error() == b""
            assert not L.bnn_mi355x_exposure_campaigns(path.encode(), 10, 1, 1, 2, 1, up(*rw), up(*rt), 9, 4, 0, None, None)
            assert b"BNN_MI355X_L1" in L.bnn_mi355x_last_error()
            assert L.bnn_mi355x_last_exposure_counts(None, 0) == 0
            assert L.bnn_mi355x_exposure_params(1, 1, 1, up(*rw), up(*rt), 9, 1, 0, None, 0) == 0
            assert b"BNN_MI355X_L1" in L.bnn_mi355x_last_error()
    finally:
        del os.environ["BNN_MI355X_L1"]
        L.load_parameters(pdir.encode())
    got, counts, _ = xcampaign(L, path, 1, 1, 2, 1, rw, rt, 4, 0)
    assert counts[..., 0].sum() > 0


def test_variant_library_runs_the_same_campaign(variant_libs, tmp_path):
    """cnvW1A1-TMR's library gives the classes and counts of the base network's library for the scheme its name implies"""
    network = "cnvW1A1"
    L, pdir = gm.load(network, "cifar10")
    V = gl.load("cnvW1A1-TMR")
    V.load_parameters(pdir.encode())
    assert V.bnn_mi355x_last_error() == b""
    path = sw.write_images(network, sw.images(network, N, seed=6), tmp_path)
    rw, rt = rates_of(network, 2.0 ** -3)
    scheme = V.bnn_mi355x_hardening_scheme()
    assert scheme == 1
    a = xcampaign(V, path, scheme, 4, RUNS, 9, rw, rt, 10, 3)
    b = xcampaign(L, path, scheme, 4, RUNS, 9, rw, rt, 10, 3)
    assert a[0].tolist() == b[0].tolist() and a[1].tolist() == b[1].tolist() and a[1][..., 1].sum() > 0
    assert (xdevice_blob(V, scheme, 4, 9, rw, rt, 4, 3) == xdevice_blob(L, scheme, 4, 9, rw, rt, 4, 3)).all()


def test_python_interface(tmp_path):
    """FaultTest.run_exposure_test on 40 images in epochs of 16 (the last one short): accuracies [run][epoch] from the C
    call's classes, the counts the C call's; NetworkTest.scrubbing_curve writes one entry per (scheme, burst, rate, scrub
    interval) with the mean accuracy per epoch"""
    from bnn.faults import faults
    network, dataset = "cnvW1A1", "cifar10"
    L, pdir = gm.load(network, dataset)
    n, runs, seed, ei = 40, 3, 77, 16
    imgs = sw.images(network, n, seed=21)
    path = sw.write_images(network, imgs, tmp_path, network)
    labels = gm.clean_classes(L, path).tolist()
    labels[0] = (labels[0] + 1) % 10
    ft = faults.CNVFaultTest(network, dataset, path, labels)
    acc, cnts = ft.run_exposure_test(runs, 2.0 ** -7, 2.0 ** -3, ei, scrub_every=2, scheme=1, burst=4, seed=seed)
    rw, rt = gm.rates(network, 2.0 ** -7, 2.0 ** -3)
    got, counts, _ = xcampaign(L, path, 1, 4, runs, seed, rw, rt, ei, 2)
    assert ft.exposure_results.tolist() == got.tolist() and cnts.tolist() == counts.tolist() and cnts.shape == (runs, 3, 9, 2, 2)
    lab = np.array(labels)
    assert acc == [[100.0 * (row[i: i + ei] == lab[i: i + ei]).sum() / len(lab[i: i + ei]) for i in range(0, n, ei)] for row in got]
    nt = faults.NetworkTest(ft)
    nt.scrubbing_curve(str(tmp_path / "out"), 2, [0.0, 2.0 ** -3], [0, 1], [0, 1], ei, bursts=[1, 4], seed=5)
    with open(tmp_path / "out" / network / dataset / "scrubbing" / ("%s_%s_scrubbing_stats.json" % (network, dataset))) as f:
        doc = json.load(f)
    assert len(doc["results"]) == 2 * 2 * 2 * 2
    for scheme in ("none", "TMR"):
        for burst in (1, 4):
            for every in (0, 1):
                zero = doc["results"]["%s burst %d upset rate 0 scrub every %d" % (scheme, burst, every)]
                some = doc["results"]["%s burst %d upset rate %g scrub every %d" % (scheme, burst, 2.0 ** -3, every)]
                assert zero["runs"]["all"] == [nt.control] * 2 and zero["physical bits"] == 0
                assert len(some["mean accuracy per epoch"]) == 3 and some["physical bits"] > 0 and len(some["logical bits per epoch"]) == 3
            grow = doc["results"]["%s burst %d upset rate %g scrub every 0" % (scheme, burst, 2.0 ** -3)]["logical bits per epoch"]
            assert grow[0] < grow[2]
