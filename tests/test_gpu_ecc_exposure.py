"""SEC-DED coded threshold memories in the exposure campaigns, on the GPU (bnn_mi355x_ecc_exposure_campaigns; the code:
csrc/ecc.h, storage and upsets: csrc/mem_org.h).  All checks are exact.

The model is pinned on the host: bnn_mi355x_ecc_exposure_mask lists an epoch's events, check memories included
(tests/test_ecc_mask.py); bnn_mi355x_pack_params_ecc applies any ordered list of physical records, de-interleaves and
decodes (tests/test_ecc_pack.py, against the plain-Python route of tests/ecc_ref.py).  The blob of (run, epoch t) must be
pack_params_ecc of the masks of the epochs since the last scrub, concatenated; bnn_mi355x_ecc_exposure_params reads back
the very blob the device classifies that epoch with, and the epoch's classes are compared with import_params(blob) +
inference_buffer in a second library handle.  The six counts are what the masks imply (ecc_ref).

The exposure tests' shape: 3 runs x 48 images, rates 2^-3 and 2^-8 per epoch on every memory, epochs of 12 images (4
epochs) and of 10 (5, the last one short).  Code 1 with (cnvW1A1, 0), (cnvW1A1, 2), (cnvW1A2, 2), (cnvW2A2, 0),
(lfcW1A1, 0), (lfcW1A2, 0); bursts 1 and 2 everywhere, burst 4 for the two cnvW1A1 cases."""
import ctypes as C
import faulthandler
import json

import numpy as np
import pytest

import ecc_ref as er
import exposure_ref as xr
import gpu_lib as gl
import hardened_ref as hr
import test_gpu_act_fault_sweep as sw
import test_gpu_exposure as gx
import test_gpu_mem_noise as gm
import test_mem_noise_mask as mm

pytestmark = pytest.mark.gpu
q32 = hr.q32
RUNS, N, SEED = 3, 48, 20261019
RATES = (2.0 ** -3, 2.0 ** -8)
EPOCH_IMAGES = (12, 10)
T_MAX = 5  # epochs of the longer configuration: ceil(48 / 10)
DATASET = dict(mm.NETS)
CASES = [("cnvW1A1", 0), ("cnvW1A1", 2), ("cnvW1A2", 2), ("cnvW2A2", 0), ("lfcW1A1", 0), ("lfcW1A2", 0)]
BURSTS = [(n, s, b) for n, s in CASES for b in ((1, 2, 4) if n == "cnvW1A1" else (1, 2))]
# 2^-12 per epoch, 4 epochs, 3 runs: seeds found on the CPU (from ecc_ref's draw alone) at which every coded word that is
# hit holds exactly one hit over the epochs, in all three runs, and every coded layer is hit (asserted again below)
# (cnvW1A1, scheme 2, burst 2: at SEED layer 1 -- 64 words -- holds no word whose hits cancelled to one; at this seed,
# found on the CPU from ecc_ref's draw alone, it does.  Asserted with the other preconditions)
SEEDS = {("cnvW1A1", 2, 2): 20261033}
LOW = 2.0 ** -12
LOW_SEEDS = {("cnvW1A1", 0, 1): 1001, ("cnvW1A1", 2, 1): 1003, ("cnvW1A1", 2, 2): 1004, ("cnvW1A2", 2, 1): 1010, ("cnvW1A2", 2, 2): 1020,
             ("cnvW2A2", 0, 1): 1002, ("lfcW1A1", 0, 1): 1005, ("lfcW1A2", 0, 1): 1108}


@pytest.fixture(autouse=True)
def _time_limit():
    """every test runs in this process under a limit of its own (a case takes a few seconds): a device call that hangs
    ends the process with a traceback, and nothing more is started on the card"""
    faulthandler.dump_traceback_later(180, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def ecampaign(L, path, scheme, code, burst, runs, seed, rw, rt, epoch_images, scrub_every=0, ncls=10):
    """-> (classes [runs, n], counts [runs, epochs, layers, 6], seeds [runs])"""
    up = C.c_uint * len(rw)
    cnt, usec = C.c_int(0), C.c_float(0)
    p = L.bnn_mi355x_ecc_exposure_campaigns(path.encode(), ncls, scheme, code, burst, runs, seed, up(*rw), up(*rt), len(rw), epoch_images,
                                            scrub_every, C.byref(cnt), C.byref(usec))
    assert p, L.bnn_mi355x_last_error().decode()
    n = cnt.value
    got = np.ctypeslib.as_array(p, shape=(max(runs * n, 1),))[: runs * n].copy().reshape(runs, n)
    L.free_results(p)
    epochs = -(-n // epoch_images)
    k = L.bnn_mi355x_last_ecc_exposure_counts(None, 0)
    assert k == runs * epochs * len(rw) * 6
    c = (C.c_long * k)()
    assert L.bnn_mi355x_last_ecc_exposure_counts(c, k) == k
    s = (C.c_ulonglong * runs)()
    assert L.bnn_mi355x_last_ecc_exposure_seeds(s, runs) == runs
    return got, np.array(c[:], np.int64).reshape(runs, epochs, len(rw), 6), list(s)


def edevice_blob(L, scheme, code, burst, seed, rw, rt, epoch, scrub_every=0):
    up = C.c_uint * len(rw)
    size = L.bnn_mi355x_ecc_exposure_params(scheme, code, burst, seed, up(*rw), up(*rt), len(rw), epoch, scrub_every, None, 0)
    assert size > 0, L.bnn_mi355x_last_error().decode()
    blob = np.zeros(size, np.uint8)
    assert L.bnn_mi355x_ecc_exposure_params(scheme, code, burst, seed, up(*rw), up(*rt), len(rw), epoch, scrub_every, blob.ctypes.data, size) == size
    return blob


def rates_of(network, p):
    return gm.rates(network, p, p)


def coded_layers(network):
    return [l for l in range(len(hr.params_io.layout(network))) if er.coded(network, 1, l)]


def small(layer, target):
    """the memories restated in plain Python: every threshold memory (data and check) and layer 0"""
    return target == 1 or layer == 0


def drawn_epochs(L, network, scheme, burst, seed, rw, rt, restate, epochs=T_MAX):
    """a run's masks of epochs 0 ... epochs - 1 from the library, each {(layer, target, module): records} in the in-epoch
    order; restate: the plain-Python draw of the threshold memories -- check memories included -- and of layer 0 takes
    their place, after the library's were found equal"""
    out = []
    for t in range(epochs):
        recs = er.lib_epoch_events(L, network, scheme, 1, burst, seed, t, rw, rt)
        if restate:
            for key, mine in er.epoch_events(network, scheme, 1, burst, seed, t, rw, rt, small).items():
                assert mine.shape == recs[key].shape and (mine == recs[key]).all(), (t, key)
                recs[key] = mine
        out.append(recs)
    return out


def assert_accumulation_preconditions(network, scheme, burst, pdir, runs_epochs, epoch_counts):
    """at 2^-3, from the restatement's events of epochs 0 ... E - 1 alone, for every E of epoch_counts, in every coded layer
    (in one of the runs):
    - a word hit in the check memory alone;
    - a word with two accumulated hits (status 2: detected, the data as stored);
    - under scheme 2, an event of an epoch later than 0 that reaches the partner line's code word;
    and, where single bits can arrive alone (burst 1; burst 2 under scheme 2, which splits every burst over two words):
    - a word with exactly one accumulated hit although a bit of it was hit in two epochs (they cancelled): only an
      accumulation that XORs decodes it as a single error;
    - a word with exactly two accumulated hits that arrived in different epochs: an epoch on its own corrects each;
    - a word with exactly three, accepted as a correction with the data wrong.
    (A burst of an even number of bits inside one word leaves even error weights alone, which decode with status 0 or 2:
    for those cases a word whose hits all cancelled is asserted instead.)"""
    singles = burst == 1 or (scheme == 2 and burst == 2)
    decode = {}
    for layer in coded_layers(network):
        seen = {E: dict(check_alone=False, status2=False, cancelled_to_one=False, two_epochs=False, three=False, all_cancelled=False) for E in epoch_counts}
        reach = {E: scheme != 2 for E in epoch_counts}
        for per_epoch in runs_epochs:
            h = er.word_hits(network, scheme, pdir, per_epoch[:max(epoch_counts)], layer)
            bits = (h[:, :, None] >> np.arange(22)) & 1  # [epoch][word][bit]
            cum = bits.cumsum(axis=0)
            net = cum & 1
            weight = net.sum(axis=2)
            for t in range(max(epoch_counts)):
                masks = (net[t] << np.arange(22)).sum(axis=1)
                for m in set(masks.tolist()) - set(decode):
                    decode[m] = er.decode(m & 0xFFFF, m >> 16)
                status = np.array([decode[m][0] for m in masks.tolist()])
                residual = np.array([decode[m][1] for m in masks.tolist()])
                together = (bits[: t + 1] & net[t][None]).sum(axis=2).max(axis=0)
                now = dict(check_alone=(((masks & 0xFFFF) == 0) & (masks != 0)).any(), status2=(status == 2).any(),
                           cancelled_to_one=((weight[t] == 1) & (cum[t] >= 2).any(axis=1) & (status == 1) & (residual == 0)).any(),
                           two_epochs=((weight[t] == 2) & (together <= 1) & (status == 2)).any(),
                           three=((weight[t] == 3) & (status == 1) & (residual != 0)).any(),
                           all_cancelled=((weight[t] == 0) & (cum[t].sum(axis=1) > 0)).any())
                for E in epoch_counts:
                    if t < E:
                        for k, v in now.items():
                            seen[E][k] |= bool(v)
            for E in epoch_counts:
                reach[E] = reach[E] or any(er.reaches_partner(scheme, e[(layer, 1, m)]) for e in per_epoch[1:E] for m in (0, 1))
        need = ["check_alone", "status2"] + (["cancelled_to_one", "two_epochs", "three"] if singles else ["all_cancelled"])
        for E in epoch_counts:
            assert all(seen[E][k] for k in need) and reach[E], (layer, E, seen[E], reach[E])


@pytest.mark.parametrize("network,scheme", gx.PAIRS, ids=str)
def test_code_0_is_the_exposure_campaign(network, scheme, tmp_path, monkeypatch):
    """every (network, scheme) of the exposure tests at 2^-5, burst 2, epochs of 12, scrub_every 2: classes, seeds, the
    first four counts and the blob of every epoch equal exposure_campaigns' / exposure_params' bit for bit; the two
    decode-status counts are 0; the exposure entry point's last_* state is not this one's"""
    L, pdir = gm.load(network, DATASET[network])
    path = sw.write_images(network, sw.images(network, N, seed=17), tmp_path)
    monkeypatch.setenv("BNN_MI355X_NOISE_GROUP", "37")
    rw, rt = rates_of(network, 2.0 ** -5)
    want, wcounts, wseeds = gx.xcampaign(L, path, scheme, 2, RUNS, SEED, rw, rt, 12, 2)
    got, counts, seeds = ecampaign(L, path, scheme, 0, 2, RUNS, SEED + 1, rw, rt, 12, 2)  # (another seed: the states are apart)
    s = (C.c_ulonglong * RUNS)()
    L.bnn_mi355x_last_exposure_seeds(s, RUNS)
    assert list(s) == wseeds and seeds == [SEED + 1 + r for r in range(RUNS)]
    got, counts, seeds = ecampaign(L, path, scheme, 0, 2, RUNS, SEED, rw, rt, 12, 2)
    assert seeds == wseeds and got.tolist() == want.tolist()
    assert counts[..., :4].reshape(wcounts.shape).tolist() == wcounts.tolist() and (counts[..., 4:] == 0).all()
    assert wcounts[..., 0].sum() > 0 and (want != gm.clean_classes(L, path)[None]).any()
    for r in range(RUNS):
        for t in range(4):
            gm.assert_same_bytes(edevice_blob(L, scheme, 0, 2, SEED + r, rw, rt, t, 2), gx.xdevice_blob(L, scheme, 2, SEED + r, rw, rt, t, 2),
                                 "%s scheme %d run %d epoch %d" % (network, scheme, r, t))


@pytest.mark.parametrize("network,scheme,burst", BURSTS, ids=str)
def test_accumulation(network, scheme, burst, tmp_path, monkeypatch):
    """code 1, scrub_every 0, both rates, epochs of 12 and of 10 images: for every run and epoch the device's blob is
    pack_params_ecc of the masks of epochs 0 ... t concatenated, byte for byte; the epoch's classes are those of that blob
    in a second library handle; the six counts are what the masks imply; another grouping of the pairs changes nothing.
    Before any device result is looked at, the cases only a correct decoder and a correct accumulation get right are
    asserted present at 2^-3 from the plain-Python restatement alone"""
    SEED = SEEDS.get((network, scheme, burst), globals()["SEED"])
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
        runs_epochs = [drawn_epochs(L, network, scheme, burst, SEED + r, rw, rt, p == RATES[0]) for r in range(RUNS)]
        if p == RATES[0]:
            assert_accumulation_preconditions(network, scheme, burst, pdir, runs_epochs, [-(-N // ei) for ei in EPOCH_IMAGES])
        classes, want_counts = [], []
        for r in range(RUNS):
            classes.append([])
            want_counts.append([])
            for t in range(T_MAX):
                blob = er.lib_pack(L, pdir, scheme, 1, er.since_scrub(runs_epochs[r], t, 0))
                gm.assert_same_bytes(edevice_blob(L, scheme, 1, burst, SEED + r, rw, rt, t), blob, what + " run %d epoch %d" % (r, t))
                classes[-1].append(gm.classify_with_blob(L2, blob, imgs))
                want_counts[-1].append(er.implied_counts(network, scheme, 1, pdir, runs_epochs[r], t, 0))
        want_counts = np.array(want_counts)
        for ei in EPOCH_IMAGES:
            E = -(-N // ei)
            monkeypatch.setenv("BNN_MI355X_NOISE_GROUP", "37")
            got, counts, seeds = ecampaign(L, path, scheme, 1, burst, RUNS, SEED, rw, rt, ei)
            assert seeds == [SEED + r for r in range(RUNS)]
            assert counts.tolist() == want_counts[:, :E].tolist(), what
            monkeypatch.setenv("BNN_MI355X_NOISE_GROUP", "1000")
            g2, c2, _ = ecampaign(L, path, scheme, 1, burst, RUNS, SEED, rw, rt, ei)
            assert g2.tolist() == got.tolist() and c2.tolist() == counts.tolist(), what
            for r in range(RUNS):
                for t in range(E):
                    want = classes[r][t][t * ei: (t + 1) * ei]
                    assert got[r, t * ei: (t + 1) * ei].tolist() == want.tolist(), what + " run %d epoch %d of %d images" % (r, t, ei)
                    changed += int((want != clean_cls[t * ei: (t + 1) * ei]).sum())
        coded = coded_layers(network)
        if p == RATES[0]:  # both decode statuses are counted in every coded layer, and none in an uncoded one
            assert (want_counts[:, :, coded, 5].sum(axis=(0, 1)) > 0).all()
            if burst == 1 or (scheme == 2 and burst == 2):  # (even bursts inside one word leave nothing to correct)
                assert (want_counts[:, :, coded, 4].sum(axis=(0, 1)) > 0).all()
        uncoded = [l for l in range(want_counts.shape[2]) if l not in coded]
        assert (want_counts[:, :, uncoded, 4:] == 0).all()
    assert changed > 0 and L.bnn_mi355x_params_crc() == crc
    assert gm.clean_classes(L, path).tolist() == clean_cls.tolist()


@pytest.mark.parametrize("network,scheme,burst", sorted(LOW_SEEDS), ids=str)
def test_correction_shows(network, scheme, burst, tmp_path):
    """2^-12 per epoch on every memory, 4 epochs of 12 images.  First, from ecc_ref's draw alone: every coded word that
    is hit holds exactly one hit over the epochs, in every run, and every coded layer is hit.  Then: the threshold logical
    count of every coded layer is 0 in every (run, epoch), physical > 0 and corrected > 0 (the words hit so far,
    exactly), none detected; the classes are those of a run with the threshold rates of the coded layers set to 0 --
    weights and layer 0 left as they are -- through this entry point and through exposure_campaigns; without the code
    the same upsets leave logical bits.  Burst 2 under scheme 2 likewise (the interleave splits every burst over two code
    words); burst 2 under scheme 0 is detected, not corrected."""
    seed, ei, E = LOW_SEEDS[(network, scheme, burst)], 12, 4
    L, pdir = gm.load(network, DATASET[network])
    path = sw.write_images(network, sw.images(network, N, seed=27), tmp_path)
    rw, rt = rates_of(network, LOW)
    coded = coded_layers(network)
    hit_so_far = np.zeros((RUNS, E, len(rw)), np.int64)
    for r in range(RUNS):
        per_epoch = [er.epoch_events(network, scheme, 1, burst, seed + r, t, rw, rt, lambda l, target: target == 1 and l in coded) for t in range(E)]
        for l in coded:
            h = er.word_hits(network, scheme, pdir, per_epoch, l)
            n = ((h[:, :, None] >> np.arange(22)) & 1).sum(axis=2)  # [epoch][word]
            assert (n.sum(axis=0) <= 1).all(), (r, l)
            hit_so_far[r, :, l] = (n.cumsum(axis=0) > 0).sum(axis=1)
    assert (hit_so_far[:, -1, coded].sum(axis=0) > 0).all()
    got, counts, _ = ecampaign(L, path, scheme, 1, burst, RUNS, seed, rw, rt, ei)
    assert (counts[:, :, coded, 3] == 0).all() and (counts[:, :, coded, 5] == 0).all()
    assert (counts[:, :, coded, 2].sum(axis=(0, 1)) > 0).all() and (counts[:, :, coded, 4].sum(axis=(0, 1)) > 0).all()
    assert counts[:, :, coded, 4].tolist() == hit_so_far[:, :, coded].tolist()
    rt0 = [0 if l in coded else x for l, x in enumerate(rt)]
    ref, rcounts, _ = ecampaign(L, path, scheme, 1, burst, RUNS, seed, rw, rt0, ei)
    assert got.tolist() == ref.tolist() and (rcounts[:, :, coded, 2:] == 0).all()
    assert counts[..., :2].tolist() == rcounts[..., :2].tolist()
    old, ocounts, _ = gx.xcampaign(L, path, scheme, burst, RUNS, seed, rw, rt0, ei)
    assert got.tolist() == old.tolist() and ocounts[:, :, :, 0].tolist() == counts[..., :2].tolist()
    bare = ecampaign(L, path, scheme, 0, burst, RUNS, seed, rw, rt, ei)[1]
    assert bare[:, :, coded, 3].sum() > 0  # (uncoded, the same data upsets stay)
    if scheme == 0:  # a burst of 2 inside one word: a double error, detected and left as stored
        _, c2, _ = ecampaign(L, path, 0, 1, 2, RUNS, seed, rw, rt, ei)
        assert c2[:, :, coded, 5].sum() > 0 and c2[:, :, coded, 3].sum() > 0


@pytest.mark.parametrize("network,scheme,burst", [("cnvW1A1", 2, 2), ("cnvW2A2", 0, 1), ("lfcW1A1", 0, 2)], ids=str)
def test_scrubbing(network, scheme, burst, tmp_path, monkeypatch):
    """5 epochs of 10 images (the last one short) at 2^-3, scrub_every 2: blobs and counts are pack_params_ecc's / the
    masks' since the last scrub -- right after a scrub epoch's upsets (epochs 2 and 4) the state is what that epoch's
    mask alone implies, data and check words rewritten; epochs 0 and 1 are the unscrubbed run's"""
    SEED = SEEDS.get((network, scheme, burst), globals()["SEED"])
    L, pdir = gm.load(network, DATASET[network])
    L2 = gl.load(network, "python_hw")
    imgs = sw.images(network, N, seed=29)
    path = sw.write_images(network, imgs, tmp_path)
    ei, E, every = 10, 5, 2
    rw, rt = rates_of(network, RATES[0])
    monkeypatch.setenv("BNN_MI355X_NOISE_GROUP", "37")
    per_epoch = [drawn_epochs(L, network, scheme, burst, SEED + r, rw, rt, True, E) for r in range(RUNS)]
    implied = {s: np.array([[er.implied_counts(network, scheme, 1, pdir, per_epoch[r], t, s) for t in range(E)] for r in range(RUNS)]) for s in (0, every)}
    coded = coded_layers(network)
    # (from the masks) the scrub before epoch 2 takes detected words away, in every run
    assert (implied[every][:, 2, coded, 5].sum(axis=1) < implied[0][:, 2, coded, 5].sum(axis=1)).all()
    what = "%s scheme %d burst %d scrub every %d" % (network, scheme, burst, every)
    got, counts, _ = ecampaign(L, path, scheme, 1, burst, RUNS, SEED, rw, rt, ei, every)
    assert counts.tolist() == implied[every].tolist(), what
    for r in range(RUNS):
        for t in range(E):
            assert xr.first_epoch(t, every) == (0, 0, 2, 2, 4)[t]
            blob = er.lib_pack(L, pdir, scheme, 1, er.since_scrub(per_epoch[r], t, every))
            dev = edevice_blob(L, scheme, 1, burst, SEED + r, rw, rt, t, every)
            gm.assert_same_bytes(dev, blob, what + " run %d epoch %d" % (r, t))
            if t in (2, 4):
                gm.assert_same_bytes(dev, er.lib_pack(L, pdir, scheme, 1, er.flat(per_epoch[r][t])), what + " run %d scrub epoch %d" % (r, t))
            if t < 2:
                assert (dev == edevice_blob(L, scheme, 1, burst, SEED + r, rw, rt, t, 0)).all()
            want = gm.classify_with_blob(L2, blob, imgs)[t * ei: (t + 1) * ei]
            assert got[r, t * ei: (t + 1) * ei].tolist() == want.tolist(), what + " run %d epoch %d" % (r, t)
    unscrubbed = ecampaign(L, path, scheme, 1, burst, RUNS, SEED, rw, rt, ei, 0)[1]
    assert unscrubbed.tolist() == implied[0].tolist() and unscrubbed[:, :2].tolist() == counts[:, :2].tolist()


def test_rate_0_refusals_and_side_effects(tmp_path):
    """all rates 0: the fault-free classes once per run, all counts 0, the parameters read back are the loaded ones; the
    loaded parameters (params_crc, the classes they give) and the last_* state of the exposure entry point are unchanged
    after every call.  Refusals return NULL / 0 with a reason and leave no counts: code 1 with scheme 1 or 3, a code
    outside 0 ... 1, what the scheme alone refuses, a bad epoch length, an imported blob."""
    network = "cnvW1A2"
    L, pdir = gm.load(network, "cifar10")
    path = sw.write_images(network, sw.images(network, N, seed=4), tmp_path)
    clean = gm.clean_classes(L, path)
    crc = L.bnn_mi355x_params_crc()
    z = [0] * 9
    rw, rt = rates_of(network, 2.0 ** -8)
    exposure = gx.xcampaign(L, path, 1, 1, 2, 11, rw, rt, 12, 0)[1:]

    def untouched():
        assert L.bnn_mi355x_params_crc() == crc and gm.clean_classes(L, path).tolist() == clean.tolist()
        k = L.bnn_mi355x_last_exposure_counts(None, 0)
        c = (C.c_long * k)()
        L.bnn_mi355x_last_exposure_counts(c, k)
        s = (C.c_ulonglong * 2)()
        assert L.bnn_mi355x_last_exposure_seeds(s, 2) == 2
        assert list(c) == exposure[0].reshape(-1).tolist() and list(s) == exposure[1]

    for scheme, code, burst, ei, every in ((0, 1, 1, 12, 0), (2, 1, 4, 10, 2), (2, 0, 16, 100, 1), (1, 0, 2, 12, 0)):
        got, counts, _ = ecampaign(L, path, scheme, code, burst, RUNS, 5, z, z, ei, every)
        assert (got == clean[None]).all() and (counts == 0).all() and counts.shape[1] == -(-N // ei)
        assert (edevice_blob(L, scheme, code, burst, 5, z, z, 3, every) == gl.pack_params(network, pdir)).all()
        untouched()
    got, counts, _ = ecampaign(L, path, 2, 1, 4, RUNS, 5, rw, rt, 12, 2)
    assert counts[..., 2].sum() > 0
    untouched()
    up = C.c_uint * 9
    for scheme, code, reason in ((1, 1, b"TMR plus a code is not modelled"), (3, 1, b"resilient patterns are defined for 32 and 48 positions only"),
                                 (0, 2, b"code must be 0 (none) or 1 (SEC-DED)"), (2, -1, b"code must be"), (4, 1, b"scheme must be")):
        assert not L.bnn_mi355x_ecc_exposure_campaigns(path.encode(), 10, scheme, code, 1, 1, 1, up(*rw), up(*rt), 9, 12, 0, None, None)
        assert reason in L.bnn_mi355x_last_error()
        assert L.bnn_mi355x_last_ecc_exposure_counts(None, 0) == 0 and L.bnn_mi355x_last_ecc_exposure_seeds(None, 0) == 0
        assert L.bnn_mi355x_ecc_exposure_params(scheme, code, 1, 1, up(*rw), up(*rt), 9, 1, 0, None, 0) == 0
        assert reason in L.bnn_mi355x_last_error()
    for ei, every in ((0, 0), (-1, 0), (12, -1)):
        assert not L.bnn_mi355x_ecc_exposure_campaigns(path.encode(), 10, 2, 1, 1, 1, 1, up(*rw), up(*rt), 9, ei, every, None, None)
        assert b"epoch_images must be at least 1" in L.bnn_mi355x_last_error()
    assert not L.bnn_mi355x_ecc_exposure_campaigns(path.encode(), 10, 2, 1, 17, 1, 1, up(*rw), up(*rt), 9, 12, 0, None, None)
    assert b"burst" in L.bnn_mi355x_last_error()
    assert L.bnn_mi355x_ecc_exposure_params(2, 1, 1, 1, up(*rw), up(*rt), 9, xr.MAX_EPOCHS, 0, None, 0) == 0
    assert b"epoch must be" in L.bnn_mi355x_last_error()
    big = tmp_path / "sparse.bin"  # too many epochs: refused from the file's size alone (a sparse file: nothing is read)
    with open(big, "wb") as f:
        f.truncate((xr.MAX_EPOCHS + 1) * 3073)
    assert not L.bnn_mi355x_ecc_exposure_campaigns(str(big).encode(), 10, 2, 1, 1, 1, 1, up(*rw), up(*rt), 9, 1, 0, None, None)
    assert b"epochs: at most 65536" in L.bnn_mi355x_last_error()
    untouched()
    W = gm.load("cnvW2A2", "cifar10")[0]
    assert not W.bnn_mi355x_ecc_exposure_campaigns(path.encode(), 10, 2, 1, 1, 1, 1, up(*rw), up(*rt), 9, 12, 0, None, None)
    assert b"cnvW2A2 with scheme 2" in W.bnn_mi355x_last_error()
    blob = gl.pack_params(network, pdir)
    assert L.bnn_mi355x_import_params(blob.ctypes.data, len(blob)) == 0
    assert not L.bnn_mi355x_ecc_exposure_campaigns(path.encode(), 10, 2, 1, 1, 1, 1, up(*rw), up(*rt), 9, 12, 0, None, None)
    assert b"imported blob" in L.bnn_mi355x_last_error()
    assert L.bnn_mi355x_ecc_exposure_params(2, 1, 1, 1, up(*rw), up(*rt), 9, 1, 0, None, 0) == 0
    assert b"imported blob" in L.bnn_mi355x_last_error()
    L.load_parameters(pdir.encode())


def test_variant_library_runs_the_same_campaign(variant_libs, tmp_path):
    """cnvW1A1-interleaved's library gives the classes, counts and blobs of the base network's library for the scheme its
    name implies, with the code"""
    network = "cnvW1A1"
    L, pdir = gm.load(network, "cifar10")
    V = gl.load("cnvW1A1-interleaved")
    V.load_parameters(pdir.encode())
    assert V.bnn_mi355x_last_error() == b""
    path = sw.write_images(network, sw.images(network, N, seed=6), tmp_path)
    rw, rt = rates_of(network, 2.0 ** -3)
    scheme = V.bnn_mi355x_hardening_scheme()
    assert scheme == 2
    a = ecampaign(V, path, scheme, 1, 2, RUNS, 9, rw, rt, 10, 3)
    b = ecampaign(L, path, scheme, 1, 2, RUNS, 9, rw, rt, 10, 3)
    assert a[0].tolist() == b[0].tolist() and a[1].tolist() == b[1].tolist() and a[1][..., 4].sum() > 0 and a[1][..., 5].sum() > 0
    assert (edevice_blob(V, scheme, 1, 2, 9, rw, rt, 4, 3) == edevice_blob(L, scheme, 1, 2, 9, rw, rt, 4, 3)).all()


def test_python_interface(tmp_path):
    """FaultTest.run_exposure_test(..., code=1) on 40 images in epochs of 16 (the last one short) returns what the C call
    returns; run_memory_noise_test(..., code=1) is the one-epoch campaign; without a code both keep their entry points;
    NetworkTest.scrubbing_curve and hardening_curve accept (scheme, code) pairs next to plain schemes and write the
    decode-status counts"""
    from bnn.faults import faults
    network, dataset = "cnvW1A1", "cifar10"
    L, pdir = gm.load(network, dataset)
    n, runs, seed, ei = 40, 3, 77, 16
    imgs = sw.images(network, n, seed=21)
    path = sw.write_images(network, imgs, tmp_path, network)
    labels = gm.clean_classes(L, path).tolist()
    labels[0] = (labels[0] + 1) % 10
    ft = faults.CNVFaultTest(network, dataset, path, labels)
    acc, cnts = ft.run_exposure_test(runs, 2.0 ** -7, 2.0 ** -3, ei, scrub_every=2, scheme=2, burst=2, seed=seed, code=1)
    rw, rt = gm.rates(network, 2.0 ** -7, 2.0 ** -3)
    got, counts, _ = ecampaign(L, path, 2, 1, 2, runs, seed, rw, rt, ei, 2)
    assert ft.exposure_results.tolist() == got.tolist() and cnts.tolist() == counts.tolist() and cnts.shape == (runs, 3, 9, 6)
    lab = np.array(labels)
    assert acc == [[100.0 * (row[i: i + ei] == lab[i: i + ei]).sum() / len(lab[i: i + ei]) for i in range(0, n, ei)] for row in got]
    acc1, cnts1 = ft.run_memory_noise_test(runs, 2.0 ** -7, 2.0 ** -3, seed, scheme=2, burst=2, code=1)
    one, c1, _ = ecampaign(L, path, 2, 1, 2, runs, seed, rw, rt, n)
    assert ft.mem_noise_results.tolist() == one.tolist() and cnts1.tolist() == c1[:, 0].tolist() and cnts1.shape == (runs, 9, 6)
    assert acc1 == [100.0 * (row == lab).sum() / n for row in one]
    _, plain = ft.run_exposure_test(runs, 2.0 ** -7, 2.0 ** -3, ei, scrub_every=2, scheme=2, burst=2, seed=seed)
    assert plain.shape == (runs, 3, 9, 2, 2) and plain.tolist() == gx.xcampaign(L, path, 2, 2, runs, seed, rw, rt, ei, 2)[1].tolist()
    nt = faults.NetworkTest(ft)
    nt.scrubbing_curve(str(tmp_path / "out"), 2, [2.0 ** -3], [0, 1], [0, (0, 1), (2, 1)], ei, bursts=[2], seed=5)
    with open(tmp_path / "out" / network / dataset / "scrubbing" / ("%s_%s_scrubbing_stats.json" % (network, dataset))) as f:
        doc = json.load(f)
    assert len(doc["results"]) == 3 * 2
    for every in (0, 1):
        bare = doc["results"]["none burst 2 upset rate %g scrub every %d" % (2.0 ** -3, every)]
        assert "code" not in bare and len(bare["logical bits per epoch"]) == 3
        for name in ("none + SEC-DED", "interleaved + SEC-DED"):
            e = doc["results"]["%s burst 2 upset rate %g scrub every %d" % (name, 2.0 ** -3, every)]
            assert e["code"] == 1 and len(e["corrected words per epoch"]) == 3 and len(e["detected words per epoch"]) == 3
            assert e["physical bits"] > bare["physical bits"] and len(e["mean accuracy per epoch"]) == 3  # (the check memories take upsets too)
        assert sum(doc["results"]["none + SEC-DED burst 2 upset rate %g scrub every %d" % (2.0 ** -3, every)]["detected words per epoch"]) > 0
        assert sum(doc["results"]["interleaved + SEC-DED burst 2 upset rate %g scrub every %d" % (2.0 ** -3, every)]["corrected words per epoch"]) > 0
    nt.hardening_curve(str(tmp_path / "out"), 2, [2.0 ** -6], [2, (2, 1)], bursts=[2], seed=5)
    with open(tmp_path / "out" / network / dataset / "hardening" / ("%s_%s_hardening_stats.json" % (network, dataset))) as f:
        doc = json.load(f)
    e = doc["results"]["interleaved + SEC-DED burst 2 upset rate %g" % 2.0 ** -6]
    assert e["code"] == 1 and e["corrected words"] > 0 and "code" not in doc["results"]["interleaved burst 2 upset rate %g" % 2.0 ** -6]
    assert e["logical bits"] < doc["results"]["interleaved burst 2 upset rate %g" % 2.0 ** -6]["logical bits"]
