"""Column-interleaved coded weight memories in the exposure campaigns, on the GPU (bnn_mi355x_iwecc_exposure_campaigns; the
model: csrc/mem_org.h "column-interleaved code words"; the kernels: csrc/iwecc_kernels.hip).  All checks are exact.

The model is pinned on the host: bnn_mi355x_pack_params_iwecc applies an ordered list of physical records with repair and
rewrite markers (tests/test_iwecc_pack.py, against the plain-Python route of tests/iwecc_ref.py).  The blob of (run, epoch
t) must be pack_params_iwecc of the marker-and-mask stream of epochs 0 ... t -- the masks are weight_code 1's, there is no
mask entry point of this family --; bnn_mi355x_iwecc_exposure_params reads back the very blob the device classifies that
epoch with, and the epoch's classes are compared with import_params(blob) + inference_buffer in a second library handle.
The twelve counts are what iwecc_ref's stepped code words give, and counts [0] are wecc_exposure_campaigns'.

The shape is tests/test_gpu_wecc_exposure.py's (wecc_ref.GPU_*): 3 runs x 24 images, 4 epochs of 6, every rate 2^-7 per
epoch (CNV layer 0's rates 0 in the coded-threshold cases), its four schedules; the cases are iwecc_ref.GPU_CASES: group
boundaries at PE ends, D = 2 / 8 / 16, two code words per 64-column word (cnvW2A2), rows shorter than a group (lfcW1A1 layer
0: 13 words a row, D = 16).  What these seeds hold is asserted on the CPU (tests/test_iwecc_pack.py, the coverage condition)."""
import ctypes as C
import faulthandler

import numpy as np
import pytest

import gpu_lib as gl
import iwecc_ref as ir
import repair_ref as rr
import test_gpu_act_fault_sweep as sw
import test_gpu_mem_noise as gm
import test_gpu_wecc_exposure as gw
import wecc_ref as wr

pytestmark = pytest.mark.gpu
RUNS, N, EI, E, SEED = wr.GPU_RUNS, wr.GPU_IMAGES, wr.GPU_EPOCH_IMAGES, wr.GPU_EPOCHS, wr.GPU_SEED
CASES = [(n, s, c, b) for n, cases in sorted(ir.GPU_CASES.items()) for s, c, b in cases]


@pytest.fixture(autouse=True)
def _time_limit():
    """every test runs in this process under a limit of its own (a case takes a few seconds): a device call that hangs
    ends the process with a traceback, and nothing more is started on the card"""
    faulthandler.dump_traceback_later(180, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def icampaign(L, path, scheme, code, weight_code, weight_interleave, burst, runs, seed, rw, rt, epoch_images, scrub_every=0, repair_every=0, ncls=10):
    """-> (classes [runs, n], counts [runs, epochs, layers, 12], seeds [runs])"""
    up = C.c_uint * len(rw)
    cnt, usec = C.c_int(0), C.c_float(0)
    p = L.bnn_mi355x_iwecc_exposure_campaigns(path.encode(), ncls, scheme, code, weight_code, weight_interleave, burst, runs, seed, up(*rw), up(*rt),
                                              len(rw), epoch_images, scrub_every, repair_every, C.byref(cnt), C.byref(usec))
    assert p, L.bnn_mi355x_last_error().decode()
    n = cnt.value
    got = np.ctypeslib.as_array(p, shape=(max(runs * n, 1),))[: runs * n].copy().reshape(runs, n)
    L.free_results(p)
    epochs = -(-n // epoch_images)
    k = L.bnn_mi355x_last_iwecc_exposure_counts(None, 0)
    assert k == runs * epochs * len(rw) * 12
    c = (C.c_long * k)()
    assert L.bnn_mi355x_last_iwecc_exposure_counts(c, k) == k
    s = (C.c_ulonglong * runs)()
    assert L.bnn_mi355x_last_iwecc_exposure_seeds(s, runs) == runs
    return got, np.array(c[:], np.int64).reshape(runs, epochs, len(rw), 12), list(s)


def idevice_blob(L, scheme, code, weight_code, weight_interleave, burst, seed, rw, rt, epoch, scrub_every=0, repair_every=0):
    up = C.c_uint * len(rw)
    size = L.bnn_mi355x_iwecc_exposure_params(scheme, code, weight_code, weight_interleave, burst, seed, up(*rw), up(*rt), len(rw), epoch, scrub_every,
                                              repair_every, None, 0)
    assert size > 0, L.bnn_mi355x_last_error().decode()
    blob = np.zeros(size, np.uint8)
    assert L.bnn_mi355x_iwecc_exposure_params(scheme, code, weight_code, weight_interleave, burst, seed, up(*rw), up(*rt), len(rw), epoch, scrub_every,
                                              repair_every, blob.ctypes.data, size) == size
    return blob


@pytest.mark.parametrize("network,scheme,code,burst", CASES, ids=str)
def test_interleaved_coded_weights(network, scheme, code, burst, tmp_path, monkeypatch):
    """the four schedules: for every run and epoch the device's blob is pack_params_iwecc of the marker-and-mask stream of
    epochs 0 ... t, byte for byte; the epoch's classes are those of that blob in a second library handle; the twelve counts
    are iwecc_ref's; counts [0] are what wecc_exposure_campaigns returns for the same arguments"""
    L, pdir = gm.load(network, wr.GPU_DATASET[network])
    L2 = gl.load(network, "python_hw")  # a second handle: importing a blob drops the raw memories the campaign draws in
    imgs = sw.images(network, N, seed=29)
    path = sw.write_images(network, imgs, tmp_path)
    clean_cls = gm.clean_classes(L, path)
    crc = L.bnn_mi355x_params_crc()
    rw, rt = wr.gpu_rates(network, code)
    coded = wr.coded_layers(network, 1)
    runs_epochs = [gw.drawn_epochs(L, network, scheme, code, burst, SEED + r, rw, rt) for r in range(RUNS)]
    monkeypatch.setenv("BNN_MI355X_NOISE_GROUP", "37")
    changed = cleared = differs = 0
    for every, repair in wr.GPU_SCHEDULES:
        what = "%s scheme %d code %d burst %d scrub every %d repair every %d" % (network, scheme, code, burst, every, repair)
        ref = [ir.campaign_counts(network, scheme, code, 1, 1, pdir, runs_epochs[r], every, repair) for r in range(RUNS)]
        want_counts = np.array([c for c, _ in ref])
        assert (want_counts[:, :, coded, 0] > 0).all() and want_counts[:, :, coded, 8].sum() > 0, what
        if repair == 0:
            assert (want_counts[..., 10:] == 0).all() and (want_counts[..., 6:8] == 0).all()
        else:
            assert (want_counts[:, 0, :, 10:] == 0).all() and want_counts[:, 1:, coded, 10].sum() > 0
        not_coded = [l for l in range(want_counts.shape[2]) if l not in coded]
        assert (want_counts[:, :, not_coded, 8:] == 0).all()
        classes = []
        for r in range(RUNS):
            classes.append([])
            before = None
            for t in range(E):
                stream = rr.stream(runs_epochs[r], t, every, repair)
                blob = ir.lib_pack(L, pdir, scheme, code, 1, 1, stream)
                gm.assert_same_bytes(idevice_blob(L, scheme, code, 1, 1, burst, SEED + r, rw, rt, t, every, repair), blob, what + " run %d epoch %d" % (r, t))
                classes[-1].append(gm.classify_with_blob(L2, blob, imgs))
                if t == E - 1:
                    differs += int((blob != wr.lib_pack(L, pdir, scheme, code, 1, stream)).sum())
                if network == "cnvW2A2":  # rows that lose their last -2 without a rewrite: the flag must go back to 0
                    now = np.concatenate([gw.row_flags(blob, l) for l in coded])
                    if before is not None and not rr.rewrites(t, every):
                        cleared += int(((before == 1) & (now == 0)).sum())
                    before = now
        got, counts, seeds = icampaign(L, path, scheme, code, 1, 1, burst, RUNS, SEED, rw, rt, EI, every, repair)
        assert seeds == [SEED + r for r in range(RUNS)]
        assert counts.tolist() == want_counts.tolist(), what
        _, plain_counts, _ = gw.wcampaign(L, path, scheme, code, 1, burst, RUNS, SEED, rw, rt, EI, every, repair)
        assert counts[..., 0].tolist() == plain_counts[..., 0].tolist(), what  # the events are the same
        assert counts[..., 2:8].tolist() == plain_counts[..., 2:8].tolist(), what  # and so is every threshold memory
        for r in range(RUNS):
            for t in range(E):
                want = classes[r][t][t * EI: (t + 1) * EI]
                assert got[r, t * EI: (t + 1) * EI].tolist() == want.tolist(), what + " run %d epoch %d" % (r, t)
                changed += int((want != clean_cls[t * EI: (t + 1) * EI]).sum())
    if network == "cnvW2A2":
        print("rows whose last -2 went away without a rewrite:", cleared)
        assert cleared > 0
    assert differs > 0  # the interleave delivers other weights than weight_code 1 alone
    assert changed > 0 and L.bnn_mi355x_params_crc() == crc
    assert gm.clean_classes(L, path).tolist() == clean_cls.tolist()


@pytest.mark.parametrize("network,scheme,code", [("cnvW1A1", 1, 0), ("cnvW1A1", 2, 1), ("cnvW2A2", 0, 1), ("lfcW1A1", 0, 1), ("lfcW1A2", 0, 0)], ids=str)
@pytest.mark.parametrize("weight_code", [0, 1])
def test_weight_interleave_0_is_the_wecc_exposure_campaign(network, scheme, code, weight_code, tmp_path, monkeypatch):
    """burst 2, scrub every 3, repair every 1: classes, seeds, the twelve counts and the blob of every epoch equal
    wecc_exposure_campaigns' / wecc_exposure_params' bit for bit; the wecc entry point's last_* state is not this one's"""
    L, pdir = gm.load(network, wr.GPU_DATASET[network])
    path = sw.write_images(network, sw.images(network, N, seed=17), tmp_path)
    monkeypatch.setenv("BNN_MI355X_NOISE_GROUP", "37")
    rw, rt = wr.gpu_rates(network, code)
    want, wcounts, wseeds = gw.wcampaign(L, path, scheme, code, weight_code, 2, RUNS, SEED, rw, rt, EI, 3, 1)
    got, counts, seeds = icampaign(L, path, scheme, code, weight_code, 0, 2, RUNS, SEED + 1, rw, rt, EI, 3, 1)  # (another seed: the states are apart)
    s = (C.c_ulonglong * RUNS)()
    L.bnn_mi355x_last_wecc_exposure_seeds(s, RUNS)
    assert list(s) == wseeds and seeds == [SEED + 1 + r for r in range(RUNS)]
    got, counts, seeds = icampaign(L, path, scheme, code, weight_code, 0, 2, RUNS, SEED, rw, rt, EI, 3, 1)
    assert seeds == wseeds and got.tolist() == want.tolist() and counts.tolist() == wcounts.tolist()
    assert wcounts[..., 0].sum() > 0 and (want != gm.clean_classes(L, path)[None]).any()
    for r in range(RUNS):
        for t in range(E):
            gm.assert_same_bytes(idevice_blob(L, scheme, code, weight_code, 0, 2, SEED + r, rw, rt, t, 3, 1),
                                 gw.wdevice_blob(L, scheme, code, weight_code, 2, SEED + r, rw, rt, t, 3, 1),
                                 "%s scheme %d code %d run %d epoch %d" % (network, scheme, code, r, t))


def test_rate_0_and_refusals(tmp_path):
    """all rates 0: the fault-free classes once per run, all counts 0; a weight rate of 0 in one coded layer leaves that
    layer's counts 0; refusals with a device present return NULL / 0 with a reason and leave no counts"""
    network = "cnvW1A1"
    L, pdir = gm.load(network, "cifar10")
    path = sw.write_images(network, sw.images(network, N, seed=4), tmp_path)
    clean = gm.clean_classes(L, path)
    z = [0] * 9
    got, counts, _ = icampaign(L, path, 1, 0, 1, 1, 1, RUNS, 5, z, z, EI, 0, 1)
    assert (got == clean[None]).all() and (counts == 0).all()
    assert (idevice_blob(L, 1, 0, 1, 1, 1, 5, z, z, 3, 0, 1) == gl.pack_params(network, pdir)).all()
    rw, rt = wr.gpu_rates(network, 0)
    rw[4] = 0
    got, counts, _ = icampaign(L, path, 0, 0, 1, 1, 2, RUNS, 5, rw, rt, EI, 0, 1)
    assert (counts[:, :, 4, [0, 1, 8, 9, 10, 11]] == 0).all() and (counts[:, :, 3, 0] > 0).all() and counts[:, :, 3, 8].sum() > 0
    up = C.c_uint * 9
    for wc, wi, reason in ((1, 2, b"weight_interleave must be 0 (none) or 1 (column-interleaved code words)"), (1, -1, b"weight_interleave must be 0 (none) or 1"),
                           (0, 1, b"weight_interleave 1 needs weight_code 1"), (2, 1, b"weight_code must be 0 (none) or 1"), (-1, 0, b"weight_code must be 0 (none) or 1")):
        assert not L.bnn_mi355x_iwecc_exposure_campaigns(path.encode(), 10, 0, 0, wc, wi, 1, 1, 1, up(*rw), up(*rt), 9, EI, 0, 1, None, None)
        assert b"iwecc_exposure_campaigns: " + reason in L.bnn_mi355x_last_error()
        assert L.bnn_mi355x_last_iwecc_exposure_counts(None, 0) == 0 and L.bnn_mi355x_last_iwecc_exposure_seeds(None, 0) == 0
        assert L.bnn_mi355x_iwecc_exposure_params(0, 0, wc, wi, 1, 1, up(*rw), up(*rt), 9, 1, 0, 1, None, 0) == 0
        assert b"iwecc_exposure_params: " + reason in L.bnn_mi355x_last_error()
    assert not L.bnn_mi355x_iwecc_exposure_campaigns(path.encode(), 10, 1, 1, 1, 1, 1, 1, 1, up(*rw), up(*rt), 9, EI, 0, 1, None, None)
    assert b"TMR plus a code is not modelled" in L.bnn_mi355x_last_error()
    assert L.bnn_mi355x_last_iwecc_exposure_counts(None, 0) == 0
    assert gm.clean_classes(L, path).tolist() == clean.tolist()


def test_another_grouping(tmp_path, monkeypatch):
    """the runs are worked off in groups (BNN_MI355X_NOISE_GROUP): 1, 2 and all at once give the same classes and counts"""
    network = "cnvW1A1"
    L, pdir = gm.load(network, "cifar10")
    path = sw.write_images(network, sw.images(network, N, seed=8), tmp_path)
    rw, rt = wr.gpu_rates(network, 0)
    results = []
    for group in ("1", "2", "37"):
        monkeypatch.setenv("BNN_MI355X_NOISE_GROUP", group)
        got, counts, seeds = icampaign(L, path, 1, 0, 1, 1, 2, RUNS, SEED, rw, rt, EI, 3, 1)
        results.append((got.tolist(), counts.tolist(), seeds))
    assert results[0] == results[1] == results[2] and np.array(results[0][1])[..., 8].sum() > 0


def test_python_interface(tmp_path):
    """FaultTest.run_exposure_test(..., weight_code=1, weight_interleave=1) returns what the C call returns; with
    weight_interleave 0 it keeps its entry points"""
    from bnn.faults import faults
    network, dataset = "cnvW1A1", "cifar10"
    L, pdir = gm.load(network, dataset)
    n, runs, seed, ei = 20, 2, 77, 8
    imgs = sw.images(network, n, seed=21)
    path = sw.write_images(network, imgs, tmp_path, network)
    labels = gm.clean_classes(L, path).tolist()
    ft = faults.CNVFaultTest(network, dataset, path, labels)
    rw, rt = gm.rates(network, 2.0 ** -7, 2.0 ** -7)
    acc, cnts = ft.run_exposure_test(runs, 2.0 ** -7, 2.0 ** -7, ei, scrub_every=0, scheme=1, burst=2, seed=seed, repair_every=1, weight_code=1,
                                     weight_interleave=1)
    got, counts, _ = icampaign(L, path, 1, 0, 1, 1, 2, runs, seed, rw, rt, ei, 0, 1)
    assert ft.exposure_results.tolist() == got.tolist() and cnts.tolist() == counts.tolist() and cnts.shape == (runs, 3, 9, 12)
    assert cnts[:, 1:, 1:, 10].sum() > 0 and cnts[..., 8].sum() > 0
    _, plain = ft.run_exposure_test(runs, 2.0 ** -7, 2.0 ** -7, ei, scrub_every=0, scheme=1, burst=2, seed=seed, repair_every=1, weight_code=1)
    assert plain.tolist() == gw.wcampaign(L, path, 1, 0, 1, 2, runs, seed, rw, rt, ei, 0, 1)[1].tolist()
    assert plain[:, :, 1, 8].sum() == 0 and cnts[:, :, 1, 8].sum() > 0  # layer 1 (32-bit elements): burst 2 corrects only when interleaved
    accs, one = ft.run_memory_noise_test(runs, 2.0 ** -7, 2.0 ** -7, seed, 1, 2, 0, 1, 1)
    assert one.shape == (runs, 9, 12) and one.tolist() == cnts[:, 0].tolist()
    assert faults.organisation_name(1, 0, 1) == "TMR + SEC-DED weights" and faults.organisation_name(1, 0, 1, 1) == "TMR + SEC-DED weights column-interleaved"
