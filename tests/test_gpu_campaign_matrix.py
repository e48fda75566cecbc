"""Campaigns on the matrix cores (bnn_mi355x_campaign_form(1): layers 1-7 of every campaign launch as FP4 GEMMs, every run
from operand tables made on the device of its own faulted copy of the parameters).  All checks are exact: stage outputs
byte for byte against the integer pipe on the host route's blobs, whole calls against form 0 with the same seed."""
import ctypes as C

import numpy as np
import pytest

import gpu_lib as gl
import saturated_params as sp
import test_fault_campaigns as fc
import test_gpu_act_fault_sweep as sw
import test_gpu_act_noise as gan
import test_gpu_exposure as gx
import test_gpu_mem_noise as gm

pytestmark = pytest.mark.gpu
CNV = ("cnvW1A1", "cnvW1A2", "cnvW2A2")
RUNS, SEED, N_MAX = 3, 4321, 33
STAGES = range(1, 8)


@pytest.fixture
def form1():
    """the matrix form in every CNV library (the switch is per library) for the test, the form before it afterwards"""
    libs = [gl.load(n) for n in CNV]
    was = [x.bnn_mi355x_campaign_form(1) for x in libs]
    yield
    for x, f in zip(libs, was):
        x.bnn_mi355x_campaign_form(f)


@pytest.fixture(scope="module", params=CNV)
def reference(request):
    """-> (network, L, images, rates, ref[run][stage] = the integer pipe's stage output of all N_MAX images under the run's
    host-built blob: bnn_mi355x_debug_stage_output after import_params; below conv_mfma_min the fault-free pass is the
    integer pipe).  Computed once per network; the loaded parameters are restored."""
    network = request.param
    L, pdir = gm.load(network, "cifar10")
    imgs = sw.images(network, N_MAX, seed=91)
    p = gm.ROUTE_RATE[network]
    rw, rt = gm.rates(network, p, p)
    clean = gl.pack_params(network, pdir)
    blobs = [gm.host_blob(L, network, pdir, SEED + r, rw, rt)[0] for r in range(RUNS)]
    if network == "cnvW2A2":  # some run's blob gains a row with a -2 in some layer the matrix form covers
        gained = [int(((gm.flags(clean, l) == 0) & (gm.flags(b, l) == 1)).sum()) for b in blobs for l in STAGES]
        print("rows that gain a -2, per (run, layer):", gained)
        assert max(gained) >= 1
    ref = []
    for blob in blobs:
        assert L.bnn_mi355x_import_params(blob.ctypes.data, len(blob)) == 0, L.bnn_mi355x_last_error()
        assert L.bnn_mi355x_matrix_stages(N_MAX) & 0xFE == 0
        per_stage = {}
        for st in STAGES:
            dst = np.zeros(N_MAX * 7200 * 2, np.uint8)
            per = L.bnn_mi355x_debug_stage_output(imgs.ctypes.data, N_MAX, st, dst.ctypes.data, dst.size)
            assert per > 0, L.bnn_mi355x_last_error()
            per_stage[st] = dst[: N_MAX * per].reshape(N_MAX, per).copy()
        ref.append(per_stage)
    L.load_parameters(pdir.encode())
    assert L.bnn_mi355x_last_error() == b""
    return network, L, imgs, (rw, rt), ref


@pytest.mark.parametrize("n,group", [(1, None), (9, None), (17, 5), (33, 20)])
def test_stage_parity(reference, form1, n, group, monkeypatch):
    """segments shorter than a kernel group, lengths and slots that are no multiple of it, a run cut across two launches
    and several runs' segments in one launch: every stage 1-7 of every (run, image) pair equals the integer pipe's"""
    network, L, imgs, (rw, rt), ref = reference
    if group:
        monkeypatch.setenv("BNN_MI355X_NOISE_GROUP", str(group))
    assert L.bnn_mi355x_campaign_matrix_stages(RUNS) == 0b11111110
    up = C.c_uint * len(rw)
    for st in STAGES:
        size = L.bnn_mi355x_debug_campaign_stage(imgs.ctypes.data, n, RUNS, SEED, up(*rw), up(*rt), len(rw), st, None, 0)
        assert size > 0 and size % (RUNS * n) == 0, L.bnn_mi355x_last_error()
        got = np.zeros(size, np.uint8)
        assert L.bnn_mi355x_debug_campaign_stage(imgs.ctypes.data, n, RUNS, SEED, up(*rw), up(*rt), len(rw), st, got.ctypes.data, size) == size, \
            L.bnn_mi355x_last_error()
        got = got.reshape(RUNS, n, -1)
        for r in range(RUNS):
            want = ref[r][st][:n]
            assert got[r].shape == want.shape
            bad = np.nonzero((got[r] != want).any(axis=1))[0]
            assert len(bad) == 0, "%s stage %d run %d: images %s differ" % (network, st, r, bad.tolist())


def _both_forms(L, call):
    out = []
    for form in (0, 1):
        L.bnn_mi355x_campaign_form(form)
        out.append(call())
    return out


@pytest.mark.parametrize("network", ["cnvW1A1", "cnvW2A2"])
def test_whole_calls(network, form1, tmp_path):
    """3 runs x 40 images: every campaign entry point returns under form 1 exactly the classes and counters of form 0 with the
    same seed -- the tables follow the patches of every wave, the upsets of every epoch and a scrub"""
    L, pdir = gm.load(network, "cifar10")
    runs, n = 3, 40
    path = sw.write_images(network, sw.images(network, n, seed=17), tmp_path)
    clean = gm.clean_classes(L, path)
    p = gm.ROUTE_RATE[network]
    rw, rt = gm.rates(network, p, p)
    zw, zt = gm.rates(network)
    nl = len(rw)
    calls = {
        "mem_noise": lambda: gm.campaign(L, path, runs, 55, rw, rt),
        "mem_noise rate 0": lambda: gm.campaign(L, path, runs, 55, zw, zt),
        "fault": lambda: fc.campaigns(L, path, runs, 66, 30, 4, 1),
        "act_noise": lambda: gan.campaign(L, path, runs, 77, [gan.q32(2.0 ** -6)] * (nl - 1)),
        "act_noise rate 0": lambda: gan.campaign(L, path, runs, 77, [0] * (nl - 1)),
        "exposure": lambda: gx.xcampaign(L, path, 0, 1, runs, 88, rw, rt, 14, scrub_every=2),
    }
    for name, call in calls.items():
        a, b = _both_forms(L, call)
        assert L.bnn_mi355x_campaign_matrix_stages(runs) == 0xFE
        changed = [int((a[0][r] != clean).sum()) for r in range(runs)]
        print(network, name, "images whose class form 0 changes, per run:", changed)
        if "rate 0" in name:
            assert max(changed) == 0
        else:
            assert max(changed) >= 1, name
        assert a[0].tolist() == b[0].tolist(), name
        assert np.array_equal(np.asarray(a[1]), np.asarray(b[1])), name


@pytest.mark.parametrize("network", CNV)
def test_saturated_parameters(network, form1, tmp_path):
    """the constant networks (accumulators at their extremes, thresholds on the boundary) through a zero-rate campaign under
    form 1 -- every run on the tables of the loaded parameters: the classes are inference_multiple's"""
    L = gl.load(network)
    imgs = sw.images(network, 32, seed=5)
    imgs[0], imgs[-1] = 0, 255
    path = sw.write_images(network, imgs, tmp_path)
    for config, neg2 in sp.variants(network):
        d = str(tmp_path / ("%s_%d" % (config, neg2)))
        sp.make(d, network, config, neg2)
        L.load_parameters(d.encode())
        assert L.bnn_mi355x_last_error() == b"", L.bnn_mi355x_last_error()
        assert L.bnn_mi355x_campaign_matrix_stages(2) == 0xFE
        want = gm.clean_classes(L, path)
        got, _, _ = gan.campaign(L, path, 2, 9, [0] * 8)
        assert got[0].tolist() == want.tolist() and got[1].tolist() == want.tolist(), (config, neg2)
    L.load_parameters(gl.param_dir("cifar10", network).encode())


def test_the_switch():
    L, _ = gm.load("cnvW1A1", "cifar10")
    was = L.bnn_mi355x_campaign_form(0)
    assert L.bnn_mi355x_campaign_form(7) == 0 and L.bnn_mi355x_campaign_form(-1) == 0 and L.bnn_mi355x_campaign_form(2) == 0
    assert L.bnn_mi355x_campaign_matrix_stages(3) == 0
    assert L.bnn_mi355x_campaign_form(1) == 0 and L.bnn_mi355x_campaign_form(7) == 1
    assert L.bnn_mi355x_campaign_matrix_stages(3) == 0b11111110
    assert L.bnn_mi355x_campaign_matrix_stages(4096) == 0  # 4096 x 775 424 bytes of tables: above the cap
    assert L.bnn_mi355x_campaign_form(was) == 1
    F, _ = gm.load("lfcW1A1", "mnist")
    was = F.bnn_mi355x_campaign_form(1)
    assert F.bnn_mi355x_campaign_matrix_stages(3) == 0
    F.bnn_mi355x_campaign_form(was)
