"""Many fault campaigns in one call (bnn_mi355x_fault_campaigns): the runs side by side on the GPU, in
waves, each with its own copy of the parameters.  Every run must be exactly what the sequential entry point returns for
the same seed (load_parameters + set_fault_seed(seed + r) + inference_multiple_with_faults), fault for fault and
class for class, and the loaded parameters must be left as they were."""
import ctypes as C
import struct

import numpy as np
import pytest

import gpu_lib as gl
import oracle_lib as ol

NETS = [("cnvW1A1", "cifar10"), ("cnvW1A2", "cifar10"), ("cnvW2A2", "cifar10"), ("lfcW1A1", "mnist"), ("lfcW1A2", "mnist")]
KMAX_CHUNK = 131072  # images per launch (runtime.hip, kMaxChunk)


def write_images(network, n, tmp_path, seed=17):
    rng = np.random.default_rng(seed)
    if network.startswith("cnv"):
        imgs = rng.integers(0, 256, (n, 3072), dtype=np.uint8)
        path = tmp_path / "imgs.bin"
        np.concatenate([np.ones((n, 1), np.uint8), imgs], axis=1).tofile(path)
    else:
        imgs = rng.integers(0, 256, (n, 784), dtype=np.uint8)
        path = tmp_path / "imgs-idx3-ubyte"
        with open(path, "wb") as f:
            f.write(struct.pack(">4I", 0x803, n, 28, 28) + imgs.tobytes())
    return imgs, str(path)


def campaigns(L, path, runs, seed, flips, word_size, target, layers=()):
    """-> (classes [runs, n], fault records [runs * flips, 9])"""
    tl = (C.c_int * max(len(layers), 1))(*layers)
    cnt, usec = C.c_int(0), C.c_float(0)
    p = L.bnn_mi355x_fault_campaigns(path.encode(), 10, runs, seed, flips, word_size, target, tl if layers else None, len(layers),
                                     C.byref(cnt), C.byref(usec))
    assert p, L.bnn_mi355x_last_error().decode()
    n = cnt.value
    got = np.ctypeslib.as_array(p, shape=(max(runs * n, 1),))[: runs * n].copy().reshape(runs, n)
    L.free_results(p)
    assert n == 0 or usec.value > 0
    k = L.bnn_mi355x_last_campaign_faults(None, 0)
    rec = (C.c_int * max(9 * k, 1))()
    assert L.bnn_mi355x_last_campaign_faults(rec, k) == k
    return got, np.array(rec[: 9 * k], np.int32).reshape(k, 9)


def sequential(L, pdir, path, seed, flips, word_size, target, layers=()):
    """one run the way the notebook's loop does it: reload, seed, one call -> (classes, fault records [flips, 8])"""
    L.load_parameters(pdir.encode())
    assert L.bnn_mi355x_set_fault_seed(seed) == 0
    tl = (C.c_int * max(len(layers), 1))(*layers)
    cnt = C.c_int(0)
    p = L.inference_multiple_with_faults(path.encode(), 10, C.byref(cnt), None, flips, word_size, target, tl if layers else None,
                                         len(layers))
    assert p, L.bnn_mi355x_last_error().decode()
    got = np.ctypeslib.as_array(p, shape=(max(cnt.value, 1),))[: cnt.value].copy()
    L.free_results(p)
    k = L.bnn_mi355x_last_faults(None, 0)
    rec = (C.c_int * max(8 * k, 1))()
    assert L.bnn_mi355x_last_faults(rec, k) == k
    return got, np.array(rec[: 8 * k], np.int32).reshape(k, 8)


def check_against_sequential(L, pdir, path, runs, seed, flips, word_size, target, layers=()):
    L.load_parameters(pdir.encode())
    got, recs = campaigns(L, path, runs, seed, flips, word_size, target, layers)
    for r in range(runs):
        want, want_recs = sequential(L, pdir, path, seed + r, flips, word_size, target, layers)
        mine = recs[recs[:, 0] == r]
        assert (mine[:, 1:] == want_recs).all() and len(mine) == len(want_recs), "run %d: fault records" % r
        assert got[r].tolist() == want.tolist(), "run %d: classes" % r
    L.load_parameters(pdir.encode())
    assert L.bnn_mi355x_set_fault_seed(0) == 0
    return got, recs


def oracle_replay(o, imgs, recs):
    """classes of one campaign replayed fault by fault (records of 8 ints, sorted by image)"""
    n = len(imgs)
    want = np.zeros(n, np.int32)
    k, start = 0, 0
    while start < n:
        while k < len(recs) and recs[k, 0] <= start:
            assert o.apply_fault(recs[k]) >= 0
            k += 1
        end = int(recs[k, 0]) if k < len(recs) else n
        want[start:end] = o.classes_batched(imgs[start:end], 10)
        start = end
    return want


def test_refusals_without_a_gpu():
    """argument checks come before anything touches the device: a run count outside 1 ... 4096 and a seed that wraps
    to 0 (the random_device seed) for some run are refused with NULL + last_error"""
    L = gl.load("cnvW1A1")
    cnt = C.c_int(0)
    for runs, seed in ((0, 5), (-1, 5), (4097, 5), (7, 2 ** 64 - 3), (2, 2 ** 64 - 1)):
        assert not L.bnn_mi355x_fault_campaigns(b"/nonexistent", 10, runs, seed, 10, 1, -1, None, 0, C.byref(cnt), None)
        assert L.bnn_mi355x_last_error().decode()
    assert L.bnn_mi355x_last_campaign_faults(None, 0) == 0


def test_variants_refused(variant_libs):
    """the hardened overlays' fault model is not modelled: refused like inference_multiple_with_faults refuses it"""
    L = gl.load("cnvW1A1-TMR")
    cnt = C.c_int(0)
    assert not L.bnn_mi355x_fault_campaigns(b"/nonexistent", 10, 3, 5, 10, 1, -1, None, 0, C.byref(cnt), None)
    assert b"not modelled" in L.bnn_mi355x_last_error()


@pytest.mark.gpu
@pytest.mark.parametrize("network,dataset", NETS, ids=lambda x: x)
@pytest.mark.parametrize("target,word_size", [(-1, 1), (0, 4), (1, 1)])
def test_runs_equal_the_sequential_calls(network, dataset, target, word_size, tmp_path):
    L = gl.load(network)
    pdir = gl.param_dir(dataset, network)
    _, path = write_images(network, 240, tmp_path)
    check_against_sequential(L, pdir, path, 7, 4321 + 10 * word_size + target, 60, word_size, target)


@pytest.mark.gpu
@pytest.mark.parametrize("network,dataset", [("cnvW1A2", "cifar10"), ("lfcW1A1", "mnist")], ids=lambda x: x)
def test_runs_replayed_in_oracle(network, dataset, tmp_path):
    L = gl.load(network)
    pdir = gl.param_dir(dataset, network)
    L.load_parameters(pdir.encode())
    imgs, path = write_images(network, 240, tmp_path)
    got, recs = campaigns(L, path, 5, 777, 60, 1, -1)
    for r in (1, 4):
        want = oracle_replay(ol.Oracle(network, pdir), imgs, recs[recs[:, 0] == r][:, 1:])
        assert got[r].tolist() == want.tolist()
    assert (got[1] != got[4]).any()  # (different faults, different classes)


@pytest.mark.gpu
def test_more_faults_than_images(tmp_path):
    """several faults before one image: empty segments in most waves"""
    L = gl.load("cnvW1A1")
    _, path = write_images("cnvW1A1", 20, tmp_path)
    _, recs = check_against_sequential(L, gl.param_dir("cifar10", "cnvW1A1"), path, 5, 99, 50, 1, -1)
    assert len(recs) == 250 and any(np.bincount(recs[recs[:, 0] == r][:, 1]).max() > 1 for r in range(5))


@pytest.mark.gpu
def test_wave_above_a_launch_is_split(tmp_path):
    """70 000 MNIST images x 4 runs, one fault each: a wave holds more images than one launch takes"""
    L = gl.load("lfcW1A1")
    _, path = write_images("lfcW1A1", 70000, tmp_path, seed=23)
    _, recs = check_against_sequential(L, gl.param_dir("mnist", "lfcW1A1"), path, 4, 5, 1, 1, 0)
    t = recs[:, 1]
    assert max(t.sum(), (70000 - t).sum()) > KMAX_CHUNK


@pytest.mark.gpu
def test_one_run_is_the_sequential_call(tmp_path):
    L = gl.load("lfcW1A2")
    _, path = write_images("lfcW1A2", 300, tmp_path)
    check_against_sequential(L, gl.param_dir("mnist", "lfcW1A2"), path, 1, 31, 40, 8, -1)


@pytest.mark.gpu
def test_minus_two_rows_in_some_runs_of_a_wave(tmp_path):
    """cnvW2A2 weight faults: a flip can turn a 2-bit weight into -2 (0b10), which only the -2-aware kernels
    evaluate right.  A wave in which some runs' copies hold such a row and others do not runs every run on
    those kernels: still exact for all of them"""
    network, dataset = "cnvW2A2", "cifar10"
    pdir = gl.param_dir(dataset, network)
    L = gl.load(network)
    runs, flips = 6, 2
    seed = None
    for s in range(1, 200):  # a seed whose runs disagree about -2 rows after their last fault (the last wave)
        has = [_holds_minus_two(network, pdir, _plan(L, s + r, 240, flips)) for r in range(runs)]
        if any(has) and not all(has):
            seed = s
            break
    assert seed is not None
    _, path = write_images(network, 240, tmp_path)
    check_against_sequential(L, pdir, path, runs, seed, flips, 1, 0)


def _plan(L, seed, n_images, flips):
    rec = (C.c_int * (8 * flips))()
    k = L.bnn_mi355x_plan_faults(seed, n_images, flips, 1, 0, None, 0, rec, flips)
    assert k == flips
    return np.array(rec[:], np.int32).reshape(flips, 8)


def _holds_minus_two(network, pdir, recs):
    """after these faults (oracle): does a row they touched hold a weight of -2"""
    o = ol.Oracle(network, pdir)
    rows = set()
    for rec in recs:
        row = o.apply_fault(rec)
        assert row >= 0
        rows.add((int(rec[2]), row))
    return any(o.L.bnn_oracle_weight(o.h, l, row, j) == -2 for l, row in rows for j in range(o.L.bnn_oracle_layer_mw(o.h, l)))


@pytest.mark.gpu
def test_loaded_parameters_untouched(tmp_path):
    network, dataset = "cnvW1A1", "cifar10"
    L = gl.load(network)
    pdir = gl.param_dir(dataset, network)
    L.load_parameters(pdir.encode())
    imgs, path = write_images(network, 240, tmp_path)
    crc = L.bnn_mi355x_params_crc()
    campaigns(L, path, 9, 11, 80, 1, -1)
    assert L.bnn_mi355x_params_crc() == crc
    cnt = C.c_int(0)
    p = L.inference_multiple(path.encode(), 10, C.byref(cnt), None, 0)
    again = np.ctypeslib.as_array(p, shape=(cnt.value,)).copy()
    L.free_results(p)
    assert again.tolist() == ol.Oracle(network, pdir).classes_batched(imgs, 10).tolist()
    # no faults: the fault-free classes once per run
    got, recs = campaigns(L, path, 3, 11, 0, 1, -1)
    assert len(recs) == 0 and all(row.tolist() == again.tolist() for row in got)


@pytest.mark.gpu
def test_imported_blob_refused(tmp_path):
    network, dataset = "lfcW1A1", "mnist"
    L = gl.load(network)
    blob = gl.pack_params(network, gl.param_dir(dataset, network))
    assert L.bnn_mi355x_import_params(blob.ctypes.data, blob.size) == 0
    _, path = write_images(network, 50, tmp_path)
    cnt = C.c_int(0)
    assert not L.bnn_mi355x_fault_campaigns(path.encode(), 10, 3, 5, 10, 1, -1, None, 0, C.byref(cnt), None)
    assert b"imported blob" in L.bnn_mi355x_last_error()
    L.load_parameters(gl.param_dir(dataset, network).encode())


@pytest.mark.gpu
def test_fault_test_batched_equals_sequential(tmp_path):
    import bnn
    from bnn.faults import faults
    imgs, path = write_images("cnvW1A1", 200, tmp_path)
    labels = list(np.random.default_rng(3).integers(0, 10, 200))
    ft = faults.CNVFaultTest("cnvW1A1", "cifar10", path, labels, bnn.RUNTIME_SW)
    seq = ft.run_test(4, 30, 1, -1, (), batched=False, seed=1000)
    bat = ft.run_test(4, 30, 1, -1, (), batched=True, seed=1000)
    assert seq[0] == bat[0] and seq[2] == bat[2] and len(bat[1]) == 4
    assert len({tuple(r) for r in bat[0]}) > 1


# Multi-run launches choose their groups per block from the launch's image count (run_cnv_multi_t, gpb_for over
# total x items per image): the campaigns below put a launch on each side of every change point of that choice
# (dispatch_forms.multi_forms), one flip per run, so that wave 0 classifies sum(t) images and wave 1 runs x images - sum(t)
# (t: the runs' fault times).  (runs, images, seed) -> the two wave totals, checked from the returned records; the last
# campaign's waves hold more than a launch takes and are cut at 131 072.
MULTI_CAMPAIGNS = [(4, 1337, 2368, (2673, 2675)), (7, 4159, 5410, (14557, 14556)), (7, 5989, 15395, (20962, 20961)),
                   (27, 4313, 2581, (58226, 58225)), (64, 4500, 1, (152194, 135806))]
MULTI_SETS = [("cnvW1A1", "cifar10"), ("cnvW1A2", "cifar10"), ("cnvW2A2", "cifar10"), ("cnvW2A2", None)]


def launch_totals(wave_totals, cap):
    return [min(cap, w - b) for w in wave_totals for b in range(0, w, cap)]


def test_multi_campaigns_straddle_every_edge():
    import dispatch_forms as df
    edges = df.edges(df.multi_forms)
    totals = set()
    for runs, n, _, waves in MULTI_CAMPAIGNS:
        totals |= set(launch_totals(waves, min(KMAX_CHUNK, runs * n)))
    assert all(e - 1 in totals or e - 2 in totals for e in edges) and all(e in totals or e + 1 in totals for e in edges)
    assert launch_totals((152194, 135806), KMAX_CHUNK) == [131072, 21122, 131072, 4734]


@pytest.mark.gpu
@pytest.mark.parametrize("network,dataset", MULTI_SETS, ids=lambda x: x or "neg2")
def test_multi_run_forms_at_every_edge(network, dataset, tmp_path):
    """every run of each campaign equal to its sequential call; for the random -2 set of cnvW2A2 (dataset None) every
    wave takes the -2-aware kernels, its base parameters holding -2 rows"""
    L = gl.load(network)
    if dataset:
        pdir = gl.param_dir(dataset, network)
    else:
        import random_params
        pdir = str(tmp_path / "neg2")
        random_params.make(pdir, network, 5, neg2=0.03)
        assert (ol.Oracle(network, pdir).weights(1) == -2).any()
    try:
        for runs, n, seed, waves in MULTI_CAMPAIGNS:
            imgs, path = write_images(network, n, tmp_path, seed=n)
            got, recs = check_against_sequential(L, pdir, path, runs, seed, 1, 1, 0)
            assert len(recs) == runs and sorted(recs[:, 0].tolist()) == list(range(runs))
            t = int(recs[:, 1].sum())
            assert (t, runs * n - t) == waves, (runs, n, seed)
            if network == "cnvW1A2" and runs == 4:  # two runs replayed fault by fault in the restatement
                for r in (0, 3):
                    want = oracle_replay(ol.Oracle(network, pdir), imgs, recs[recs[:, 0] == r][:, 1:])
                    assert got[r].tolist() == want.tolist()
    finally:
        L.load_parameters(gl.param_dir("cifar10", network).encode())
