"""Exhaustive single-fault sweeps on the GPU (bnn_mi355x_fault_sweep): every record alone, on every image.  Each
fault's changed images and their classes must be exactly what the dense route gives -- pack_params_faulty +
import_params + inference_buffer, one fault at a time -- and, for a sample, what the CPU restatement gives with
apply_fault; whatever the grouping of records into run groups, windows and launches, and whatever the pruning
dropped."""
import ctypes as C
import os
import struct
import sys

import numpy as np
import pytest

import gpu_lib as gl
import oracle_lib as ol

sys.path.insert(0, os.path.join(gl.ROOT, "bnn-pynq_amd"))
from bnn import params_io  # noqa: E402

NETS = [("cnvW1A1", "cifar10"), ("cnvW1A2", "cifar10"), ("cnvW2A2", "cifar10"), ("lfcW1A1", "mnist"), ("lfcW1A2", "mnist")]
KMAX_RUNS = 4096  # runtime.hip, kMaxRuns
ip = C.POINTER(C.c_int)
pytestmark = pytest.mark.gpu


def golden_images(network):
    if network.startswith("cnv"):
        names = ["deer.cifar", "car.cifar", "six.cifar", "stop.cifar", "road_stop.cifar", "road_cross.cifar"]
        return np.concatenate([ol.read_cifar(os.path.join(ol.GOLDEN, f)) for f in names])
    return ol.read_mnist(os.path.join(ol.GOLDEN, "3.image-idx3-ubyte"))


def write_images(network, imgs, tmp_path, name="imgs"):
    n = len(imgs)
    if network.startswith("cnv"):
        path = tmp_path / (name + ".bin")
        np.concatenate([np.ones((n, 1), np.uint8), imgs], axis=1).tofile(path)
    else:
        path = tmp_path / (name + "-idx3-ubyte")
        with open(path, "wb") as f:
            f.write(struct.pack(">4I", 0x803, n, 28, 28) + imgs.tobytes())
    return str(path)


def images(network, n, tmp_path, seed=29, golden=True):
    isz = 3072 if network.startswith("cnv") else 784
    imgs = np.random.default_rng(seed).integers(0, 256, (n, isz), dtype=np.uint8)
    if golden:
        imgs = np.concatenate([imgs, golden_images(network)])
    return imgs, write_images(network, imgs, tmp_path)


def enumerate_faults(L, layer, target, ws):
    k = L.bnn_mi355x_enumerate_faults(layer, target, ws, 0, None, 0)
    assert k >= 0
    rec = np.zeros((max(k, 1), 8), np.int32)
    L.bnn_mi355x_enumerate_faults(layer, target, ws, 0, rec.ctypes.data_as(ip), k)
    return rec[:k]


def sample(L, network, per, seed=5, word_sizes=(1, 2, 8), layers=None):
    """`per` records of every (layer, target, word size) that has faults"""
    rng = np.random.default_rng(seed)
    out = []
    for layer in layers if layers is not None else range(len(params_io.layout(network))):
        for target in (0, 1):
            for ws in word_sizes:
                rec = enumerate_faults(L, layer, target, ws)
                if len(rec):
                    out.append(rec[rng.choice(len(rec), min(per, len(rec)), replace=False)])
    return np.concatenate(out)


def sweep(L, path, recs, cap=None, ncls=10):
    """-> (changed [k], diffs [m, 3], total, n, usec)"""
    recs = np.ascontiguousarray(recs, np.int32)
    k = len(recs)
    changed = np.full(max(k, 1), -7, np.int32)
    cap = k * 200000 if cap is None else cap
    cap = min(cap, 1 << 24)
    diffs = np.zeros((max(cap, 1), 3), np.int32)
    cnt, usec = C.c_int(0), C.c_float(0)
    total = L.bnn_mi355x_fault_sweep(path.encode(), ncls, recs.ctypes.data_as(ip), k, changed.ctypes.data_as(ip),
                                     diffs.ctypes.data_as(ip), cap, C.byref(cnt), C.byref(usec))
    assert total >= 0, L.bnn_mi355x_last_error().decode()
    return changed[:k], diffs[:min(cap, total)], total, cnt.value, usec.value


def stages(L):
    s = L.bnn_mi355x_last_sweep_stages(None, 0)
    out = (C.c_long * max(s, 1))()
    assert L.bnn_mi355x_last_sweep_stages(out, s) == s
    return np.array(out[:s], np.int64)


def classes(L, imgs, ncls=10):
    n = len(imgs)
    p = L.bnn_mi355x_inference_buffer(np.ascontiguousarray(imgs).ctypes.data, n, ncls, None, 0)
    assert p, L.bnn_mi355x_last_error().decode()
    out = np.ctypeslib.as_array(p, shape=(n,)).astype(np.int32, copy=True)
    L.free_results(p)
    return out


def dense(L, pdir, imgs, recs, ncls=10):
    """per fault, the whole classification with the faulty parameters: (changed [k], diffs [m, 3]); leaves the
    library with `pdir` loaded again"""
    L.load_parameters(pdir.encode())
    clean = classes(L, imgs, ncls)
    nb = L.bnn_mi355x_pack_params(pdir.encode(), None, 0)
    blob = np.zeros(nb, np.uint8)
    changed, diffs = [], []
    for f, r in enumerate(np.ascontiguousarray(recs, np.int32)):
        assert L.bnn_mi355x_pack_params_faulty(pdir.encode(), r.ctypes.data_as(ip), 1, blob.ctypes.data, nb) == nb
        assert L.bnn_mi355x_import_params(blob.ctypes.data, nb) == 0, L.bnn_mi355x_last_error().decode()
        got = classes(L, imgs, ncls)
        idx = np.nonzero(got != clean)[0]
        changed.append(len(idx))
        diffs.extend([f, int(i), int(got[i])] for i in idx)
    L.load_parameters(pdir.encode())
    return np.array(changed, np.int32), np.array(diffs, np.int32).reshape(-1, 3), clean


def oracle_changed(network, pdir, imgs, rec, clean, ncls=10):
    o = ol.Oracle(network, pdir)
    assert o.apply_fault(rec) >= 0
    got = o.classes_batched(imgs, ncls)
    o.close()
    idx = np.nonzero(got != clean)[0]
    return [[int(i), int(got[i])] for i in idx]


@pytest.mark.parametrize("network,dataset", NETS, ids=lambda x: x)
def test_sweep_equals_dense(network, dataset, tmp_path):
    """~256 records over every layer, both targets, word sizes 1, 2, 8, on 300 random images plus the golden ones;
    16 of them also against the CPU restatement.  The loaded parameters (CRC) and a following classification are
    unchanged by the sweep."""
    L = gl.load(network)
    pdir = gl.param_dir(dataset, network)
    L.load_parameters(pdir.encode())
    imgs, path = images(network, 300, tmp_path)
    nl = len(params_io.layout(network))
    recs = sample(L, network, 10 if nl == 4 else 5)
    assert 200 <= len(recs) <= 300
    crc = L.bnn_mi355x_params_crc()
    before = classes(L, imgs)
    changed, diffs, total, n, usec = sweep(L, path, recs)
    assert n == len(imgs) and usec > 0 and total == changed.sum() == len(diffs)
    assert L.bnn_mi355x_params_crc() == crc
    assert (classes(L, imgs) == before).all()
    want_changed, want_diffs, clean = dense(L, pdir, imgs, recs)
    assert (clean == before).all()
    assert changed.tolist() == want_changed.tolist()
    assert diffs.tolist() == want_diffs.tolist()
    assert (changed == 0).any() and (changed > 0).any()
    rng = np.random.default_rng(3)
    for f in rng.choice(len(recs), 16, replace=False):
        assert diffs[diffs[:, 0] == f][:, 1:].tolist() == oracle_changed(network, pdir, imgs, recs[f], clean), recs[f]


def test_cnvW2A2_faults_that_create_minus_two(tmp_path):
    """2-bit weights: a word flip of both bits of a +1 weight (01 -> 10) makes it -2, which only the -2-aware kernels
    compute; such records, mixed with others, give the dense results"""
    network, dataset = "cnvW2A2", "cifar10"
    L = gl.load(network)
    pdir = gl.param_dir(dataset, network)
    o = ol.Oracle(network, pdir)
    lay = params_io.layout(network)
    rng = np.random.default_rng(8)
    picked = []
    for layer in range(1, 9):
        rec = enumerate_faults(L, layer, 0, 2)
        got = 0
        for r in rec[rng.choice(len(rec), 400, replace=False)]:
            P = lay[layer]
            row = (r[4] // (P["wmem"] // P["tmem"])) * P["pe"] + r[3]
            col = (r[4] % (P["wmem"] // P["tmem"])) * P["simd"] + r[6] // 2
            assert o.apply_fault(r) >= 0
            w = o.L.bnn_oracle_weight(o.h, layer, int(row), int(col))
            assert o.apply_fault(r) >= 0  # (a weight flip undoes itself)
            if w == -2:
                picked.append(r)
                got += 1
            if got == 3:
                break
    o.close()
    assert len(picked) >= 8
    recs = np.concatenate([np.array(picked), sample(L, network, 1, seed=9, word_sizes=(1,))])
    L.load_parameters(pdir.encode())
    imgs, path = images(network, 200, tmp_path)
    changed, diffs, total, _, _ = sweep(L, path, recs)
    want_changed, want_diffs, clean = dense(L, pdir, imgs, recs)
    assert changed.tolist() == want_changed.tolist() and diffs.tolist() == want_diffs.tolist()
    assert changed[:len(picked)].sum() > 0


def test_no_change_and_every_change(tmp_path):
    """the top bit of a layer-7 threshold turns its neuron on or off for every image: some such faults change no
    image; the one that changes the most changes EVERY image of the set of images it changes (re-swept on those)"""
    network, dataset = "cnvW1A1", "cifar10"
    L = gl.load(network)
    pdir = gl.param_dir(dataset, network)
    L.load_parameters(pdir.encode())
    imgs, path = images(network, 120, tmp_path, golden=False)
    rec = enumerate_faults(L, 7, 1, 1)
    top = rec[rec[:, 6] == 15]
    changed, diffs, _, n, _ = sweep(L, path, top)
    zero = np.nonzero(changed == 0)[0]
    f = int(np.argmax(changed))
    assert len(zero) and changed[f] > 0
    sub = imgs[diffs[diffs[:, 0] == f][:, 1]]
    path2 = write_images(network, sub, tmp_path, "sub")
    pick = np.concatenate([[f], zero[:3]])
    c2, d2, _, n2, _ = sweep(L, path2, top[pick])
    assert n2 == len(sub) and c2[0] == n2 and (c2[1:] == 0).all()
    want_changed, want_diffs, _ = dense(L, pdir, sub, top[pick])
    assert c2.tolist() == want_changed.tolist() and d2.tolist() == want_diffs.tolist()


def test_cap_below_total(tmp_path):
    """diffs are the first cap_diffs of the (fault, image) order; the return value is still the total"""
    network, dataset = "lfcW1A1", "mnist"
    L = gl.load(network)
    L.load_parameters(gl.param_dir(dataset, network).encode())
    _, path = images(network, 200, tmp_path)
    recs = sample(L, network, 30, seed=2)
    changed, diffs, total, _, _ = sweep(L, path, recs)
    assert total > 10
    for cap in (1, total // 3, total - 1, total):
        c2, d2, t2, _, _ = sweep(L, path, recs, cap=cap)
        assert t2 == total and c2.tolist() == changed.tolist()
        assert d2.tolist() == diffs[:cap].tolist()
    c0, d0, t0, _, _ = sweep(L, path, recs, cap=0)
    assert t0 == total and len(d0) == 0 and c0.tolist() == changed.tolist()


@pytest.mark.parametrize("k", [KMAX_RUNS - 1, KMAX_RUNS, KMAX_RUNS + 1])
def test_run_group_edges(k, tmp_path):
    """kMaxRuns - 1 / kMaxRuns / kMaxRuns + 1 records on 8 images (one or two run groups): the same as the records in
    calls of 97, and a sample against the dense route"""
    network, dataset = "cnvW1A1", "cifar10"
    L = gl.load(network)
    pdir = gl.param_dir(dataset, network)
    L.load_parameters(pdir.encode())
    imgs, path = images(network, 8, tmp_path, golden=False)
    rec = enumerate_faults(L, 1, 0, 1)
    recs = rec[np.random.default_rng(k).choice(len(rec), k, replace=False)]
    changed, diffs, _, _, _ = sweep(L, path, recs)
    parts = [sweep(L, path, recs[i:i + 97]) for i in range(0, k, 97)]
    assert changed.tolist() == np.concatenate([p[0] for p in parts]).tolist()
    assert diffs.tolist() == np.concatenate([p[1] + [i * 97, 0, 0] for i, p in enumerate(parts)]).tolist()
    pick = np.concatenate([np.arange(4), np.arange(k - 4, k)])
    want_changed, want_diffs, _ = dense(L, pdir, imgs, recs[pick])
    assert changed[pick].tolist() == want_changed.tolist()


def test_workspace_cut(tmp_path):
    """1 000 images x 200 layer-1 faults: more pairs than one run group's workspace holds (groups of ~131 runs), the
    same as calls of 40 records (one group each)"""
    network, dataset = "cnvW1A2", "cifar10"
    L = gl.load(network)
    pdir = gl.param_dir(dataset, network)
    L.load_parameters(pdir.encode())
    imgs, path = images(network, 1000, tmp_path, golden=False)
    rec = enumerate_faults(L, 1, 0, 1)
    recs = rec[np.random.default_rng(4).choice(len(rec), 200, replace=False)]
    changed, diffs, _, _, _ = sweep(L, path, recs)
    parts = [sweep(L, path, recs[i:i + 40]) for i in range(0, 200, 40)]
    assert changed.tolist() == np.concatenate([p[0] for p in parts]).tolist()
    assert diffs.tolist() == np.concatenate([p[1] + [i * 40, 0, 0] for i, p in enumerate(parts)]).tolist()
    want_changed, want_diffs, _ = dense(L, pdir, imgs, recs[:6])
    assert changed[:6].tolist() == want_changed.tolist()


def test_image_windows(tmp_path):
    """more images than one pass holds (133 072 MNIST images): a run group covers them in windows"""
    network, dataset = "lfcW1A1", "mnist"
    L = gl.load(network)
    pdir = gl.param_dir(dataset, network)
    L.load_parameters(pdir.encode())
    imgs, path = images(network, 133072, tmp_path, golden=False)
    recs = np.concatenate([enumerate_faults(L, 0, 1, 1)[[15, 31]], enumerate_faults(L, 2, 0, 8)[[5]]])
    changed, diffs, _, n, _ = sweep(L, path, recs)
    assert n == 133072
    want_changed, want_diffs, _ = dense(L, pdir, imgs, recs)
    assert changed.tolist() == want_changed.tolist() and diffs.tolist() == want_diffs.tolist()
    assert (diffs[:, 1] >= 131072).any()  # (the second window's images are reached)


@pytest.mark.parametrize("network,dataset", [("cnvW1A1", "cifar10"), ("lfcW1A2", "mnist")], ids=lambda x: x)
def test_interleaved_layers(network, dataset, tmp_path):
    """records of several layers, shuffled, in one call = one call per layer"""
    L = gl.load(network)
    L.load_parameters(gl.param_dir(dataset, network).encode())
    _, path = images(network, 150, tmp_path)
    recs = sample(L, network, 6, seed=21)
    recs = recs[np.random.default_rng(1).permutation(len(recs))]
    changed, diffs, _, _, _ = sweep(L, path, recs)
    want_c = np.zeros(len(recs), np.int32)
    want_d = []
    for layer in np.unique(recs[:, 2]):
        idx = np.nonzero(recs[:, 2] == layer)[0]
        c, d, _, _, _ = sweep(L, path, recs[idx])
        want_c[idx] = c
        want_d.extend([int(idx[f]), int(i), int(k)] for f, i, k in d)
    assert changed.tolist() == want_c.tolist()
    assert diffs.tolist() == sorted(want_d)


def test_pruning(tmp_path):
    """faults in the FC layer 7 of cnvW1A1: no pair runs before layer 7, every pair at 7, and far fewer at 8 -- with
    the dense results"""
    network, dataset = "cnvW1A1", "cifar10"
    L = gl.load(network)
    pdir = gl.param_dir(dataset, network)
    L.load_parameters(pdir.encode())
    imgs, path = images(network, 300, tmp_path)
    recs = sample(L, network, 24, seed=13, word_sizes=(1,), layers=[7])
    recs = recs[recs[:, 1] == 0]
    changed, diffs, _, n, _ = sweep(L, path, recs)
    st = stages(L)
    assert len(st) == 9
    assert (st[:7] == 0).all() and st[7] == len(recs) * n
    assert st[8] < st[7] // 2
    want_changed, want_diffs, _ = dense(L, pdir, imgs, recs)
    assert changed.tolist() == want_changed.tolist() and diffs.tolist() == want_diffs.tolist()
    # a layer-1 sweep runs every later layer too, its pairs never more than at layer 1
    sweep(L, path, enumerate_faults(L, 1, 0, 1)[:20])
    st = stages(L)
    assert st[0] == 0 and st[1] == 20 * n and (st[2:] <= st[1]).all()


def test_refusals(tmp_path):
    """an imported blob, BNN_MI355X_L1=mfma, a record outside its layer's memories: -1 and last_error"""
    network, dataset = "cnvW1A1", "cifar10"
    L = gl.load(network)
    pdir = gl.param_dir(dataset, network)
    _, path = images(network, 16, tmp_path, golden=False)
    good = enumerate_faults(L, 3, 0, 1)[:2]
    L.load_parameters(pdir.encode())
    for bad in ([0, 0, 1, 99, 0, 0, 0, 1], [0, 0, 1, 0, 0, 0, 64, 1], [0, 1, 8, 0, 0, 0, 0, 1], [0, 0, 9, 0, 0, 0, 0, 1],
                [0, 0, 1, 0, 0, 0, 0, 0], [0, 2, 1, 0, 0, 0, 0, 1], [0, 1, 1, 0, 0, 3, 0, 1]):
        recs = np.concatenate([good, np.array([bad], np.int32)])
        ch = np.zeros(3, np.int32)
        assert L.bnn_mi355x_fault_sweep(path.encode(), 10, recs.ctypes.data_as(ip), 3, ch.ctypes.data_as(ip), None, 0, None, None) == -1
        assert b"record 2" in L.bnn_mi355x_last_error(), bad
    nb = L.bnn_mi355x_params_bytes()
    blob = np.zeros(nb, np.uint8)
    assert L.bnn_mi355x_export_params(blob.ctypes.data, nb) == nb
    assert L.bnn_mi355x_import_params(blob.ctypes.data, nb) == 0
    ch = np.zeros(2, np.int32)
    assert L.bnn_mi355x_fault_sweep(path.encode(), 10, good.ctypes.data_as(ip), 2, ch.ctypes.data_as(ip), None, 0, None, None) == -1
    assert b"imported blob" in L.bnn_mi355x_last_error()
    os.environ["BNN_MI355X_L1"] = "mfma"
    try:
        L.load_parameters(pdir.encode())
        assert L.bnn_mi355x_fault_sweep(path.encode(), 10, good.ctypes.data_as(ip), 2, ch.ctypes.data_as(ip), None, 0, None, None) == -1
        assert b"BNN_MI355X_L1" in L.bnn_mi355x_last_error()
    finally:
        del os.environ["BNN_MI355X_L1"]
        L.load_parameters(pdir.encode())
    c, _, _, _, _ = sweep(L, path, good)
    assert len(c) == 2


def test_sensitivity_accuracies(tmp_path):
    """FaultTest.sensitivity on lfcW1A1 layer 3 weights: every fault's accuracy is the one its full classes give
    (rebuilt from the fault-free classes and its diffs for all faults, from the dense route for a sample)"""
    from bnn.faults import faults
    from bnn import bnn as B
    network, dataset = "lfcW1A1", "mnist"
    imgs, path = images(network, 250, tmp_path)
    labels = np.random.default_rng(77).integers(0, 10, len(imgs)).tolist()
    ft = faults.LFCFaultTest(network, dataset, path, labels)
    recs, changed, acc = ft.sensitivity([3], 0, 1)
    L = gl.load(network)
    assert len(recs) == L.bnn_mi355x_enumerate_faults(3, 0, 1, 0, None, 0)
    clf = B.LfcClassifier(network, dataset)
    clean = clf.classify_mnists(path)
    c2, diffs = clf.classify_mnists_fault_sweep(path, recs)
    assert c2.tolist() == changed.tolist()
    lab = np.array(labels)
    start = np.searchsorted(diffs[:, 0], np.arange(len(recs) + 1))
    for f in range(len(recs)):
        cls = clean.copy()
        d = diffs[start[f]:start[f + 1]]
        cls[d[:, 1]] = d[:, 2]
        assert acc[f] == pytest.approx(100.0 * (cls == lab).sum() / len(lab), abs=1e-9)
    assert ft.control_accuracy == pytest.approx(100.0 * (clean == lab).sum() / len(lab))
    pick = np.argsort(-changed)[:6]
    pdir = gl.param_dir(dataset, network)
    _, want_diffs, want_clean = dense(L, pdir, imgs, recs[pick])
    for j, f in enumerate(pick):
        cls = want_clean.copy()
        d = want_diffs[want_diffs[:, 0] == j]
        cls[d[:, 1]] = d[:, 2]
        assert acc[f] == pytest.approx(100.0 * (cls == lab).sum() / len(lab), abs=1e-9)
