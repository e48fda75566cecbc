"""Activation-fault sweeps on the GPU (bnn_mi355x_act_fault_sweep): every record -- one activation of a layer's
output changed to another level -- alone, on every image.  Each record's changed images and their classes must be
exactly what an independent numpy restatement gives: the network from the faulted activations on, layer by layer,
from the oracle's weights and thresholds (bnn_oracle_weight / bnn_oracle_threshold), decoded with the oracle's
batched decoders."""
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
CNV_MAPS = [(30, 30, 64), (14, 14, 64), (12, 12, 128), (5, 5, 128), (3, 3, 256), (1, 1, 256), (1, 1, 512), (1, 1, 512)]
LFC_MAPS = [(1, 1, 1024)] * 3
ip = C.POINTER(C.c_int)
pytestmark = pytest.mark.gpu


class Restatement:
    """layers L+1 ... of one network on value-domain activations [batch, h * w * c] (HWC), from the oracle's matrices:
    an im2col in (ky, kx, c) column order for the 3x3 convolutions, a 2x2 max-pool after CNV layers 1 and 3, an XNOR
    popcount (1-bit nets) or a signed sum, then `thr < acc` against each threshold"""

    def __init__(self, network, pdir):
        self.o = ol.Oracle(network, pdir)
        o, lib = self.o, self.o.L
        self.cnv, self.a1 = o.is_cnv, network.endswith("A1")
        self.maps = CNV_MAPS if self.cnv else LFC_MAPS
        layout = params_io.layout(network)
        W, _ = params_io.read_params(pdir, network)  # (fast to read; every entry used is checked against the oracle below)
        self.W, self.T = [], []
        rng = np.random.default_rng(1)
        for l in range(o.nl):
            mh, mw = lib.bnn_oracle_layer_mh(o.h, l), lib.bnn_oracle_layer_mw(o.h, l)
            w = W[l][:mh, :mw]
            for n, j in zip(rng.integers(0, mh, 300), rng.integers(0, mw, 300)):
                assert w[n, j] == lib.bnn_oracle_weight(o.h, l, int(n), int(j)), (l, n, j)
            nthr = layout[l]["nthr"]
            self.T.append(np.array([[lib.bnn_oracle_threshold(o.h, l, n, i) for i in range(nthr)] for n in range(mh)], np.int64))
            self.W.append(np.ascontiguousarray(w.T, np.float32))  # [mw, mh]: exact in float32 (|acc| < 2^24)

    def layer(self, l, x):
        """x [b, elements] int8 -> layer l's output [b, elements] int8, or (last layer) raw accumulators [b, mh]"""
        b = x.shape[0]
        if self.cnv and l <= 4:
            h, w, c = self.maps[l - 1]
            win = np.lib.stride_tricks.sliding_window_view(x.reshape(b, h, w, c), (3, 3), axis=(1, 2))  # [b, oy, ox, c, ky, kx]
            od = h - 2
            cols = win.transpose(0, 1, 2, 4, 5, 3).reshape(b * od * od, 9 * c)
        else:
            od, cols = 1, x
        dot = np.rint(cols.astype(np.float32) @ self.W[l]).astype(np.int64)
        acc = (self.W[l].shape[0] + dot) // 2 if self.a1 else dot  # XNOR: matches = (mw + signed sum) / 2
        if l == len(self.W) - 1:
            return acc
        T = self.T[l]
        y = (-1 + sum((T[None, :, i] < acc).astype(np.int64) for i in range(T.shape[1]))) if T.shape[1] == 2 else \
            np.where(T[None, :, 0] < acc, 1, -1)
        mh = T.shape[0]
        y = y.astype(np.int8).reshape(b, od, od, mh)
        if self.cnv and l in (1, 3):
            y = y.reshape(b, od // 2, 2, od // 2, 2, mh).max(axis=(2, 4))
        return y.reshape(b, -1)


def lfc_last(rs, acc):
    T = rs.T[-1]
    return np.where(T[None, :, 0] < acc, 1, -1)


def restate(rs, base, recs, ncls=10):
    """per record: (changed, diffs [m, 3]) from the restatement"""
    n = base[0].shape[0]
    changed = np.zeros(len(recs), np.int64)
    diffs = []
    levels = 2 if rs.a1 else 3
    clean = classes_of(rs, len(base) - 1, base[-1], ncls)
    for L in sorted(set(int(r[0]) for r in recs)):
        idx = [f for f, r in enumerate(recs) if r[0] == L]
        h, w, c = rs.maps[L]
        x = np.repeat(base[L][None], len(idx), axis=0)  # [k, n, elements]
        for k, f in enumerate(idx):
            _, y, xx, ch, shift = (int(v) for v in recs[f])
            e = (y * w + xx) * c + ch
            i = (x[k, :, e].astype(np.int64) + 1) // (2 if levels == 2 else 1)
            i = (i + shift) % levels
            x[k, :, e] = (2 * i - 1) if levels == 2 else (i - 1)
        cls = classes_of(rs, L, x.reshape(len(idx) * n, -1), ncls).reshape(len(idx), n)
        for k, f in enumerate(idx):
            ch_img = np.nonzero(cls[k] != clean)[0]
            changed[f] = len(ch_img)
            diffs.extend([f, int(j), int(cls[k, j])] for j in ch_img)
    diffs.sort()
    return changed, np.array(diffs, np.int64).reshape(-1, 3)


def classes_of(rs, L, x, ncls):
    """layer L's outputs x [b, elements] -> classes [b], 64 rows at a time (the im2col of layer 1 is large)"""
    if len(x) > 64:
        return np.concatenate([classes_of(rs, L, x[i:i + 64], ncls) for i in range(0, len(x), 64)])
    for l in range(L + 1, len(rs.W)):
        x = rs.layer(l, x)
    lib = rs.o.L
    if rs.cnv:
        s = (x & 0xFFFF).astype(np.uint16).view(np.int16)
        return np.array([lib.bnn_oracle_decode_cnv_batched(np.ascontiguousarray(r).ctypes.data_as(C.POINTER(C.c_int16)), ncls)
                         for r in s], np.int64)
    bits = lfc_last(rs, x) > 0
    words = (bits[:, :64].astype(np.uint64) << np.arange(64, dtype=np.uint64)).sum(axis=1, dtype=np.uint64)
    return np.array([lib.bnn_oracle_decode_lfc_batched(int(wd), ncls) for wd in words], np.int64)


def fault_free(rs, imgs):
    """every layer's fault-free output: layer 0 from the oracle's layer_ref, the rest restated"""
    x = np.stack([rs.o.layer_ref(i, 0) for i in imgs])
    outs = [x]
    for l in range(1, len(rs.W) - 1):
        x = rs.layer(l, x)
        outs.append(x)
    return outs


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


def images(network, n, seed=31):
    isz = 3072 if network.startswith("cnv") else 784
    return np.random.default_rng(seed).integers(0, 256, (n, isz), dtype=np.uint8)


def enumerate_act(L, layer):
    k = L.bnn_mi355x_enumerate_act_faults(layer, 0, None, 0)
    assert k > 0, L.bnn_mi355x_last_error()
    rec = np.zeros((k, 5), np.int32)
    L.bnn_mi355x_enumerate_act_faults(layer, 0, rec.ctypes.data_as(ip), k)
    return rec


def sweep(L, path, recs, cap=None, ncls=10):
    """-> (changed [k], diffs [m, 3], total, n)"""
    recs = np.ascontiguousarray(recs, np.int32)
    k = len(recs)
    changed = np.full(max(k, 1), -7, np.int32)
    cap = min(k * 200000 if cap is None else cap, 1 << 24)
    diffs = np.zeros((max(cap, 1), 3), np.int32)
    cnt, usec = C.c_int(0), C.c_float(0)
    total = L.bnn_mi355x_act_fault_sweep(path.encode(), ncls, recs.ctypes.data_as(ip), k, changed.ctypes.data_as(ip),
                                         diffs.ctypes.data_as(ip), cap, C.byref(cnt), C.byref(usec))
    assert total >= 0, L.bnn_mi355x_last_error().decode()
    return changed[:k], diffs[:min(cap, total)], total, cnt.value


def act_stages(L):
    s = L.bnn_mi355x_last_act_sweep_stages(None, 0)
    out = (C.c_long * max(s, 1))()
    assert L.bnn_mi355x_last_act_sweep_stages(out, s) == s
    return np.array(out[:s], np.int64)


def sample_sites(L, network, rng, per=3):
    """per non-last layer: the map's corners and the channel-word edges (c = 0, 31, 32, 63, 64, C-1), plus `per` random
    sites, every shift of each"""
    maps = CNV_MAPS if network.startswith("cnv") else LFC_MAPS
    levels = 3 if network.endswith("A2") else 2
    out = []
    for layer, (h, w, c) in enumerate(maps):
        pts = {(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)}
        chans = sorted({0, 31, 32, 63, 64, c - 1} & set(range(c)))
        sites = [(y, x, chans[k % len(chans)]) for k, (y, x) in enumerate(sorted(pts))]
        sites += [(0, 0, ch) for ch in chans]
        sites += [(int(rng.integers(h)), int(rng.integers(w)), int(rng.integers(c))) for _ in range(per)]
        for (y, x, ch) in dict.fromkeys(sites):
            out.extend([layer, y, x, ch, s] for s in range(1, levels))
    return np.array(out, np.int32)


@pytest.fixture(scope="module")
def shipped_and_random(tmp_path_factory):
    import random_params
    sets = {}
    for k, (network, dataset) in enumerate(NETS):
        d = tmp_path_factory.mktemp("rp_" + network)
        random_params.make(str(d), network, 71 + k)
        sets[network] = [gl.param_dir(dataset, network), str(d)]
    return sets


def test_restatement_self_check(shipped_and_random):
    """with no fault the restatement reproduces layer_ref at every layer and the oracle's scores / words at the end"""
    for network, _ in NETS:
        for pdir in shipped_and_random[network]:
            rs = Restatement(network, pdir)
            imgs = images(network, 6, seed=5)
            base = fault_free(rs, imgs[:1])
            for l, x in enumerate(base):
                assert (x[0] == rs.o.layer_ref(imgs[0], l)).all(), (network, pdir, l)
            x = np.stack([rs.o.layer_ref(i, 0) for i in imgs])
            for l in range(1, len(rs.W)):
                x = rs.layer(l, x)
            if rs.cnv:
                assert ((x & 0xFFFF).astype(np.uint16).view(np.int16) == rs.o.scores_fast(imgs)).all(), (network, pdir)
            else:
                bits = lfc_last(rs, x)[:, :64] > 0
                words = (bits.astype(np.uint64) << np.arange(64, dtype=np.uint64)).sum(axis=1, dtype=np.uint64)
                assert (words == rs.o.words_fast(imgs)).all(), (network, pdir)
            rs.o.close()


@pytest.mark.parametrize("network,dataset", NETS, ids=lambda x: x)
def test_sweep_equals_restatement(network, dataset, shipped_and_random, tmp_path):
    """sampled sites of every non-last layer (corners, channel-word edges, every shift) and a whole-layer sweep of the
    last hidden layer, shipped and random parameters: changed, diffs and the total exactly as restated; layer-0 sites
    on fewer images (their restatement runs almost the whole network)"""
    L = gl.load(network)
    last_hidden = len(CNV_MAPS if network.startswith("cnv") else LFC_MAPS) - 1
    for p, pdir in enumerate(shipped_and_random[network]):
        L.load_parameters(pdir.encode())
        assert L.bnn_mi355x_last_error() == b"", L.bnn_mi355x_last_error()
        rs = Restatement(network, pdir)
        rng = np.random.default_rng(11 + p)
        recs = sample_sites(L, network, rng)
        for layers, n, recs_part in (([0], 16, recs[recs[:, 0] == 0]), (None, 40, recs[recs[:, 0] > 0]),
                                     ([last_hidden], 40, enumerate_act(L, last_hidden))):
            imgs = images(network, n, seed=40 + p)
            path = write_images(network, imgs, tmp_path, "i%d_%d" % (p, n))
            changed, diffs, total, got_n = sweep(L, path, recs_part)
            assert got_n == n
            want_changed, want_diffs = restate(rs, fault_free(rs, imgs), recs_part)
            assert changed.tolist() == want_changed.tolist(), (network, pdir, layers)
            assert diffs.tolist() == want_diffs.tolist(), (network, pdir, layers)
            assert total == want_changed.sum()
        rs.o.close()
    L.load_parameters(shipped_and_random[network][0].encode())


def test_cap_diffs_and_stage_counts(tmp_path):
    """a truncated list is the head of the full one and the full total is still returned; per-layer pair counts of a
    one-layer sweep: zero up to the site's layer, every pair at the next, then never growing"""
    network, dataset = "cnvW1A2", "cifar10"
    L = gl.load(network)
    L.load_parameters(gl.param_dir(dataset, network).encode())
    imgs = images(network, 48)
    path = write_images(network, imgs, tmp_path)
    recs = enumerate_act(L, 4)[::37]
    changed, diffs, total, n = sweep(L, path, recs)
    assert total == changed.sum() == len(diffs) and total > 4
    st = act_stages(L)
    assert len(st) == 9 and (st[:5] == 0).all() and st[5] == len(recs) * n
    assert all(st[l + 1] <= st[l] for l in range(5, 8)), st.tolist()
    for cap in (1, total // 2, total - 1):
        c2, d2, t2, _ = sweep(L, path, recs, cap=cap)
        assert t2 == total and c2.tolist() == changed.tolist() and d2.tolist() == diffs[:cap].tolist()
    c3, d3, t3, _ = sweep(L, path, recs, cap=0)
    assert t3 == total and len(d3) == 0


def test_several_groups_and_windows(tmp_path):
    """133 072 MNIST images x 3 sites: every record is a run group of its own, covering the images in two windows; the
    same as two calls on the two halves of the file, and the second half as restated"""
    network, dataset = "lfcW1A1", "mnist"
    L = gl.load(network)
    pdir = gl.param_dir(dataset, network)
    L.load_parameters(pdir.encode())
    imgs = images(network, 133072, seed=8)
    recs = np.array([[0, 0, 0, 17, 1], [1, 0, 0, 512, 1], [2, 0, 0, 1023, 1]], np.int32)
    changed, diffs, total, n = sweep(L, write_images(network, imgs, tmp_path, "all"), recs)
    assert n == 133072
    a = sweep(L, write_images(network, imgs[:131072], tmp_path, "a"), recs)
    b = sweep(L, write_images(network, imgs[131072:], tmp_path, "b"), recs)
    assert changed.tolist() == (a[0] + b[0]).tolist()
    merged = sorted(a[1].tolist() + [[f, i + 131072, c] for f, i, c in b[1].tolist()])
    assert diffs.tolist() == merged and total == a[2] + b[2]
    rs = Restatement(network, pdir)
    want_changed, want_diffs = restate(rs, fault_free(rs, imgs[131072:]), recs)
    assert b[0].tolist() == want_changed.tolist() and b[1].tolist() == want_diffs.tolist()
    assert (diffs[:, 1] >= 131072).any()


def test_loaded_parameters_untouched(tmp_path):
    """classes, the parameter CRC, last_faults and last_sweep_stages are the same before and after an activation sweep"""
    network, dataset = "cnvW2A2", "cifar10"
    L = gl.load(network)
    L.load_parameters(gl.param_dir(dataset, network).encode())
    imgs = images(network, 64)
    path = write_images(network, imgs, tmp_path)

    def classes():
        p = L.bnn_mi355x_inference_buffer(np.ascontiguousarray(imgs).ctypes.data, len(imgs), 10, None, 0)
        assert p, L.bnn_mi355x_last_error().decode()
        out = np.ctypeslib.as_array(p, shape=(len(imgs),)).astype(np.int32, copy=True)
        L.free_results(p)
        return out

    rec8 = np.array([[0, 0, 2, 0, 0, 0, 3, 1]], np.int32)
    ch = np.zeros(1, np.int32)
    assert L.bnn_mi355x_fault_sweep(path.encode(), 10, rec8.ctypes.data_as(ip), 1, ch.ctypes.data_as(ip), None, 0, None, None) >= 0
    before = (classes(), L.bnn_mi355x_params_crc(), L.bnn_mi355x_last_faults(None, 0), L.bnn_mi355x_last_sweep_stages(None, 0))
    sst = (C.c_long * 9)()
    L.bnn_mi355x_last_sweep_stages(sst, 9)
    sweep(L, path, np.concatenate([enumerate_act(L, 2)[::101], enumerate_act(L, 6)[::53]]))
    after = (classes(), L.bnn_mi355x_params_crc(), L.bnn_mi355x_last_faults(None, 0), L.bnn_mi355x_last_sweep_stages(None, 0))
    assert before[0].tolist() == after[0].tolist() and before[1:] == after[1:]
    sst2 = (C.c_long * 9)()
    L.bnn_mi355x_last_sweep_stages(sst2, 9)
    assert list(sst) == list(sst2)


def test_bad_records_refused_before_device_work(tmp_path):
    """a bad record anywhere in the list: -1 naming the record, and the previous sweep's stage counts are gone without
    any new ones (nothing ran)"""
    network, dataset = "lfcW1A2", "mnist"
    L = gl.load(network)
    L.load_parameters(gl.param_dir(dataset, network).encode())
    path = write_images(network, images(network, 16), tmp_path)
    good = enumerate_act(L, 1)[:4]
    sweep(L, path, good)
    assert L.bnn_mi355x_last_act_sweep_stages(None, 0) == 4
    for bad in ([3, 0, 0, 0, 1], [1, 0, 0, 1024, 1], [2, 0, 0, 5, 3], [0, 0, 1, 0, 1]):
        recs = np.concatenate([good, np.array([bad], np.int32)])
        ch = np.zeros(len(recs), np.int32)
        assert L.bnn_mi355x_act_fault_sweep(path.encode(), 10, recs.ctypes.data_as(ip), len(recs), ch.ctypes.data_as(ip), None, 0,
                                            None, None) == -1
        assert ("record 4 {%s}" % ", ".join(map(str, bad))).encode() in L.bnn_mi355x_last_error()
        assert L.bnn_mi355x_last_act_sweep_stages(None, 0) == 0


def test_variant_refused(variant_libs, tmp_path):
    L = gl.load("cnvW2A2-interleaved")
    L.load_parameters(gl.param_dir("cifar10", "cnvW2A2").encode())
    path = write_images("cnvW2A2", images("cnvW2A2", 4), tmp_path)
    rec = (C.c_int * 5)(3, 1, 1, 5, 2)
    ch = (C.c_int * 1)()
    assert L.bnn_mi355x_act_fault_sweep(path.encode(), 10, rec, 1, ch, None, 0, None, None) == -1
    assert b"not modelled" in L.bnn_mi355x_last_error()


def test_activation_sensitivity_and_map(tmp_path):
    """FaultTest.activation_sensitivity on lfcW1A2 layer 2 and cnvW1A1 layer 6: per-record accuracies rebuilt from the
    fault-free classes and the diffs, maps of the layer's shape; activation_sensitivity_map writes per-layer totals and
    per-channel / per-pixel vulnerability"""
    import json
    from bnn.faults import faults
    from bnn import bnn as B
    for network, dataset, layer, shape in (("lfcW1A2", "mnist", 2, (1, 1, 1024, 2)), ("cnvW1A1", "cifar10", 6, (1, 1, 512))):
        imgs = images(network, 60, seed=12)
        path = write_images(network, imgs, tmp_path, network)
        labels = np.random.default_rng(5).integers(0, 10, len(imgs)).tolist()
        cls_ = faults.CNVFaultTest if network.startswith("cnv") else faults.LFCFaultTest
        ft = cls_(network, dataset, path, labels)
        res = ft.activation_sensitivity([layer])[layer]
        clf = (B.CnvClassifier if network.startswith("cnv") else B.LfcClassifier)(network, dataset)
        kind = "cifars" if network.startswith("cnv") else "mnists"
        clean = np.asarray(getattr(clf, "classify_" + kind)(path))
        changed, diffs = getattr(clf, "classify_%s_act_fault_sweep" % kind)(path, res["records"])
        assert changed.tolist() == res["changed"].tolist()
        assert res["changed map"].shape == shape and res["changed map"].ravel().tolist() == changed.tolist()
        lab = np.array(labels)
        start = np.searchsorted(diffs[:, 0], np.arange(len(changed) + 1))
        for f in range(0, len(changed), 7):
            cls = clean.copy()
            d = diffs[start[f]:start[f + 1]]
            cls[d[:, 1]] = d[:, 2]
            assert res["accuracy"][f] == pytest.approx(100.0 * (cls == lab).sum() / len(lab), abs=1e-9)
        faults.NetworkTest(ft).activation_sensitivity_map(str(tmp_path / "out"), [layer])
        with open(tmp_path / "out" / network / dataset / "sensitivity" / ("%s_layer%d_activations.json" % (network, layer))) as f:
            doc = json.load(f)
        vul = res["changed map"].reshape(shape[:3] + (-1,)).mean(axis=3) / len(imgs)
        assert doc["totals"]["faults"] == len(changed) and doc["totals"]["max changed"] == int(changed.max())
        assert np.allclose(doc["per channel vulnerability"], vul.mean(axis=(0, 1)))
        assert np.allclose(doc["per pixel vulnerability"], vul.mean(axis=2))
