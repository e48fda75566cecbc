"""Propagation profiles of the single-fault sweeps on the GPU (bnn_mi355x_sweep_profile / bnn_mi355x_last_sweep_profile):
per record and layer the images whose output differs from the fault-free one and the activations that differ in them.
Every profile must equal, exactly, what a reference that is not the code under test gives: the oracle's layer_ref with the
fault applied (parameter faults), layer_ref of the host-flipped image (input bits), the numpy restatement of
test_gpu_act_fault_sweep from the changed site on (activation sites).  37 images: the last block of a record has one
live wave of four."""
import ctypes as C
import json
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import gpu_lib as gl
import oracle_lib as ol
import test_gpu_act_fault_sweep as ta
import test_gpu_fault_sweep as tp
import test_gpu_input_faults as ti

pytestmark = pytest.mark.gpu
lp = C.POINTER(C.c_long)
N = 37
DATASET = {"cnvW1A1": "cifar10", "cnvW2A2": "cifar10", "lfcW1A1": "mnist", "lfcW1A2": "mnist"}
POOL = ThreadPoolExecutor(min(16, os.cpu_count() or 1))  # (layer_ref: plain C on its own buffers, the GIL released)
_IMAGES, _BASE = {}, {}


def maps(network):
    return ta.CNV_MAPS if network.startswith("cnv") else ta.LFC_MAPS


def elements(network):
    return np.array([h * w * c for h, w, c in maps(network)], np.int64)


def the_images(network):
    """random images plus the golden ones, 37 in all, the same for every test of a network"""
    if network not in _IMAGES:
        gold = tp.golden_images(network)
        isz = 3072 if network.startswith("cnv") else 784
        _IMAGES[network] = np.concatenate([np.random.default_rng(29).integers(0, 256, (N - len(gold), isz), dtype=np.uint8), gold])
    return _IMAGES[network]


def image_file(network, tmp_path):
    imgs = the_images(network)
    assert len(imgs) == N
    return imgs, tp.write_images(network, imgs, tmp_path)


def layer_outputs(o, imgs, first=0):
    """the oracle's layer_ref of every image for the layers first ... S - 2 -> {layer: int8 [n, elements]}"""
    jobs = [(l, i) for l in range(first, o.nl - 1) for i in range(len(imgs))]
    got = list(POOL.map(lambda j: o.layer_ref(imgs[j[1]], j[0]), jobs))
    return {l: np.stack([g for (jl, _), g in zip(jobs, got) if jl == l]) for l in range(first, o.nl - 1)}


def fault_free(network):
    """every layer's fault-free output of the 37 images from the oracle, computed once per network"""
    if network not in _BASE:
        o = ol.Oracle(network, gl.param_dir(DATASET[network], network))
        _BASE[network] = layer_outputs(o, the_images(network))
        o.close()
    return _BASE[network]


def counted(outs, base, cols):
    """-> (alive [cols], flipped [cols]) of one record from its layers' outputs against the fault-free ones"""
    alive, flipped = np.zeros(cols, np.int64), np.zeros(cols, np.int64)
    for l, x in outs.items():
        d = x != base[l]
        alive[l], flipped[l] = d.any(axis=1).sum(), d.sum()
    return alive, flipped


def read_profile(L):
    cols = C.c_int(0)
    rows = L.bnn_mi355x_last_sweep_profile(0, None, None, 0, C.byref(cols))
    assert rows >= 0
    a, f = np.full((rows, cols.value), -1, np.int64), np.full((rows, cols.value), -1, np.int64)
    assert L.bnn_mi355x_last_sweep_profile(0, a.ctypes.data_as(lp), f.ctypes.data_as(lp), rows, None) == rows
    return a, f


def profiled(L, sweep, path, recs):
    """the sweep with profiling on -> (what the sweep returns, alive, flipped); the setting found is put back"""
    before = L.bnn_mi355x_sweep_profile(1)
    try:
        res = sweep(L, path, recs)
        alive, flipped = read_profile(L)
    finally:
        L.bnn_mi355x_sweep_profile(before)
    assert alive.shape == flipped.shape == (len(recs), len(maps(L.bnn_mi355x_network().decode())))
    return res, alive, flipped


def check_invariants(network, alive, flipped, changed, s0, n=N):
    el, cols = elements(network), alive.shape[1]
    assert (alive >= 0).all() and (alive <= n).all()
    assert (alive <= flipped).all() and (flipped <= alive * el[None]).all()
    for f in range(len(alive)):
        assert not alive[f, :s0[f]].any() and not flipped[f, :s0[f]].any(), f
        for l in range(s0[f], cols - 1):
            assert alive[f, l] > 0 or alive[f, l + 1] == 0, (f, l)
        if s0[f] <= cols - 1:
            assert changed[f] <= alive[f, cols - 1], f


def loaded(network):
    L = gl.load(network)
    L.load_parameters(gl.param_dir(DATASET[network], network).encode())
    assert L.bnn_mi355x_last_error() == b""
    return L


# -- parameter faults

def parameter_records(L, network):
    """a record of every layer (the last one among them) and of both targets -- LFC: both in every layer that has
    thresholds; CNV: the layers take turns, cnvW1A1 starting with a weight and cnvW2A2 with a threshold, since the
    reference of a CNV record runs the network once per image and layer --, and three flips of a threshold's lowest bit
    in the last hidden layer, of which the reference must find one to change nothing"""
    rng = np.random.default_rng(17)
    S = len(maps(network)) + 1
    out = []
    for layer in range(S):
        for target in (((layer + (network == "cnvW2A2")) % 2,) if S == 9 and layer < S - 1 else (0, 1)):
            rec = tp.enumerate_faults(L, layer, target, 1)
            if len(rec):
                out.append(rec[rng.integers(len(rec))])
    thr = tp.enumerate_faults(L, S - 2, 1, 1)
    low = thr[thr[:, 6] == 0]
    out.extend(low[[len(low) // 5, 2 * len(low) // 5, 3 * len(low) // 5]])
    recs = np.array(out, np.int32)
    assert (recs[:, 2] == S - 1).any() and len(recs) <= 30
    return recs


def parameter_reference(network, imgs, recs):
    base, cols = fault_free(network), len(maps(network))
    alive, flipped = np.zeros((len(recs), cols), np.int64), np.zeros((len(recs), cols), np.int64)
    for f, rec in enumerate(recs):
        o = ol.Oracle(network, gl.param_dir(DATASET[network], network))
        assert o.apply_fault(rec) >= 0
        alive[f], flipped[f] = counted(layer_outputs(o, imgs, first=int(rec[2])), base, cols)
        o.close()
    return alive, flipped


@pytest.mark.parametrize("network", ["cnvW1A1", "cnvW2A2", "lfcW1A1", "lfcW1A2"])
def test_parameter_faults_against_the_oracle(network, tmp_path):
    L = loaded(network)
    imgs, path = image_file(network, tmp_path)
    recs = parameter_records(L, network)
    (changed, _, total, n, _), alive, flipped = profiled(L, tp.sweep, path, recs)
    assert n == N
    want_alive, want_flipped = parameter_reference(network, imgs, recs)
    print(network, "alive", alive.sum(axis=0).tolist(), "flipped", flipped.sum(axis=0).tolist())
    assert alive.tolist() == want_alive.tolist()
    assert flipped.tolist() == want_flipped.tolist()
    last = recs[:, 2] == len(maps(network))
    assert last.any() and not alive[last].any() and not flipped[last].any()  # (the last layer has no output map)
    assert (want_alive[-3:].sum(axis=1) == 0).any(), "no threshold fault without effect among the three"
    assert alive.any()
    check_invariants(network, alive, flipped, changed, recs[:, 2])
    # paging: rows [first, first + cap_rows), either array may be missing
    a = np.full((2, alive.shape[1]), -1, np.int64)
    assert L.bnn_mi355x_last_sweep_profile(1, a.ctypes.data_as(lp), None, 2, None) == len(recs)
    assert a.tolist() == alive[1:3].tolist()
    assert L.bnn_mi355x_last_sweep_profile(len(recs) - 1, None, a.ctypes.data_as(lp), 2, None) == len(recs)
    assert a[0].tolist() == flipped[-1].tolist() and a[1].tolist() == alive[2].tolist()  # (one row was left to write)


# -- activation sites

def activation_records(network, layers):
    """per layer the map's corners and centre with the channels 0, 31, 32, 63 and the last one, every shift of each"""
    levels = 3 if network.endswith("A2") else 2
    out = []
    for k, layer in enumerate(layers):
        h, w, c = maps(network)[layer]
        pos = [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (h // 2, w // 2)]
        chans = [0, 31, 32, 63, c - 1]
        for i in range(5 if levels == 2 else 3):
            y, x = pos[(k + i) % 5]
            out.extend([layer, y, x, chans[(k + 2 * i) % 5], s] for s in range(1, levels))
    assert len(out) <= 30
    return np.array(out, np.int32)


def activation_reference(network, imgs, recs):
    """the restatement from the changed site on, each layer's output kept"""
    rs = ta.Restatement(network, gl.param_dir(DATASET[network], network))
    base = ta.fault_free(rs, imgs)
    cols, levels = len(base), 2 if rs.a1 else 3
    alive, flipped = np.zeros((len(recs), cols), np.int64), np.zeros((len(recs), cols), np.int64)
    for f, (layer, y, xx, ch, shift) in enumerate(recs.tolist()):
        h, w, c = rs.maps[layer]
        e = (y * w + xx) * c + ch
        x = base[layer].copy()
        i = (x[:, e].astype(np.int64) + 1) // (2 if levels == 2 else 1)
        i = (i + shift) % levels
        x[:, e] = (2 * i - 1) if levels == 2 else (i - 1)
        for l in range(layer + 1, cols):
            x = rs.layer(l, x)
            d = x != base[l]
            alive[f, l], flipped[f, l] = d.any(axis=1).sum(), d.sum()
    rs.o.close()
    return alive, flipped


@pytest.mark.parametrize("network,layers", [("cnvW1A1", [0, 1, 2, 3, 7]), ("cnvW2A2", [0, 1, 2, 3, 7]), ("lfcW1A2", [1])])
def test_activation_sites_against_the_restatement(network, layers, tmp_path, monkeypatch):
    L = loaded(network)
    imgs, path = image_file(network, tmp_path)
    recs = activation_records(network, layers)
    want_alive, want_flipped = activation_reference(network, imgs, recs)
    for route in ("0", "1"):  # (the dense first stage, and the site's window alone where there is a window kernel)
        monkeypatch.setenv("BNN_MI355X_ACT_WINDOW", route)
        (changed, _, total, n), alive, flipped = profiled(L, ta.sweep, path, recs)
        print(network, "route", route, "alive", alive.sum(axis=0).tolist(), "flipped", flipped.sum(axis=0).tolist())
        assert n == N
        assert alive.tolist() == want_alive.tolist(), route
        assert flipped.tolist() == want_flipped.tolist(), route
        check_invariants(network, alive, flipped, changed, recs[:, 0] + 1)
    assert alive.any()
    hidden = recs[:, 0] == len(maps(network)) - 1
    if hidden.any():  # (a site of the last hidden layer: nothing is evaluated that has an output map)
        assert not alive[hidden].any() and not flipped[hidden].any()


# -- input sites

def input_records(network):
    """bits 0 and 7 of the bytes at the 16-byte lanes' and the planes' edges"""
    if network.startswith("cnv"):  # (six records: the reference of each runs the whole network once per image and layer)
        return np.array([(15, 0), (16, 7), (1023, 0), (1024, 7), (2047, 7), (3071, 0)], np.int32)
    return np.array([(b, bit) for b in (0, 15, 16, 767, 768, 783) for bit in (0, 7)], np.int32)


def input_reference(network, imgs, recs):
    base, cols = fault_free(network), len(maps(network))
    o = ol.Oracle(network, gl.param_dir(DATASET[network], network))
    alive, flipped = np.zeros((len(recs), cols), np.int64), np.zeros((len(recs), cols), np.int64)
    for f, (b, bit) in enumerate(recs.tolist()):
        host = imgs.copy()
        host[:, b] ^= np.uint8(1 << bit)
        alive[f], flipped[f] = counted(layer_outputs(o, host), base, cols)
    o.close()
    return alive, flipped


@pytest.mark.parametrize("network", ["cnvW1A1", "lfcW1A1"])
def test_input_sites_against_the_oracle(network, tmp_path):
    L = loaded(network)
    imgs, path = image_file(network, tmp_path)
    recs = input_records(network)
    (changed, _, total, n), alive, flipped = profiled(L, ti.sweep, path, recs)
    want_alive, want_flipped = input_reference(network, imgs, recs)
    print(network, "alive", alive.sum(axis=0).tolist(), "flipped", flipped.sum(axis=0).tolist())
    assert n == N
    assert alive.tolist() == want_alive.tolist()
    assert flipped.tolist() == want_flipped.tolist()
    assert alive.any()
    if network.startswith("lfc"):  # (the binariser reads bit 7 alone)
        assert not alive[recs[:, 1] < 7].any() and not flipped[recs[:, 1] < 7].any()
    check_invariants(network, alive, flipped, changed, np.zeros(len(recs), np.int64))


# -- groups and image windows

@pytest.mark.parametrize("network,kind", [("cnvW1A1", "activation"), ("lfcW1A2", "activation"), ("cnvW1A1", "input"), ("lfcW1A1", "input")])
def test_groups_and_image_windows(network, kind, tmp_path, monkeypatch):
    """the same records in one group, in groups of three faults, and one fault per group in two image windows of 20 and
    17: the counts of a fault's windows are added up"""
    L = loaded(network)
    _, path = image_file(network, tmp_path)
    if kind == "activation":
        recs, sweep = activation_records(network, [0, 1, 2, 3, 7] if network.startswith("cnv") else [0, 1]), ta.sweep
        s0 = recs[:, 0] + 1
    else:
        recs, sweep = input_records(network), ti.sweep
        s0 = np.zeros(len(recs), np.int64)
    monkeypatch.delenv("BNN_MI355X_SWEEP_GROUP", raising=False)
    monkeypatch.delenv("BNN_MI355X_ACT_WINDOW", raising=False)
    res, alive, flipped = profiled(L, sweep, path, recs)
    assert alive.any()
    for group in (3 * N + 1, 20):
        monkeypatch.setenv("BNN_MI355X_SWEEP_GROUP", str(group))
        res2, alive2, flipped2 = profiled(L, sweep, path, recs)
        assert res2[0].tolist() == res[0].tolist() and res2[1].tolist() == res[1].tolist(), group
        assert alive2.tolist() == alive.tolist(), group
        assert flipped2.tolist() == flipped.tolist(), group
        check_invariants(network, alive2, flipped2, res2[0], s0)


# -- against the pair counts of the pruning loop

@pytest.mark.parametrize("kind", ["parameter", "activation", "input"])
def test_alive_sums_equal_the_stage_pairs(kind, tmp_path):
    """records of one layer: the pairs a layer has to run are the pairs alive after the layer before it"""
    network = "cnvW1A1"
    L = loaded(network)
    _, path = image_file(network, tmp_path)
    rng = np.random.default_rng(23)
    if kind == "parameter":
        rec = tp.enumerate_faults(L, 2, 0, 1)
        recs, sweep, stages, s0 = rec[rng.choice(len(rec), 30, replace=False)], tp.sweep, tp.stages, 2
    elif kind == "activation":
        rec = ta.enumerate_act(L, 1)
        recs, sweep, stages, s0 = rec[rng.choice(len(rec), 30, replace=False)], ta.sweep, ta.act_stages, 2
    else:
        rec = np.stack([rng.integers(0, 3072, 30), rng.integers(5, 8, 30)], axis=1).astype(np.int32)
        recs, sweep, stages, s0 = rec, ti.sweep, ti.stages, 0
    res, alive, flipped = profiled(L, sweep, path, recs)
    pairs = stages(L)
    S = len(pairs)
    assert S == alive.shape[1] + 1 and pairs[s0] == len(recs) * N and not pairs[:s0].any()
    for l in range(s0, S - 1):
        assert alive[:, l].sum() == pairs[l + 1], l
    assert alive[:, s0].sum() > 0
    check_invariants(network, alive, flipped, res[0], np.full(len(recs), s0))


# -- off means off

@pytest.mark.parametrize("network,kind", [("cnvW2A2", "parameter"), ("lfcW1A2", "activation"), ("lfcW1A1", "input")])
def test_off_means_off(network, kind, tmp_path):
    """with profiling off the results are those of the profiled call and the earlier profile stays"""
    L = loaded(network)
    _, path = image_file(network, tmp_path)
    if kind == "parameter":
        recs, sweep, stages = parameter_records(L, network), tp.sweep, tp.stages
    elif kind == "activation":
        recs, sweep, stages = activation_records(network, [0, 1]), ta.sweep, ta.act_stages
    else:
        recs, sweep, stages = input_records(network), ti.sweep, ti.stages
    res, alive, flipped = profiled(L, sweep, path, recs)
    pairs = stages(L)
    assert L.bnn_mi355x_sweep_profile(0) == 0
    off = sweep(L, path, recs[::-1][:7])  # (other records: a profile of this call would look different)
    assert read_profile(L)[0].tolist() == alive.tolist() and read_profile(L)[1].tolist() == flipped.tolist()
    off = sweep(L, path, recs)
    assert off[0].tolist() == res[0].tolist() and off[1].tolist() == res[1].tolist() and off[2:4] == res[2:4]
    assert stages(L).tolist() == pairs.tolist()
    assert read_profile(L)[0].tolist() == alive.tolist() and read_profile(L)[1].tolist() == flipped.tolist()
    # a profiled sweep without records: an empty profile, and a failing one: none
    assert L.bnn_mi355x_sweep_profile(1) == 0
    try:
        sweep(L, path, recs[:0])
        assert read_profile(L)[0].shape == (0, len(maps(network)))
        sweep(L, path, recs[:2])
        assert read_profile(L)[0].tolist() == alive[:2].tolist()
        ch = (C.c_int * 2)()
        args = (b"/nonexistent", 10, np.ascontiguousarray(recs[:2]).ctypes.data_as(C.POINTER(C.c_int)), 2, ch, None, 0, None, None)
        fn = {"parameter": L.bnn_mi355x_fault_sweep, "activation": L.bnn_mi355x_act_fault_sweep, "input": L.bnn_mi355x_input_fault_sweep}[kind]
        assert fn(*args) == -1
        assert read_profile(L)[0].shape[0] == 0
    finally:
        L.bnn_mi355x_sweep_profile(0)


# -- Python

def test_python_propagation(tmp_path):
    from bnn.faults import faults
    network, dataset = "lfcW1A1", "mnist"
    L = loaded(network)
    imgs, path = image_file(network, tmp_path)
    labels = tp.classes(L, imgs).tolist()
    ft = faults.LFCFaultTest(network, dataset, path, labels)
    recs = parameter_records(L, network)
    (changed, _, _, _, _), alive, flipped = profiled(L, tp.sweep, path, recs)
    r = ft.propagation("parameter", records=recs)
    assert r["alive"].shape == r["flipped"].shape == (len(recs), 3) and r["alive"].dtype == np.int64 and r["images"] == N
    assert r["changed"].tolist() == changed.tolist() and r["alive"].tolist() == alive.tolist() and r["flipped"].tolist() == flipped.tolist()
    r = ft.propagation("activation", layers=[2])
    assert r["records"].shape == (1024, 5) and r["alive"].shape == (1024, 3) and not r["alive"].any()
    r = ft.propagation("input", records=[[0, 7], [783, 7], [5, 0]])
    assert r["alive"].shape == (3, 3) and r["changed"].shape == (3,) and not r["alive"][2].any()
    assert L.bnn_mi355x_sweep_profile(0) == 0  # (put back after each)
    # the setting found is put back after an exception, on or off
    for on in (1, 0):
        L.bnn_mi355x_sweep_profile(on)
        with pytest.raises(RuntimeError):
            ft.propagation("activation", records=[[9, 0, 0, 0, 1]])
        assert L.bnn_mi355x_sweep_profile(0) == on
    with pytest.raises(ValueError):
        ft.propagation("weights")
    # the map's files: one per site layer, a curve entry per downstream layer
    out = faults.NetworkTest(ft).propagation_map(str(tmp_path / "out"), "activation", [0, 1])
    folder = tmp_path / "out" / network / dataset / "sensitivity"
    for layer in (0, 1):
        with open(folder / ("%s_layer%d_activation_propagation.json" % (network, layer))) as f:
            doc = json.load(f)
        assert doc == json.loads(json.dumps(out[layer]))
        assert doc["downstream layers"] == list(range(layer + 1, 3)) and doc["totals"]["faults"] == 1024 and doc["images"] == N
        assert len(doc["share alive"]) == len(doc["mean error size"]) == 2 - layer
        assert 0.0 < doc["share alive"][0] <= 1.0 and doc["mean error size"][0] >= 1.0
    r = ft.propagation("activation", layers=[1])
    share, size = faults.propagation_curves(r["alive"], r["flipped"], N, 2)
    assert doc["share alive"] == share == [r["alive"][:, 2].sum() / (1024.0 * N)] and doc["mean error size"] == size
    out = faults.NetworkTest(ft).propagation_map(str(tmp_path / "out"), "input")
    with open(folder / (network + "_input_propagation.json")) as f:
        doc = json.load(f)
    assert doc["totals"]["faults"] == 784 * 8 and doc["downstream layers"] == [0, 1, 2] and len(doc["share alive"]) == 3
    assert 0.0 < doc["share alive"][0] <= 1.0 / 8
    assert L.bnn_mi355x_sweep_profile(0) == 0
