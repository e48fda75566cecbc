"""The windowed first stage of activation-fault sweeps on the GPU: for a CNV site of layers 0-2 the layer
after the site is evaluated only inside the window the changed activation reaches.  Nothing about a sweep's result may
change: the windowed route against the dense one (BNN_MI355X_ACT_WINDOW=0, the parent's code path) at every position of
the three maps, against the numpy restatement, over several run groups and image windows, and after persistent
parameter faults; and the trace says which route a group took."""
import contextlib
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import gpu_lib as gl
from test_gpu_act_fault_sweep import (CNV_MAPS, Restatement, act_stages, enumerate_act, fault_free, images, restate, sample_sites,  # noqa: F401
                                      sweep, write_images)

pytestmark = pytest.mark.gpu

TESTS = os.path.dirname(os.path.abspath(__file__))
NETS = ("cnvW1A1", "cnvW1A2", "cnvW2A2")
EDGE_CHANNELS = {0: (0, 31, 32, 63), 1: (0, 31, 32, 63), 2: (0, 31, 32, 63, 64, 127)}


@contextlib.contextmanager
def route(window, group=None):
    """the switches are read at every call: window=True forces the windowed first stage for every site layer 0-2 (whatever
    the per-case policy of an unset switch says), window=False the dense one; group caps a run group's pairs.
    Both switches are always set here and restored afterwards, so a value given from outside never reaches a sweep of
    these tests: every test runs both routes itself, and running the suite under BNN_MI355X_ACT_WINDOW=0 exercises
    nothing else."""
    keys = ("BNN_MI355X_ACT_WINDOW", "BNN_MI355X_SWEEP_GROUP")
    saved = {k: os.environ.pop(k, None) for k in keys}
    os.environ[keys[0]] = "1" if window else "0"
    if group is not None:
        os.environ[keys[1]] = str(group)
    try:
        yield
    finally:
        for k in keys:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]


def run(L, path, recs, window, group=None):
    """-> (changed, diffs, total, stages) as lists"""
    with route(window, group):
        changed, diffs, total, _ = sweep(L, path, recs, cap=len(recs) * 64)
        return changed.tolist(), diffs.tolist(), int(total), act_stages(L).tolist()


def every_position(network, layer):
    """all (y, x) of the layer's map x the channels at the word edges x every shift"""
    h, w, _ = CNV_MAPS[layer]
    shifts = range(1, 3 if network.endswith("A2") else 2)
    return np.array([[layer, y, x, c, s] for y in range(h) for x in range(w) for c in EDGE_CHANNELS[layer] for s in shifts], np.int32)


def load(L, pdir):
    L.load_parameters(pdir.encode())
    assert L.bnn_mi355x_last_error() == b"", L.bnn_mi355x_last_error()


@pytest.fixture(scope="module")
def param_sets(tmp_path_factory):
    import random_params
    sets = {}
    for k, network in enumerate(NETS):
        d = tmp_path_factory.mktemp("rp_" + network)
        random_params.make(str(d), network, 171 + k)
        sets[network] = [gl.param_dir("cifar10", network), str(d)]
    d = tmp_path_factory.mktemp("rp_neg2")
    random_params.make(str(d), "cnvW2A2", 181, neg2=0.05)
    sets["cnvW2A2"].append(str(d))
    return sets


@pytest.mark.parametrize("network", NETS)
def test_every_position_windowed_equals_dense(network, param_sets, tmp_path):
    """site layers 0, 1, 2: every pixel of the map (the borders, both pool parities), the channels at the word edges, every
    shift, 8 images; shipped and random parameters, cnvW2A2 also with weights of -2: changed, diffs, the total and the
    per-layer pair counts of the two routes agree exactly"""
    L = gl.load(network)
    path = write_images(network, images(network, 8, seed=61), tmp_path)
    for pdir in param_sets[network]:
        load(L, pdir)
        for layer in (0, 1, 2):
            recs = every_position(network, layer)
            win, dense = run(L, path, recs, True), run(L, path, recs, False)
            assert win[3] == dense[3], (pdir, layer, win[3], dense[3])
            assert win[2] == dense[2] and win[0] == dense[0], (pdir, layer)
            assert win[1] == dense[1], (pdir, layer)
            assert win[3][layer + 1] == len(recs) * 8 and sum(win[3][:layer + 1]) == 0
            # the window does change layer L+1's output: some pairs go on (a property of the inputs: the dense counts are
            # the same).  Classes must change for the shipped set; a random network may map all 8 images to classes that
            # no single activation moves.
            assert win[3][layer + 2] > 0, (pdir, layer, win[3])
            if pdir == param_sets[network][0]:
                assert sum(win[0]) > 0, (pdir, layer)
    load(L, param_sets[network][0])


def border_sites(network, layer):
    """y, x in {0, 1, 2, H-3, H-2, H-1}: every y with an x of the other and one of the same parity"""
    h, _, c = CNV_MAPS[layer]
    vals = [0, 1, 2, h - 3, h - 2, h - 1]
    levels = 3 if network.endswith("A2") else 2
    chans = EDGE_CHANNELS[layer]
    out = []
    for i, y in enumerate(vals):
        for j in (1, 2):
            k = len(out)
            out.append([layer, y, vals[(i + j) % 6], chans[k % len(chans)], 1 + k % (levels - 1)])
    return np.array(out, np.int32)


@pytest.mark.parametrize("network", NETS)
def test_windowed_sweep_equals_restatement(network, param_sets, tmp_path):
    """sample_sites' records of layers 0-2 and sites along the borders with mixed parities, shipped and random parameters:
    changed, diffs and the total exactly as the numpy restatement gives them (layer 0 on 16 images, layers 1-2 on 40)"""
    L = gl.load(network)
    for p, pdir in enumerate(param_sets[network][:2]):
        load(L, pdir)
        rs = Restatement(network, pdir)
        recs = sample_sites(L, network, np.random.default_rng(23 + p))
        recs = np.concatenate([recs[recs[:, 0] <= 2]] + [border_sites(network, l) for l in (0, 1, 2)])
        for n, part in ((16, recs[recs[:, 0] == 0]), (40, recs[recs[:, 0] > 0])):
            imgs = images(network, n, seed=50 + p)
            path = write_images(network, imgs, tmp_path, "i%d_%d" % (p, n))
            with route(True):
                changed, diffs, total, got_n = sweep(L, path, part)
            assert got_n == n
            want_changed, want_diffs = restate(rs, fault_free(rs, imgs), part)
            assert changed.tolist() == want_changed.tolist(), (network, pdir, n)
            assert diffs.tolist() == want_diffs.tolist(), (network, pdir, n)
            assert total == want_changed.sum()
        rs.o.close()
    load(L, param_sets[network][0])


def test_not_vacuous(param_sets, tmp_path):
    """the records of the every-position test do change what the next layers see: for shipped cnvW1A1 layer-0 sites at
    least half of the pairs still differ from the fault-free output after the windowed layer (80 % do even
    at layer 8) -- on the dense route too, so it is a property of the inputs --, and for every net and site layer some
    image changes its class"""
    for network in NETS:
        L = gl.load(network)
        load(L, param_sets[network][0])
        path = write_images(network, images(network, 8, seed=61), tmp_path, network)
        for layer in (0, 1, 2):
            recs = every_position(network, layer)
            win = run(L, path, recs, True)
            assert sum(win[0]) > 0, (network, layer)
            if network == "cnvW1A1" and layer == 0:
                dense = run(L, path, recs, False)
                for st in (win[3], dense[3]):
                    print("cnvW1A1 layer 0: pairs at layer 1 %d, at layer 2 %d" % (st[1], st[2]))
                    assert st[1] == len(recs) * 8 and st[2] >= 0.5 * st[1], st


@pytest.mark.parametrize("network", ("cnvW1A1", "cnvW2A2"))
def test_groups_and_image_windows(network, param_sets, tmp_path):
    """40 images x 30 layer-0 records under BNN_MI355X_SWEEP_GROUP: 320 pairs a group (8 records x all images: four run
    groups) and 25 pairs (one record a group, the images in two windows of 25 and 15): the same result as the
    unconstrained call, and as the dense route under the same cap"""
    L = gl.load(network)
    load(L, param_sets[network][0])
    n = 40
    path = write_images(network, images(network, n, seed=62), tmp_path)
    recs = enumerate_act(L, 0)
    recs = recs[np.random.default_rng(3).choice(len(recs), 30, replace=False)]
    free = run(L, path, recs, True)
    assert free[2] == sum(free[0]) and free[3][1] == 30 * n
    for cap in (8 * n, 25):
        win, dense = run(L, path, recs, True, group=cap), run(L, path, recs, False, group=cap)
        assert win == free, cap
        assert dense == free, cap


CHILD = (
    "import sys, numpy as np; sys.path[:0] = [%r, %r]\n"
    "import gpu_lib as gl\n"
    "from test_gpu_act_fault_sweep import images, write_images, sweep\n"
    "import pathlib\n"
    "L = gl.load('cnvW1A1'); L.load_parameters(gl.param_dir('cifar10', 'cnvW1A1').encode())\n"
    "path = write_images('cnvW1A1', images('cnvW1A1', 12), pathlib.Path(%r))\n"
    "sweep(L, path, np.array([[0, 3, 4, 5, 1], [0, 29, 0, 63, 1], [0, 14, 15, 32, 1]], np.int32))\n"
    "sweep(L, path, np.array([[4, 1, 1, 7, 1], [4, 2, 0, 255, 1]], np.int32))\n"
    "print('child-ok')\n")


def traced_groups(tmp_path, **env):
    """one layer-0 sweep (3 sites) and one layer-4 sweep (2 sites) on 12 images in a fresh process under BNN_MI355X_TRACE:
    -> [(layer, windowed pairs, pixels per pair)] of the new trace line, in order"""
    e = dict(os.environ)
    for k in ("BNN_MI355X_ACT_WINDOW", "BNN_MI355X_SWEEP_GROUP"):
        e.pop(k, None)
    e.update(BNN_MI355X_TRACE="1", **env)
    out = subprocess.run([sys.executable, "-c", CHILD % (TESTS, os.path.join(gl.ROOT, "bnn-pynq_amd"), str(tmp_path))], env=e,
                         capture_output=True, text=True, timeout=600)
    assert "child-ok" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]
    assert len(re.findall(r"trace act_fault_sweep: layer \d+ sites", out.stderr)) == 2   # (the existing line stays)
    return [tuple(int(v) for v in m) for m in
            re.findall(r"trace act_fault_sweep window: layer (\d+), (\d+) pairs windowed, (\d+) pixels per pair", out.stderr)]


def test_the_window_route_is_the_one_taken(tmp_path):
    """the layer-0 group reports all its pairs windowed with 16 pixels per pair, the layer-4 group none; with the switch
    off both report none.  Switch unset: the per-case policy decides, so the layer-0 group takes one of the two routes."""
    on, off = [(0, 3 * 12, 16), (4, 0, 0)], [(0, 0, 0), (4, 0, 0)]
    assert traced_groups(tmp_path, BNN_MI355X_ACT_WINDOW="1") == on
    assert traced_groups(tmp_path, BNN_MI355X_ACT_WINDOW="0") == off
    assert traced_groups(tmp_path) in (on, off)


def test_after_persistent_faults(param_sets, tmp_path):
    """cnvW2A2 after inference_multiple_with_faults has left faults in the loaded rows (single-bit flips: weights of -2
    among them): a layer-1 sweep is the same on both routes, and the parameter CRC, last_faults and the classes of a
    plain call are what they were before the sweeps"""
    network = "cnvW2A2"
    L = gl.load(network)
    load(L, param_sets[network][0])
    imgs = images(network, 48, seed=63)
    path = write_images(network, imgs, tmp_path)

    def classes():
        p = L.bnn_mi355x_inference_buffer(np.ascontiguousarray(imgs).ctypes.data, len(imgs), 10, None, 0)
        assert p, L.bnn_mi355x_last_error().decode()
        out = np.ctypeslib.as_array(p, shape=(len(imgs),)).astype(np.int32, copy=True)
        L.free_results(p)
        return out.tolist()

    try:
        crc0 = L.bnn_mi355x_params_crc()
        assert L.bnn_mi355x_set_fault_seed(77) == 0
        cnt = C.c_int(0)
        for _ in range(4):
            p = L.inference_multiple_with_faults(path.encode(), 10, C.byref(cnt), None, 200, 1, 0, (C.c_int * 3)(1, 2, 3), 3)
            assert p and cnt.value == len(imgs), L.bnn_mi355x_last_error()
            L.free_results(p)
            if L.bnn_mi355x_params_crc() != crc0:
                break
        assert L.bnn_mi355x_params_crc() != crc0
        before = (classes(), L.bnn_mi355x_params_crc(), L.bnn_mi355x_last_faults(None, 0))
        recs = enumerate_act(L, 1)[::29]
        win, dense = run(L, path, recs, True), run(L, path, recs, False)
        assert win == dense and sum(win[0]) > 0
        assert (classes(), L.bnn_mi355x_params_crc(), L.bnn_mi355x_last_faults(None, 0)) == before
    finally:
        load(L, param_sets[network][0])
