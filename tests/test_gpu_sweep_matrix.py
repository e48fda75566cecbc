"""Single-fault sweeps on the matrix cores (bnn_mi355x_campaign_form(1): every stage of layers 1-7 that reads the loaded
parameters runs as FP4 GEMMs on tiles packed from the list of the stage's alive slots, csrc/list_mfma_kernels.hip).  All
checks are exact: form 1 against form 0, and both against the references the sweeps' own tests use.  24 images: a multiple
of no tile's 32 or 128 images, a ragged last tile everywhere; pruning leaves the survivors scattered."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import gpu_lib as gl
import test_gpu_act_fault_sweep as sw
import test_gpu_fault_sweep as tp
import test_gpu_input_faults as ti
import test_gpu_sweep_profile as pf

pytestmark = pytest.mark.gpu
CNV = ("cnvW1A1", "cnvW1A2", "cnvW2A2")
N = 24
SITE_LAYERS = (0, 1, 2, 3, 5, 6)  # the stage behind each: one per list kernel family and pooling case


def both_forms(L, call):
    """call() under form 0, then under form 1; the form found is put back"""
    was = L.bnn_mi355x_campaign_form(0)
    try:
        a = call()
        L.bnn_mi355x_campaign_form(1)
        return a, call()
    finally:
        L.bnn_mi355x_campaign_form(was)


def sites(L, layer, k=40):
    """about k of the layer's sites, evenly over the enumeration (rows, columns, channels, shifts), the four corners among them"""
    rec = sw.enumerate_act(L, layer)
    corners = [int(np.nonzero((rec[:, 1] == y) & (rec[:, 2] == x))[0][0]) for y in (0, rec[:, 1].max()) for x in (0, rec[:, 2].max())]
    return rec[sorted(set(np.linspace(0, len(rec) - 1, k - 4).astype(int).tolist() + corners))]


def act_call(L, path, recs):
    changed, diffs, total, n = sw.sweep(L, path, recs)
    return changed.tolist(), diffs.tolist(), total, n, sw.act_stages(L).tolist()


@pytest.fixture(scope="module", params=CNV)
def case(request, tmp_path_factory):
    """-> (network, library with the shipped parameters, images, their file, restatement, its fault-free outputs): once per network"""
    network = request.param
    pdir = gl.param_dir("cifar10", network)
    L = gl.load(network)
    L.load_parameters(pdir.encode())
    assert L.bnn_mi355x_last_error() == b""
    imgs = sw.images(network, N, seed=23)
    path = sw.write_images(network, imgs, tmp_path_factory.mktemp("sweep_matrix"))
    rs = sw.Restatement(network, pdir)
    yield network, L, pdir, imgs, path, rs, sw.fault_free(rs, imgs)
    rs.o.close()


@pytest.mark.parametrize("layer", SITE_LAYERS)
def test_activation_sweep(case, layer):
    network, L, _, _, path, rs, base = case
    recs = sites(L, layer)
    a, b = both_forms(L, lambda: act_call(L, path, recs))
    want_changed, want_diffs = sw.restate(rs, base, recs)
    print(network, "site layer", layer, len(recs), "sites, pairs per stage:", a[4], "changed:", int(want_changed.sum()))
    assert b == a
    assert a[0] == want_changed.tolist() and a[1] == want_diffs.tolist() and a[2] == want_changed.sum() and a[3] == N
    assert a[4][layer + 1] == len(recs) * N  # (the first stage runs every pair)


def test_one_pair(case, tmp_path):
    """one image, one site of layer 0: every list is one entry long"""
    network, L, _, imgs, _, rs, base = case
    path = sw.write_images(network, imgs[:1], tmp_path)
    recs = sites(L, 0)[17:18]
    a, b = both_forms(L, lambda: act_call(L, path, recs))
    want_changed, want_diffs = sw.restate(rs, [x[:1] for x in base], recs)
    assert b == a and a[0] == want_changed.tolist() and a[1] == want_diffs.tolist() and a[4][1] == 1


def test_parameter_sweep(case, tmp_path):
    """36 faults of layers 1 and 4, weights and thresholds, word sizes 1, 2 and 8: the layers behind the faulted one from the list"""
    network, L, pdir, _, _, _, _ = case
    imgs, path = tp.images(network, N, tmp_path, golden=False)
    recs = tp.sample(L, network, 3, layers=[1, 4])
    assert 30 <= len(recs) <= 40
    a, b = both_forms(L, lambda: [x.tolist() for x in tp.sweep(L, path, recs)[:2]] + [tp.stages(L).tolist()])
    assert b == a
    want_changed, want_diffs, clean = tp.dense(L, pdir, imgs, recs)
    assert a[0] == want_changed.tolist() and a[1] == want_diffs.tolist() and sum(a[0]) > 0
    diffs = np.array(a[1], np.int32).reshape(-1, 3)
    for f in np.nonzero(want_changed)[0][:3]:
        assert diffs[diffs[:, 0] == f][:, 1:].tolist() == tp.oracle_changed(network, pdir, imgs, recs[f], clean), recs[f]


def test_input_sweep(case):
    network, L, _, _, path, _, _ = case
    recs = ti.records_of(network)[:16]
    a, b = both_forms(L, lambda: [x.tolist() for x in ti.sweep(L, path, recs)[:2]] + [ti.stages(L).tolist()])
    assert b == a and a[2][0] == 16 * N


def test_propagation_profile(case):
    network, L, _, _, path, _, _ = case
    recs = sites(L, 0)

    def call():
        res, alive, flipped = pf.profiled(L, lambda *args: act_call(*args)[:2], path, recs)
        return res, alive.tolist(), flipped.tolist()

    a, b = both_forms(L, call)
    assert b == a and np.array(a[2]).sum() > 0


CHILD = (
    "import sys; sys.path[:0] = [%r, %r]\n"
    "import torch, gpu_lib as gl, test_gpu_act_fault_sweep as sw, test_gpu_sweep_matrix as m\n"
    "L = gl.load(%r); L.load_parameters(gl.param_dir('cifar10', %r).encode())\n"
    "a, b = m.both_forms(L, lambda: m.act_call(L, %r, m.sites(L, 0)))\n"
    "assert a == b and a[3] == m.N\n"
    "print('child-ok')\n")


def test_window_route(case):
    """BNN_MI355X_ACT_WINDOW=1 in a fresh process: layer 1 stays the window kernels', the list takes over at layer 2"""
    network, _, _, _, path, _, _ = case
    env = dict(os.environ, BNN_MI355X_ACT_WINDOW="1", BNN_MI355X_TRACE="1")
    env.pop("BNN_MI355X_SWEEP_GROUP", None)
    here = os.path.dirname(os.path.abspath(__file__))
    out = subprocess.run([sys.executable, "-c", CHILD % (here, os.path.join(gl.ROOT, "bnn-pynq_amd"), network, network, path)], env=env,
                         capture_output=True, text=True, timeout=600)
    assert "child-ok" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]
    assert "layer 0, %d pairs windowed" % (len(sites(case[1], 0)) * N) in out.stderr
    listed = [int(l) for l in re.findall(r"trace sweep list: layer (\d+),", out.stderr)]
    assert listed and min(listed) == 2
