"""The matrix-core form of the LFC nets (k_lfc_mfma, csrc/lfc_mfma_kernels.hip; BNN_MI355X_LFC=mfma): raw words and
classes against the CPU restatement (oracle/) at the sizes its tiling can go wrong at, every stage's bytes against the
integer-pipe kernels', and the selection rule.  Sizes are written in the kernel's constants (lfc_mfma_kernels.h):
kLfcMfmaItemTile = 32 images per accumulator tile, kLfcMfmaGroup = 128 images per block and group, kLfcMfmaGrid = 128 groups in
flight, so that 128 * 128 + 1 images give one block a second group (the prefetched one)."""
import functools

import numpy as np
import pytest

import gpu_lib as gl
import oracle_lib as ol
import random_params
from test_gpu_layers import stage_output, unpack

pytestmark = pytest.mark.gpu

TILE, G, GRID = 32, 128, 128
SIZES = [1, TILE - 1, TILE, TILE + 1, G - 1, G, G + 1, 2 * G + 1, G * GRID + 1]
NETS = ["lfcW1A1", "lfcW1A2"]
SETS = [(net, ps) for net in NETS for ps in ("mnist", "random")] + [("lfcW1A1", "chars_merged")]
ALL = 0x1E  # stages 1-4 of kLfcStages: the four layers


@pytest.fixture(scope="module")
def pdirs(tmp_path_factory):
    """(network, parameter set) -> directory; the random sets are made once"""
    out = {}
    for k, (net, ps) in enumerate(SETS):
        if ps == "random":
            out[net, ps] = str(tmp_path_factory.mktemp(net))
            random_params.make(out[net, ps], net, 50 + k)
        else:
            out[net, ps] = gl.param_dir(ps, net)
    return out


def images(n, seed):
    """seeded random bytes, a quarter of the pixels on the binarisation edge"""
    rng = np.random.default_rng(seed)
    px = rng.integers(0, 256, (n, 784), dtype=np.uint8)
    edge = rng.integers(126, 130, (n, 784), dtype=np.uint8)
    return np.where(rng.random((n, 784)) < 0.25, edge, px)


@functools.lru_cache(None)
def reference(net, pdir, ncls):
    """images, the restatement's words and classes: once per parameter set, every size a prefix"""
    imgs = images(SIZES[-1], 38)
    w = ol.Oracle(net, pdir).words_fast(imgs)
    return imgs, w, np.array([ol.lib().bnn_oracle_decode_lfc_batched(int(x), ncls) for x in w], np.int32)


def load(net, pdir):
    L = gl.load(net)
    L.load_parameters(pdir.encode())
    assert L.bnn_mi355x_last_error() == b"", L.bnn_mi355x_last_error()
    return L


@pytest.fixture
def matrix(monkeypatch):
    """load(net, pdir, minimum) with the matrix form switched on; afterwards every library used is reloaded without it"""
    used = []

    def go(net, pdir, minimum=1):
        monkeypatch.setenv("BNN_MI355X_LFC", "mfma")
        monkeypatch.setenv("BNN_MI355X_LFC_MFMA_MIN", str(minimum))
        used.append(net)
        return load(net, pdir)
    yield go
    monkeypatch.delenv("BNN_MI355X_LFC")
    monkeypatch.delenv("BNN_MI355X_LFC_MFMA_MIN")
    for net in used:
        assert load(net, gl.param_dir("mnist", net)).bnn_mi355x_matrix_stages(G) == 0


def run(L, imgs, ncls):
    import torch
    n = len(imgs)
    d = torch.from_numpy(np.ascontiguousarray(imgs)).cuda()
    w, c = torch.zeros(n, dtype=torch.int64, device="cuda"), torch.full((n,), -1, dtype=torch.int32, device="cuda")
    assert L.bnn_mi355x_inference_device(d.data_ptr(), n, ncls, c.data_ptr(), None, w.data_ptr(), None) == 0, L.bnn_mi355x_last_error()
    torch.cuda.synchronize()
    return w.cpu().numpy().view(np.uint64), c.cpu().numpy()


def check(L, net, pdir, ncls, n):
    imgs, want_w, want_c = reference(net, pdir, ncls)
    w, c = run(L, imgs[:n], ncls)
    bad = np.nonzero((w != want_w[:n]) | (c != want_c[:n]))[0]
    assert bad.size == 0, "%s, %d images: %d differ, first %s" % (net, n, bad.size, bad[:8].tolist())


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("net,ps", SETS)
def test_words_and_classes_equal_the_restatement(net, ps, n, pdirs, matrix):
    ncls = ol.num_classes(ps, net) if ps != "random" else 10
    L = matrix(net, pdirs[net, ps])
    assert L.bnn_mi355x_matrix_stages(n) & ALL == ALL
    check(L, net, pdirs[net, ps], ncls, n)


@pytest.mark.parametrize("net", NETS)
def test_every_stage_equals_the_integer_kernels(net, pdirs, matrix):
    pdir, imgs = pdirs[net, "random"], images(G + 33, 39)
    plain = [stage_output(load(net, pdir), imgs, s) for s in range(4)]
    L = matrix(net, pdir)
    assert L.bnn_mi355x_matrix_stages(len(imgs)) & ALL == ALL
    for s in range(4):
        assert (stage_output(L, imgs, s) == plain[s]).all(), "stage %d" % s
    if net == "lfcW1A1":  # the chain's first link against the restatement itself
        o, got = ol.Oracle(net, pdir), stage_output(L, imgs, 1)
        for i in range(len(imgs)):
            assert (unpack(got[i], 1, 1024, 1) == o.layer_ref(imgs[i], 0)).all(), "image %d" % i


@pytest.mark.parametrize("net", NETS)
def test_selection(net, pdirs, matrix):
    pdir = pdirs[net, "mnist"]
    L = load(net, pdir)
    assert [L.bnn_mi355x_matrix_stages(n) for n in (0, 1, 131072)] == [0, 0, 0]
    L = matrix(net, pdir, 300)
    assert [L.bnn_mi355x_matrix_stages(n) & ALL for n in (0, 299, 300)] == [0, 0, ALL]
    for n in (299, 300):
        check(L, net, pdir, 10, n)


def test_matrix_stages_before_load_parameters():
    """a fresh process: nothing loaded, -1 whatever the switch says"""
    import os
    import subprocess
    import sys
    code = "import sys; sys.path.insert(0, %r)\nimport gpu_lib as gl\nprint('stages', gl.load('lfcW1A1').bnn_mi355x_matrix_stages(128))\n" % os.path.dirname(__file__)
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, BNN_MI355X_LFC="mfma"), capture_output=True, text=True, timeout=300)
    assert "stages -1" in out.stdout, out.stdout[-1000:] + out.stderr[-2000:]
