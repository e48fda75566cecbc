"""GPU: every kernel form on the saturated parameter sets of tests/saturated_params.py -- accumulators at 0, 1, mw - 1, mw
matches, at d = +-mw and +-2 mw, thresholds at and one below the accumulator, at the neighbours of the tables' clamps and
at the int16 extremes; all-zero rows, rows of -2 in every column.  Every comparison is exact, against the generator's
closed form (tests/test_saturated_params.py has shown it equal to the faithful scalar restatement) or, for the
matched-filter and layer-0 sets, against the restatement itself.

The switches are read once per process: each form runs in a child process under its own timeout.  A child makes its own
sets (the generator is deterministic), runs every configuration and leaves nothing behind; the parent's libraries are
never loaded with a crafted set."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import dispatch_forms as df
import gpu_lib as gl
import saturated_params as sp

pytestmark = pytest.mark.gpu

TESTS = os.path.dirname(os.path.abspath(__file__))
CNV = ("cnvW1A1", "cnvW1A2", "cnvW2A2")
LFC = ("lfcW1A1", "lfcW1A2")
SWITCHES = ("BNN_MI355X_CONV", "BNN_MI355X_CONV_MFMA_MIN", "BNN_MI355X_TAIL_MFMA_MIN", "BNN_MI355X_L1", "BNN_MI355X_L0",
            "BNN_MI355X_L0_TILE_MIN", "BNN_MI355X_LFC_BLOCK_MAX", "BNN_MI355X_LFC_FUSED_MAX", "BNN_MI355X_LANES")
MATRIX = {"BNN_MI355X_CONV_MFMA_MIN": "1", "BNN_MI355X_TAIL_MFMA_MIN": "1"}
L17 = 0xFE     # bnn_mi355x_matrix_stages: layers 1-7
# form -> (switches, wanted value of matrix_stages & L17 on small batches or None)
CNV_FORMS = {"default": ({}, None), "matrix": (MATRIX, L17), "valu": ({"BNN_MI355X_CONV": "valu"}, 0),
             "l0-valu": ({"BNN_MI355X_L0": "valu"}, None), "l0-tile": ({"BNN_MI355X_L0_TILE_MIN": "1"}, None)}
L1_FORMS = {"l1-mfma": ({"BNN_MI355X_L1": "mfma"}, None), "l1-lds": ({"BNN_MI355X_L1": "lds"}, None)}
LFC_FORMS = {"default": {}, "staged": {"BNN_MI355X_LFC_BLOCK_MAX": "0"}, "block": {"BNN_MI355X_LFC_BLOCK_MAX": "1000000"}}


def child(main, env, *args, timeout=600):
    e = dict(os.environ)
    for k in SWITCHES:
        e.pop(k, None)
    e.update(env)
    code = "import sys; sys.path[:0] = [%r, %r]\nimport torch\nimport test_gpu_saturation as t\nt.%s(*%r)\nprint('child-ok')\n" % (
        TESTS, os.path.join(gl.ROOT, "bnn-pynq_amd"), main, args)
    out = subprocess.run([sys.executable, "-c", code], env=e, capture_output=True, text=True, timeout=timeout)
    assert "child-ok" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


# ---------------------------------------------------------------------------------------------------------------------
# what the children run
# ---------------------------------------------------------------------------------------------------------------------
def _load(L, pdir):
    L.load_parameters(pdir.encode())
    assert L.bnn_mi355x_last_error() == b"", L.bnn_mi355x_last_error()


def _net(L, network):
    n = gl.Net.__new__(gl.Net)
    n.L, n.network, n.is_cnv = L, network, network.startswith("cnv")
    n.isz = 3072 if n.is_cnv else 784
    return n


def _sets(network, tmp):
    """every configuration: (name, directory, expected)"""
    out = []
    for config, neg2 in sp.variants(network):
        name = config + ("/neg2" if neg2 else "")
        d = os.path.join(tmp, name.replace("/", "_"))
        out.append((name, d, sp.make(d, network, config, neg2)[2]))
    return out


def _cnv_images(n, seed):
    """random images, the first all 0 and the last all 255"""
    imgs = np.random.default_rng(seed).integers(0, 256, (n, 3072), dtype=np.uint8)
    imgs[0] = 0
    imgs[-1] = 255 if n > 1 else imgs[-1]
    return imgs


def _cls_cnv(scores):
    import oracle_lib as ol
    return ol.decode_cnv_batched(scores, 10)


def _cls_lfc(word):
    import oracle_lib as ol
    return ol.lib().bnn_oracle_decode_lfc_batched(int(word), 10)


def _cnv_stages(L, network, name, E, want_bits):
    """every stage on 1, 2, 5 and 33 images against the closed form, and the scores of the same images"""
    from test_gpu_layers import stage_output, unpack
    planes = 2 if network.endswith("A2") else 1
    for n in (1, 2, 5, 33):
        if want_bits is not None:
            assert L.bnn_mi355x_matrix_stages(n) & L17 == want_bits, (name, n, L.bnn_mi355x_matrix_stages(n))
        imgs = _cnv_images(n, 300 + n)
        for stage, (pixels, channels) in enumerate(sp.CNV_SHAPE):
            raw = stage_output(L, imgs, stage)
            got = unpack(raw[0], pixels, channels, planes)
            bad = np.nonzero(got != E["layers"][stage])[0]
            if bad.size:     # the closed form says which catalogue case a row is
                rows = sorted(set((bad % channels).tolist()))
                D = E["design"][stage]
                what = [(r, D["weights"][r], D["thresholds"][r], int(D["acc"][r])) for r in rows[:6]] if D["weights"] else rows[:6]
                raise AssertionError("%s %s, %d images, stage %d: %d values differ, rows %s" % (network, name, n, stage, bad.size, what))
            assert (raw == raw[0]).all(), (name, n, stage, "images differ")
        assert (_net(L, network).raw(imgs) == E["scores"][None]).all(), (name, n)


def _cnv_device_pass(L, E, m, seed=1):
    """one device call of m device-generated random images (a few slots all 0 / all 255): every row equals the one expected"""
    import torch
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    d = torch.randint(0, 256, (m, 3072), dtype=torch.uint8, device="cuda", generator=g)
    _cnv_sweep(L, E, d, [m], "pass")


def _cnv_sweep(L, E, d, sizes, what):
    import torch
    for i, v in ((0, 0), (1, 255), (len(d) // 2, 0), (len(d) - 1, 255)):
        if i < len(d):
            d[i] = v
    want = torch.from_numpy(E["scores"].copy()).cuda()
    want_cls = _cls_cnv(E["scores"])
    sc = torch.empty((len(d), 64), dtype=torch.int16, device="cuda")
    cls = torch.empty(len(d), dtype=torch.int32, device="cuda")
    for m in sizes:
        sc.fill_(12345)
        cls.fill_(-1)
        torch.cuda.synchronize()
        rc = L.bnn_mi355x_inference_device(d.data_ptr(), m, 10, cls.data_ptr(), sc.data_ptr(), None, None)
        assert rc == 0, (what, m, L.bnn_mi355x_last_error())
        torch.cuda.synchronize()
        bad = (sc[:m] != want[None]).any(1) | (cls[:m] != want_cls)
        assert not bool(bad.any()), (what, m, torch.nonzero(bad).flatten()[:8].tolist(), sc[int(torch.nonzero(bad)[0])].tolist())
        assert bool((cls[m:] == -1).all()) and bool((sc[m:] == 12345).all()), (what, m, "written beyond the call's images")


def _campaign(L, path, runs, nrates):
    rq = (C.c_uint * nrates)(*([0] * nrates))
    cnt, usec = C.c_int(0), C.c_float(0)
    p = L.bnn_mi355x_act_noise_campaigns(path.encode(), 10, runs, 77, rq, nrates, C.byref(cnt), C.byref(usec))
    assert p, L.bnn_mi355x_last_error().decode()
    got = np.ctypeslib.as_array(p, shape=(runs * cnt.value,)).copy().reshape(runs, cnt.value)
    L.free_results(p)
    return got


def _blob_import(L, network, pdir, shipped, imgs, want):
    """the crafted blob imported from device memory: the device-built tables give what load_parameters gave"""
    import torch
    _load(L, shipped)
    size = L.bnn_mi355x_params_bytes()
    blob = gl.pack_params(network, pdir)
    assert blob.size == size
    d = torch.from_numpy(blob).cuda()
    assert L.bnn_mi355x_import_params_device(d.data_ptr(), size, torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    assert (_net(L, network).raw(imgs) == want).all()


def _layer0_set(directory, network):
    """layer 0 with rows of all +1, all -1 and (cnvW2A2) all -2 whose file thresholds put the blob threshold (half the
    file's, rounded down) one below, at and one above the row's dot product on the all-0 or the all-255 image"""
    import random_params
    from bnn import params_io
    W, T = random_params.make(directory, network, 91, **({"neg2": 0.02} if network == "cnvW2A2" else {}))
    vals = [1, -1] + ([-2] if network == "cnvW2A2" else [])
    n = 0
    for w in vals:
        for q in (-128, 127):                          # the quantised all-0 / all-255 pixel
            acc = 2 * 27 * w * q
            for off in (-2, -1, 0, 1, 2):
                W[0][n] = w
                T[0][n] = acc + off if T[0].shape[1] == 1 else ((acc + off, acc + off), (acc + off, acc - off))[n % 2]
                n += 1
    assert n <= 64
    params_io.write_params(directory, network, W, T, classes=[str(i) for i in range(10)])


def _layer0(L, network, tmp):
    import oracle_lib as ol
    from test_gpu_layers import stage_output, unpack
    d = os.path.join(tmp, "layer0")
    _layer0_set(d, network)
    _load(L, d)
    o = ol.Oracle(network, d)
    imgs = _cnv_images(9, 17)
    imgs[1] = 255
    imgs[2] = 0
    want = [o.layer_ref(i, 0) for i in imgs]
    assert len({w[:30].tobytes() for w in want[:2]}) == 2          # (the crafted rows tell the two images apart)
    for n in (2, 9):
        raw = stage_output(L, imgs[:n], 0)
        for i in range(n):
            assert (unpack(raw[i], 900, 64, 2 if network.endswith("A2") else 1) == want[i]).all(), (network, "layer 0", n, i)


def _matched(L, network, tmp):
    """the matched-filter sets of the pooled layers 1 and 3 against the restatement: 1 and 33 images"""
    import oracle_lib as ol
    from test_gpu_layers import stage_output, unpack
    planes = 2 if network.endswith("A2") else 1
    for layer in (1, 3):
        d = os.path.join(tmp, "matched%d" % layer)
        img = np.random.default_rng(40 + layer).integers(0, 256, 3072, dtype=np.uint8)
        sp.make_matched(d, network, 60 + layer, layer, img)
        _load(L, d)
        o = ol.Oracle(network, d)
        imgs = _cnv_images(33, 50 + layer)
        imgs[[0, 16, 32]] = img
        want = {i: o.layer_ref(imgs[i], layer) for i in (0, 1)}
        pixels, channels = sp.CNV_SHAPE[layer]
        for n in (1, 33):
            raw = stage_output(L, imgs[:n], layer)
            for i in (0, 1, 16, 32):
                if i < n:
                    assert (unpack(raw[i], pixels, channels, planes) == want[0 if i != 1 else 1]).all(), (network, "matched", layer, n, i)


def _cnv_main(network, form, tmp):
    """one form of one CNV net: every configuration's stages and scores on small batches and one device pass; layer 0
    at its thresholds' edges; the matched-filter sets; in the default and the matrix form also a multi-run campaign
    without faults and the blob import"""
    L = gl.load(network)
    shipped = gl.param_dir("cifar10", network)
    want_bits = dict(CNV_FORMS, **L1_FORMS)[form][1]
    for name, d, E in _sets(network, tmp):
        _load(L, d)
        _cnv_stages(L, network, name, E, want_bits)
        _cnv_device_pass(L, E, 3001)
        if form in ("default", "matrix") and name.startswith("mixed"):
            imgs = _cnv_images(6, 5)
            path = os.path.join(tmp, "six.bin")
            np.concatenate([np.ones((6, 1), np.uint8), imgs], axis=1).tofile(path)
            if form == "default":      # (the campaign entry points run the integer-pipe MULTI kernels whatever the switches)
                assert (_campaign(L, path, 3, 8) == _cls_cnv(E["scores"])).all(), name
            _blob_import(L, network, d, shipped, imgs, E["scores"][None])
    _layer0(L, network, tmp)
    _matched(L, network, tmp)


def _cnv_sweep_main(network, tmp):
    """every size of dispatch_forms.edges() and the size before it, every configuration (the -2 sets on their own edges)"""
    import torch
    L = gl.load(network)
    g = torch.Generator(device="cuda")
    g.manual_seed(2)
    d = torch.randint(0, 256, (df.NMAX, 3072), dtype=torch.uint8, device="cuda", generator=g)
    for name, pdir, E in _sets(network, tmp):
        two = name.endswith("neg2")
        sizes = sorted({x for e in df.edges(lambda n: df.cnv_forms(n, network, two)) for x in (e - 1, e)} | {1, df.NMAX})
        _load(L, pdir)
        _cnv_sweep(L, E, d, sizes, "%s %s" % (network, name))


def _lfc_main(network, form, tmp):
    """one form of one LFC net: every stage on the crafted images tiled to 1, 3, 64 and 257, the words at every policy
    edge (device calls on the images tiled to 131 072), a campaign without faults, the blob import"""
    import torch
    from test_gpu_layers import stage_output, unpack
    L = gl.load(network)
    planes = 2 if network.endswith("A2") else 1
    block_max = {"default": None, "staged": 0, "block": 1000000}[form]
    edges = df.edges(lambda n: df.lfc_forms(n, network, None, block_max) if network == "lfcW1A1" else df.lfc_forms(n, network))
    sizes = sorted({x for e in edges for x in (e - 1, e)} | {1, df.NMAX})
    idx = np.arange(df.NMAX) % 4
    for name, pdir, E in _sets(network, tmp):
        _load(L, pdir)
        for n in (1, 3, 64, 257):
            imgs = E["images"][idx[:n]]
            bits = np.unpackbits(stage_output(L, imgs, 0), axis=1, bitorder="little")
            assert (bits[:, :784] == (imgs >= 128)).all() and (bits[:, 784:] == 0).all()
            for layer in range(3):
                raw = stage_output(L, imgs, layer + 1)
                for i in range(n):
                    assert (unpack(raw[i], 1, 1024, planes) == E["layers"][layer][i % 4]).all(), (name, n, layer, i)
            assert (_net(L, network).raw(imgs) == np.array(E["words"], np.uint64)[idx[:n]]).all(), (name, n)
        words = np.array(E["words"], np.uint64)
        didx = torch.arange(df.NMAX, device="cuda") % 4                      # tiled on the device
        d = torch.from_numpy(E["images"]).cuda()[didx].contiguous()
        want = torch.from_numpy(words.view(np.int64)).cuda()[didx]
        want_cls = torch.from_numpy(np.array([_cls_lfc(w) for w in words], np.int32)).cuda()[didx]
        out = torch.empty(df.NMAX, dtype=torch.int64, device="cuda")
        cls = torch.empty(df.NMAX, dtype=torch.int32, device="cuda")
        for m in sizes:
            out.fill_(-1)
            cls.fill_(-1)
            torch.cuda.synchronize()
            assert L.bnn_mi355x_inference_device(d.data_ptr(), m, 10, cls.data_ptr(), None, out.data_ptr(), None) == 0, (name, m)
            torch.cuda.synchronize()
            assert bool((out[:m] == want[:m]).all()) and bool((cls[:m] == want_cls[:m]).all()), (name, m)
            assert bool((cls[m:] == -1).all()), (name, m)
        if name == "mixed":
            path = os.path.join(tmp, "four.idx")
            with open(path, "wb") as f:
                f.write(bytes([0, 0, 8, 3, 0, 0, 0, 4, 0, 0, 0, 28, 0, 0, 0, 28]))
                f.write(E["images"].tobytes())
            assert (_campaign(L, path, 3, 3) == np.array([_cls_lfc(w) for w in words])[None]).all()
            _blob_import(L, network, pdir, gl.param_dir("mnist", network), E["images"], words)


# ---------------------------------------------------------------------------------------------------------------------
# the tests
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", list(CNV_FORMS))
@pytest.mark.parametrize("network", CNV)
def test_cnv_saturated_sets(network, form, tmp_path):
    """stages 0-7 and the scores of every configuration on 1, 2, 5 and 33 images against the closed form, a 3 001-image
    device pass, layer 0 at the edges of its thresholds and the matched-filter sets of layers 1 and 3 against the
    restatement: in the default small-batch forms, with layers 1-7 forced onto the matrix cores (bits 1-7 of
    bnn_mi355x_matrix_stages asserted), on the integer pipe, and with layer 0 in its valu and tile forms"""
    child("_cnv_main", CNV_FORMS[form][0], network, form, str(tmp_path))


@pytest.mark.parametrize("form", list(L1_FORMS))
def test_cnvW1A1_layer1_comparison_forms(form, tmp_path):
    child("_cnv_main", L1_FORMS[form][0], "cnvW1A1", form, str(tmp_path))


@pytest.mark.parametrize("valu", (False, True), ids=("default", "valu"))
@pytest.mark.parametrize("network", CNV)
def test_cnv_policy_edges(network, valu, tmp_path):
    """the network's output does not depend on the image: one device call per edge size of dispatch_forms.edges() (and
    the size before it) on device-generated random images, a few slots all 0 / all 255, every row of scores and classes
    compared on the device with the one expected row; under the committed policy and on the integer pipe alone"""
    child("_cnv_sweep_main", {"BNN_MI355X_CONV": "valu"} if valu else {}, network, str(tmp_path))


@pytest.mark.parametrize("network,form", [("lfcW1A1", f) for f in LFC_FORMS] + [("lfcW1A2", "default")])
def test_lfc_saturated_sets(network, form, tmp_path):
    """every stage on the crafted images tiled to 1, 3, 64 and 257 and the output words at every policy edge: the
    one-launch kernel at 1, 2, 4 and 8 images per block, the block kernel and the staged forms"""
    child("_lfc_main", LFC_FORMS[form], network, form, str(tmp_path))
