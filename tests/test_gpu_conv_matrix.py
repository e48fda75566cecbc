"""GPU: cnvW1A1 layers 1-3 on the matrix pipe (k_conv_mfma, DESIGN.md 5 "The matrix pipe") -- the throughput path from
conv_mfma_min() images on.  Every bit of the three stages against the faithful scalar restatement on small batches (the
policy forced down with BNN_MI355X_CONV_MFMA_MIN=1), the policy edge, the forked 131 072-image pass against the
XNOR-popcount kernels (BNN_MI355X_CONV=valu) byte for byte, and the places where the blob changes (a fault campaign's
persistent row patches, a blob imported from device memory).  The switches are read once per process: each
configuration runs in a child process."""
import os
import subprocess
import sys

import numpy as np
import pytest

import gpu_lib as gl

pytestmark = pytest.mark.gpu

TESTS = os.path.dirname(os.path.abspath(__file__))
PRELUDE = (
    "import sys, ctypes as C, numpy as np; sys.path[:0] = [%r, %r]\n"
    "import torch, gpu_lib as gl, oracle_lib as ol\n"
    "from test_gpu_layers import stage_output, unpack\n"
    "L = gl.load('cnvW1A1')\n"
    "def load(pdir):\n"
    "    L.load_parameters(pdir.encode()); assert L.bnn_mi355x_last_error() == b''\n"
    "def net():\n"
    "    n = gl.Net.__new__(gl.Net); n.L, n.network, n.is_cnv, n.isz = L, 'cnvW1A1', True, 3072\n"
    "    return n\n"
    "SHIPPED = gl.param_dir('cifar10', 'cnvW1A1')\n" % (TESTS, os.path.join(gl.ROOT, "bnn-pynq_amd")))
STAGES = ((1, 196, 64), (2, 144, 128), (3, 25, 128))  # stage, pixels, channels


def child(code, timeout=900, **env):
    e = dict(os.environ)
    for k in ("BNN_MI355X_CONV", "BNN_MI355X_CONV_MFMA_MIN", "BNN_MI355X_L1"):
        e.pop(k, None)
    e.update({k: str(v) for k, v in env.items()})
    out = subprocess.run([sys.executable, "-c", PRELUDE + code + "\nprint('child-ok')\n"], env=e, capture_output=True, text=True,
                         timeout=timeout)
    assert "child-ok" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]
    return out.stdout


def policy_min():
    import re
    with open(os.path.join(gl.ROOT, "bnn-pynq_amd", "csrc", "kernels.hip")) as f:
        src = f.read()
    return int(re.search(r'getenv\("BNN_MI355X_CONV_MFMA_MIN"\);\s*return e \? std::atoll\(e\) : (\d+)LL;', src).group(1))


def test_stages_1_to_3_bit_exact_small_batches(tmp_path):
    """the matrix forms on 1, 2, 5, 33 and 203 images (ragged last groups and tiles), shipped and random parameters
    (never / always firing thresholds among them): every bit of stages 1-3 against Oracle.layer_ref, and the whole
    network's raw scores on 3 001 images against scores_fast"""
    import random_params
    random_params.make(str(tmp_path), "cnvW1A1", 31)
    child(
        "for pdir in (SHIPPED, %r):\n"
        "    load(pdir); o = ol.Oracle('cnvW1A1', pdir)\n"
        "    for n in (1, 2, 5, 33, 203):\n"
        "        imgs = np.random.default_rng(70 + n).integers(0, 256, (n, 3072), dtype=np.uint8)\n"
        "        for stage, pixels, channels in %r:\n"
        "            raw = stage_output(L, imgs, stage)\n"
        "            for i in sorted({0, n - 1} | set(range(0, n, 7))):\n"
        "                assert (unpack(raw[i], pixels, channels, 1) == o.layer_ref(imgs[i], stage)).all(), (pdir, n, stage, i)\n"
        "    imgs = np.random.default_rng(9).integers(0, 256, (3001, 3072), dtype=np.uint8)\n"
        "    assert (net().raw(imgs) == o.scores_fast(imgs)).all(), pdir\n" % (str(tmp_path), STAGES),
        BNN_MI355X_CONV_MFMA_MIN=1)


def test_policy_edge():
    """min - 1 images (XNOR-popcount kernels) against min images (matrix forms): the same stage outputs"""
    m = policy_min()
    assert 1 < m <= 65536
    child(
        "load(SHIPPED)\n"
        "imgs = np.random.default_rng(5).integers(0, 256, (%d, 3072), dtype=np.uint8)\n"
        "for stage, pixels, channels in %r:\n"
        "    a = stage_output(L, imgs[:-1], stage); b = stage_output(L, imgs, stage)\n"
        "    assert (a == b[:-1]).all(), stage\n" % (m, STAGES))


def _dump_forked(path):
    return (
        "load(SHIPPED)\n"
        "imgs = np.random.default_rng(13).integers(0, 256, (131072, 3072), dtype=np.uint8)\n"
        "d = torch.from_numpy(imgs).cuda(); cls = torch.zeros(131072, dtype=torch.int32, device='cuda')\n"
        "sc = torch.zeros((131072, 64), dtype=torch.int16, device='cuda')\n"
        "assert L.bnn_mi355x_inference_device(d.data_ptr(), 131072, 10, cls.data_ptr(), sc.data_ptr(), None, None) == 0\n"
        "torch.cuda.synchronize()\n"
        "st = [stage_output(L, imgs[:16384], s) for s, _, _ in %r]\n"
        "np.savez(%r, cls=cls.cpu().numpy(), sc=sc.cpu().numpy(), s1=st[0], s2=st[1], s3=st[2])\n" % (STAGES, str(path)))


def test_forked_pass_equals_xnor_kernels(tmp_path):
    """131 072 images through the device entry point (the pass forks over two lanes of 65 536): classes and raw
    scores equal those of the XNOR-popcount kernels byte for byte, stage 1-3 outputs of a 16 384-image host call too,
    and 2 048 of the images equal the restatement"""
    child(_dump_forked(tmp_path / "mfma.npz"))
    child(_dump_forked(tmp_path / "valu.npz"), BNN_MI355X_CONV="valu")
    a, b = np.load(tmp_path / "mfma.npz"), np.load(tmp_path / "valu.npz")
    for k in ("cls", "sc", "s1", "s2", "s3"):
        assert (a[k] == b[k]).all(), k
    import oracle_lib as ol
    imgs = np.random.default_rng(13).integers(0, 256, (131072, 3072), dtype=np.uint8)
    pick = np.random.default_rng(1).choice(131072, 2048, replace=False)
    o = ol.Oracle("cnvW1A1", gl.param_dir("cifar10", "cnvW1A1"))
    assert (a["sc"][pick] == o.scores_fast(imgs[pick])).all()


def _after_faults(path, tmp):
    return (
        "load(SHIPPED)\n"
        "imgs = np.random.default_rng(21).integers(0, 256, (300, 3072), dtype=np.uint8)\n"
        "f = %r\n"
        "np.concatenate([np.ones((300, 1), np.uint8), imgs], axis=1).tofile(f)\n"
        "assert L.bnn_mi355x_set_fault_seed(77) == 0\n"
        "cnt = C.c_int(0)\n"
        "p = L.inference_multiple_with_faults(f.encode(), 10, C.byref(cnt), None, 400, 1, -1, (C.c_int * 3)(1, 2, 3), 3)\n"
        "assert p and cnt.value == 300, L.bnn_mi355x_last_error()\n"
        "camp = np.ctypeslib.as_array(p, shape=(300,)).copy(); L.free_results(p)\n"
        "big = np.random.default_rng(22).integers(0, 256, (8192, 3072), dtype=np.uint8)\n"
        "np.savez(%r, camp=camp, sc=net().raw(big))\n" % (str(tmp / "imgs.bin"), str(path)))


def test_plain_call_after_fault_campaign(tmp_path):
    """inference_multiple_with_faults patches rows of layers 1-3 and the patches persist: the next plain call (matrix
    forms, 8 192 images) classifies with the patched weights -- the same scores as under BNN_MI355X_CONV=valu"""
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    child(_after_faults(tmp_path / "mfma.npz", tmp_path / "a"))
    child(_after_faults(tmp_path / "valu.npz", tmp_path / "b"), BNN_MI355X_CONV="valu")
    a, b = np.load(tmp_path / "mfma.npz"), np.load(tmp_path / "valu.npz")
    assert (a["camp"] == b["camp"]).all()
    assert (a["sc"] == b["sc"]).all()


def test_blob_imported_from_device(tmp_path):
    """a random parameter set's blob imported from device memory (the host never sees the parameter files) gives the
    matrix forms the same tables as load_parameters: equal scores on 8 192 images, equal to the restatement"""
    import random_params
    random_params.make(str(tmp_path), "cnvW1A1", 32)
    child(
        "pdir = %r\n"
        "imgs = np.random.default_rng(23).integers(0, 256, (8192, 3072), dtype=np.uint8)\n"
        "load(pdir); want = net().raw(imgs)\n"
        "load(SHIPPED)\n"
        "size = L.bnn_mi355x_params_bytes(); blob = gl.pack_params('cnvW1A1', pdir); assert blob.size == size\n"
        "d = torch.from_numpy(blob).cuda()\n"
        "assert L.bnn_mi355x_import_params_device(d.data_ptr(), size, torch.cuda.current_stream().cuda_stream) == 0\n"
        "got = net().raw(imgs)\n"
        "assert (got == want).all()\n"
        "assert (got[:512] == ol.Oracle('cnvW1A1', pdir).scores_fast(imgs[:512])).all()\n" % str(tmp_path))
