"""Every kernel form the batch-size policy can select, on every image of the pass that selects it.

The sizes come from dispatch_forms.edges() (the policy restated from kernels.hip / runtime.hip): each change point and
the size before it, so a retuned threshold moves the sweep with it.  Each call classifies a prefix of one seeded master
batch of 131 072 images (the first 16 384 of quantiser-edge values), so one reference serves every size:
- CNV: the GPU's own smallest forms (calls of 512 images: pixel lanes, one-launch tail) over the whole master, checked
  against the restatement (oracle/) on all images below 6 144, the 256 images either side of every call end and lane
  boundary used here, and every 16th image of the rest; then raw scores and classes of EVERY image of every call against
  that reference, unforked (a child process with BNN_MI355X_LANES=1), forked over the two lanes so that a lane lands on
  each side of each change point, and through a captured graph;
- LFC: words and classes of every image against the restatement itself.
A call must also leave its output buffers alone beyond its own images."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import dispatch_forms as df
import gpu_lib as gl
import oracle_lib as ol
import random_params
from test_gpu_parity import rand_images

pytestmark = pytest.mark.gpu

N = df.NMAX
EDGE_IMAGES = 16384  # the master's first images: quantiser-edge values
SENTINEL = 12345     # scores a kernel never wrote (beyond any |score| of these nets)
# parameter set -> (network, dataset or None for the random -2 set, master seed)
SETS = {"cnvW1A1": ("cnvW1A1", "cifar10", 101), "cnvW1A2": ("cnvW1A2", "cifar10", 102), "cnvW2A2": ("cnvW2A2", "cifar10", 103),
        "cnvW2A2-neg2": ("cnvW2A2", None, 104)}
LFC_SETS = {"lfcW1A1": ("lfcW1A1", "mnist", 105), "lfcW1A2": ("lfcW1A2", "mnist", 106)}
TESTS = os.path.dirname(os.path.abspath(__file__))


def master(network, seed):
    """the seeded batch every call classifies a prefix of"""
    edge = rand_images(network, EDGE_IMAGES, seed, kind="edges")
    rest = rand_images(network, N - EDGE_IMAGES, seed + 1000)
    return np.ascontiguousarray(np.concatenate([edge, rest]))


def neg2_params(directory):
    random_params.make(directory, "cnvW2A2", 5, neg2=0.03)
    return directory


@functools.lru_cache(None)
def cnv_edges(two):
    return tuple(df.edges(lambda n: df.cnv_forms(n, "cnvW2A2", two)))


def unforked_sizes(two):
    return sorted({1, 2, N - 1, N} | {x for e in cnv_edges(two) for x in (e - 1, e)})


def forked_calls(two):
    """(m, first lane, second lane): a device call of m images whose second lane is exactly a change point or the size
    before it (m = 256 ceil(x / 256) + x).  Below 8 192 such a call would not fork; beyond 65 536 no lane can reach."""
    out = []
    for e in cnv_edges(two):
        for x in (e - 1, e):
            h = 256 * -(-x // 256)
            if e > 8192 and h + x <= N:
                assert df.fork_lanes(h + x) == (h, x)
                out.append((h + x, h, x))
    return out


def oracle_sample(cuts):
    keep = np.zeros(N, bool)
    keep[:6144] = True
    keep[::16] = True
    for c in cuts:
        keep[max(c - 256, 0):c + 256] = True
    return np.nonzero(keep)[0]


def load_set(name, pdir):
    """the library of the set's network with the set's parameters loaded"""
    network = (SETS.get(name) or LFC_SETS[name])[0]
    L = gl.load(network)
    L.load_parameters(pdir.encode())
    assert L.bnn_mi355x_last_error() == b"", L.bnn_mi355x_last_error()
    return L


def small_calls_reference(L, is_cnv, d):
    """raw outputs and classes of the whole master through device calls of 512 images (the smallest forms)"""
    import torch
    raw = torch.full((N, 64), SENTINEL, dtype=torch.int16, device="cuda") if is_cnv else torch.zeros(N, dtype=torch.int64, device="cuda")
    cls = torch.full((N,), -1, dtype=torch.int32, device="cuda")
    isz = 3072 if is_cnv else 784
    for b in range(0, N, 512):
        rc = L.bnn_mi355x_inference_device(d.data_ptr() + b * isz, 512, 10, cls.data_ptr() + 4 * b, raw.data_ptr() + 128 * b if is_cnv else None,
                                           None if is_cnv else raw.data_ptr() + 8 * b, None)
        assert rc == 0, L.bnn_mi355x_last_error()
    torch.cuda.synchronize()
    return raw, cls


def sweep(L, is_cnv, d, sizes, ref_raw, ref_cls, forms, what):
    """a device call on the first m images of the master `d` for every m in sizes: raw outputs and classes of every image
    equal to the reference (device tensors), nothing written beyond the m images"""
    import torch
    raw = torch.empty((N, 64), dtype=torch.int16, device="cuda") if is_cnv else torch.empty(N, dtype=torch.int64, device="cuda")
    cls = torch.empty(N, dtype=torch.int32, device="cuda")
    for m in sizes:
        raw.fill_(SENTINEL)
        cls.fill_(-1)
        torch.cuda.synchronize()
        rc = L.bnn_mi355x_inference_device(d.data_ptr(), m, 10, cls.data_ptr(), raw.data_ptr() if is_cnv else None,
                                           None if is_cnv else raw.data_ptr(), None)
        assert rc == 0, (what, m, L.bnn_mi355x_last_error())
        torch.cuda.synchronize()
        bad = (raw[:m] != ref_raw[:m]).reshape(m, -1).any(1) | (cls[:m] != ref_cls[:m])
        if bool(bad.any()):
            idx = torch.nonzero(bad).flatten()
            raise AssertionError("%s, %d images %s: %d images differ, first %s" % (what, m, forms(m), idx.numel(), idx[:8].tolist()))
        assert bool((cls[m:] == -1).all()) and bool((raw[m:] == SENTINEL).all()), (what, m, "written beyond the call's images")


def _unforked_main(name, pdir, out):
    """child process (BNN_MI355X_LANES=1, read once per process): the unforked sweep against this process's own 512-image
    reference, which is saved for the parent to compare with its own (checked against the restatement)"""
    import torch
    network, _, seed = SETS[name]
    two = name.endswith("neg2")
    L = load_set(name, pdir)
    d = torch.from_numpy(master(network, seed)).cuda()
    ref_raw, ref_cls = small_calls_reference(L, True, d)
    sweep(L, True, d, unforked_sizes(two), ref_raw, ref_cls, lambda m: df.cnv_forms(m, network, two), name + " unforked")
    np.save(out + ".raw.npy", ref_raw.cpu().numpy())
    np.save(out + ".cls.npy", ref_cls.cpu().numpy())
    print("unforked-ok")


def _staged_lfc_main(pdir, ref):
    """child process (BNN_MI355X_LFC_FUSED_MAX=0, BNN_MI355X_LFC_BLOCK_MAX=0): lfcW1A1 on its staged kernels"""
    import torch
    network, _, seed = LFC_SETS["lfcW1A1"]
    L = load_set("lfcW1A1", pdir)
    d = torch.from_numpy(master(network, seed)).cuda()
    w = torch.from_numpy(np.load(ref + ".raw.npy").view(np.int64)).cuda()
    c = torch.from_numpy(np.load(ref + ".cls.npy")).cuda()
    sweep(L, False, d, lfc_sizes(), w, c, lambda m: df.lfc_forms(m, network, 0, 0), "lfcW1A1 staged")
    print("staged-ok")


def child(main, env, *args):
    code = "import sys; sys.path[:0] = [%r, %r]\nimport torch\nimport test_gpu_forms as t\nt.%s(*%r)\n" % (
        TESTS, os.path.join(gl.ROOT, "bnn-pynq_amd"), main, args)
    return subprocess.Popen([sys.executable, "-c", code], env=dict(os.environ, **env), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)


def finish(p, token):
    out, err = p.communicate(timeout=900)
    assert token in out, out[-2000:] + err[-4000:]


@pytest.mark.parametrize("name", list(SETS))
def test_cnv_every_form_every_image(name, tmp_path):
    import torch
    network, dataset, seed = SETS[name]
    two = name.endswith("neg2")
    pdir = neg2_params(str(tmp_path)) if two else gl.param_dir(dataset, network)
    out = str(tmp_path / "unforked")
    p = child("_unforked_main", {"BNN_MI355X_LANES": "1"}, name, pdir, out)
    try:
        L = load_set(name, pdir)
        o = ol.Oracle(network, pdir)
        if two:  # the blob really holds -2 rows: every call of this set runs the -2-aware (TWO) kernels
            assert (o.weights(1) == -2).any()
            size = L.bnn_mi355x_export_params(None, 0)
            blob = np.zeros(size, np.uint8)
            assert L.bnn_mi355x_export_params(blob.ctypes.data, size) == size
            assert (blob == gl.pack_params(network, pdir)).all()
        imgs = master(network, seed)
        d = torch.from_numpy(imgs).cuda()
        ref_raw, ref_cls = small_calls_reference(L, True, d)
        forks = forked_calls(two)
        pick = oracle_sample(unforked_sizes(two) + [c for m, h, _ in forks for c in (m, h)])
        want = o.scores_fast(imgs[pick])
        got_raw, got_cls = ref_raw.cpu().numpy(), ref_cls.cpu().numpy()
        bad = np.nonzero((got_raw[pick] != want).any(1))[0]
        assert bad.size == 0, (name, "512-image calls against the restatement", pick[bad[:8]].tolist())
        assert got_cls[pick].tolist() == [ol.decode_cnv_batched(s, 10) for s in want]
        # forked: a lane on each side of each change point, the way bench.py and inference_device users run them
        sweep(L, True, d, [m for m, _, _ in forks], ref_raw, ref_cls,
              lambda m: [df.cnv_forms(x, network, two) for x in df.fork_lanes(m)], name + " forked")
        if two:
            # captured into a graph: the pass runs unforked, all 131 072 images in one lane (the last row of the table)
            sc = torch.full((N, 64), SENTINEL, dtype=torch.int16, device="cuda")
            cls = torch.full((N,), -1, dtype=torch.int32, device="cuda")
            assert L.bnn_mi355x_reserve(N) == 0
            assert L.bnn_mi355x_inference_device(d.data_ptr(), N, 10, cls.data_ptr(), sc.data_ptr(), None, None) == 0   # warm-up
            torch.cuda.synchronize()
            sc.fill_(SENTINEL)
            cls.fill_(-1)
            s, g = torch.cuda.Stream(), torch.cuda.CUDAGraph()
            torch.cuda.synchronize()
            with torch.cuda.graph(g, stream=s):
                rc = L.bnn_mi355x_inference_device(d.data_ptr(), N, 10, cls.data_ptr(), sc.data_ptr(), None, torch.cuda.current_stream().cuda_stream)
            assert rc == 0, L.bnn_mi355x_last_error()
            g.replay()
            torch.cuda.synchronize()
            assert bool((sc == ref_raw).all()) and bool((cls == ref_cls).all()), "captured 131 072-image call"
        finish(p, "unforked-ok")
        # the child's 512-image reference is this one: its sweep is then checked against the restatement as well
        assert (np.load(out + ".raw.npy") == got_raw).all() and (np.load(out + ".cls.npy") == got_cls).all()
    finally:
        if p.poll() is None:
            p.kill()
            p.wait()
        gl.load(network).load_parameters(gl.param_dir("cifar10", network).encode())


def lfc_sizes():
    e = set(df.edges(lambda n: df.lfc_forms(n, "lfcW1A2"))) | set(df.edges(lambda n: df.lfc_forms(n, "lfcW1A1", 0, 0)))
    return sorted({1, N} | {x for v in e for x in (v - 1, v, v + 1)})


def lfc_reference(network, seed, pdir):
    imgs = master(network, seed)
    w = ol.Oracle(network, pdir).words_fast(imgs)
    c = np.array([ol.lib().bnn_oracle_decode_lfc_batched(int(x), 10) for x in w], np.int32)
    return imgs, w, c


def test_lfc_every_form_every_image(tmp_path):
    """lfcW1A2 at its change points +-1 (one-launch kernel at 1/2/4/8 images per block, staged 8- and 32-neuron forms) and
    lfcW1A1 on its staged kernels (BNN_MI355X_LFC_FUSED_MAX=0, BNN_MI355X_LFC_BLOCK_MAX=0) at the same sizes: every word and
    class against the restatement on the whole master"""
    import torch
    network, dataset, seed = LFC_SETS["lfcW1A1"]
    pdir1 = gl.param_dir(dataset, network)
    _, w, c = lfc_reference(network, seed, pdir1)
    ref = str(tmp_path / "lfcW1A1")
    np.save(ref + ".raw.npy", w)
    np.save(ref + ".cls.npy", c)
    p = child("_staged_lfc_main", {"BNN_MI355X_LFC_FUSED_MAX": "0", "BNN_MI355X_LFC_BLOCK_MAX": "0"}, pdir1, ref)
    try:
        network, dataset, seed = LFC_SETS["lfcW1A2"]
        pdir = gl.param_dir(dataset, network)
        imgs, w, c = lfc_reference(network, seed, pdir)
        L = load_set("lfcW1A2", pdir)
        d = torch.from_numpy(imgs).cuda()
        sweep(L, False, d, lfc_sizes(), torch.from_numpy(w.view(np.int64)).cuda(), torch.from_numpy(c).cuda(),
              lambda m: df.lfc_forms(m, network), "lfcW1A2")
        finish(p, "staged-ok")
    finally:
        if p.poll() is None:
            p.kill()
            p.wait()
