"""GPU: layer 0's tile form (k_conv0_tile, forced onto small batches with BNN_MI355X_L0_TILE_MIN=1) against the integer
form k_conv0 (BNN_MI355X_L0=valu), which shares none of its code: stage-0 output bytes of the same images, for the
three CNV nets, at the block edges -- n in {1, I - 1, I, I + 1, 2 I + 1} for I images per block -- on images built so
that a run fetched a byte, a row or a plane off, a wrong shift, a missed ragged image, the padding behind a plane or
stale LDS from the call before changes bits.  Each form runs in one child process (the forms are chosen at load time)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import gpu_lib as gl

pytestmark = pytest.mark.gpu

NETS = ("cnvW1A1", "cnvW1A2", "cnvW2A2")
CHILD = r"""
import sys
import numpy as np
sys.path[:0] = [%(tests)r, %(pkg)r]
import torch  # first: one HIP runtime per process
import gpu_lib as gl
from test_gpu_layers import stage_output
from test_gpu_conv0_tile_edges import cases, images
out, loaded = {}, None
for net, name, pdir, n in cases(%(dirs)r):
    if loaded != (net, name):
        L = gl.load(net)
        L.load_parameters(pdir.encode()); assert L.bnn_mi355x_last_error() == b''
        loaded = (net, name)
    for call in (0, 1):  # the second call: other images through the same LDS and buffers
        out['%%s/%%s/%%d/%%d' %% (net, name, n, call)] = stage_output(L, images(n, call), 0).copy()
np.savez(%(dst)r, **out)
print('edges-done')
"""


def images_per_block():
    with open(os.path.join(gl.ROOT, "bnn-pynq_amd", "csrc", "kernels.hip")) as f:
        return int(re.search(r"constexpr int kL0Imgs = (\d+);", f.read()).group(1))


def sizes():
    i = images_per_block()
    return sorted({1, i - 1, i, i + 1, 2 * i + 1} - {0})


def images(n, call):
    """image k of a call is one of three kinds, in turn: every byte a distinct function of (c, y, x); bytes at the edges of
    the quantiser; random.  The second call starts the turn one kind later and draws other values"""
    rng = np.random.default_rng(1000 * n + call)
    c, y, x = np.meshgrid(np.arange(3), np.arange(32), np.arange(32), indexing="ij")
    out = np.empty((n, 3072), np.uint8)
    for k in range(n):
        kind = (k + call) % 3
        if kind == 0:
            out[k] = ((37 * x + 101 * y + 53 * c + 29 * k + 7 * call) & 255).astype(np.uint8).reshape(-1)
        elif kind == 1:
            out[k] = rng.choice(np.array([0, 1, 127, 128, 254, 255], np.uint8), 3072)
        else:
            out[k] = rng.integers(0, 256, 3072, dtype=np.uint8)
    return out


def cases(dirs):
    for net in NETS:
        for name, pdir in (("shipped", gl.param_dir("cifar10", net)),) + tuple(sorted(dirs[net].items())):
            for n in sizes():
                yield net, name, pdir, n


def make_params(tmp):
    """per net besides the shipped set: cnvW1A1: the boundary set of threshold_params (layers 1-3 rewritten), with layer 0's
    thresholds set the same way -- of four consecutive neurons one always fires, one never, two within 3 of the
    accumulator's mean (0: +-1 weights on centred inputs) -- so that one tap off flips bits; the others: a random set"""
    import random_params
    import threshold_params
    from bnn import params_io
    dirs = {}
    d = os.path.join(tmp, "cnvW1A1-boundary")
    os.makedirs(d)
    threshold_params.make_base(d, 24)
    threshold_params.boundary(d, 24)
    rng = np.random.default_rng(24)
    mh = params_io.layout("cnvW1A1")[0]["mh"]
    kind = (np.arange(mh) + 1) % 4
    lo, hi = -(1 << 23), (1 << 23) - 1
    threshold_params._write_thresholds(d, 0, np.where(kind == 0, lo, np.where(kind == 1, hi, rng.integers(-3, 4, mh))))
    dirs["cnvW1A1"] = {"boundary": d}
    for k, net in enumerate(NETS[1:]):
        d = os.path.join(tmp, net + "-random")
        os.makedirs(d)
        random_params.make(d, net, 240 + k, **({"neg2": 0.04} if net == "cnvW2A2" else {}))
        dirs[net] = {"random": d}
    return dirs


def run_form(env, dirs, dst):
    code = CHILD % {"tests": os.path.join(gl.ROOT, "tests"), "pkg": os.path.join(gl.ROOT, "bnn-pynq_amd"), "dirs": dirs, "dst": dst}
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True, timeout=600)
    assert "edges-done" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]
    return np.load(dst)


@pytest.fixture(scope="module")
def both_forms(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("l0edges"))
    dirs = make_params(tmp)
    tile = run_form({"BNN_MI355X_L0_TILE_MIN": "1"}, dirs, os.path.join(tmp, "tile.npz"))
    valu = run_form({"BNN_MI355X_L0": "valu"}, dirs, os.path.join(tmp, "valu.npz"))
    return dirs, tile, valu


def test_images_differ_between_the_calls_and_cover_the_quantiser_edges():
    a, b = images(9, 0), images(9, 1)
    assert (a != b).any(axis=1).all()
    assert set(np.unique(a[1])) == {0, 1, 127, 128, 254, 255}
    # the pattern image: no two of a window's 27 taps equal at (0, 0), and a byte / row / plane off is another value
    p = a[0].reshape(3, 32, 32)
    assert p[0, 0, 0] != p[0, 0, 1] and p[0, 0, 0] != p[0, 1, 0] and p[0, 0, 0] != p[1, 0, 0]


@pytest.mark.parametrize("net", NETS)
def test_tile_form_equals_integer_form_at_block_edges(both_forms, net):
    dirs, tile, valu = both_forms
    per_pixel = 16 if net.endswith("A2") else 8  # bytes: [pixel][C/64][plane][half] dwords / [pixel][2] dwords
    keys = [k for k in tile.files if k.startswith(net + "/")]
    assert len(keys) == 2 * 2 * len(sizes()) and sorted(valu.files) == sorted(tile.files)
    for k in keys:
        t, v = tile[k], valu[k]
        assert t.shape == v.shape and t.shape[1] == 900 * per_pixel, (k, t.shape, v.shape)
        if (t != v).any():
            img, byte = np.argwhere(t != v)[0]
            pix = byte // per_pixel
            raise AssertionError("%s: image %d of %d, output row %d column %d differs (%d bytes in all; rows %s, columns %s)" % (
                k, img, t.shape[0], pix // 30, pix % 30, int((t != v).sum()),
                sorted(set((np.argwhere(t != v)[:, 1] // per_pixel // 30).tolist()))[:8],
                sorted(set((np.argwhere(t != v)[:, 1] // per_pixel % 30).tolist()))[:8]))
        # what the comparison stands on: the last image of the (ragged) block, the last rows and the last columns hold fired
        # and unfired neurons in both forms, so equal bytes there are not equal zeros
        last = v[-1].reshape(30, 30, per_pixel)
        for part in (last[27:], last[:, 28:]):
            assert 0 < np.unpackbits(part).mean() < 1, k
