"""GPU: the tile epilogue of cnvW1A1 layers 1-3 on the matrix pipe (k_conv_mfma, DESIGN.md 5 "The matrix pipe"): the
vertical pool as an AND of the accumulators' bits, and whatever the epilogue carries from one tile to the next (a
deferred form -- pending tile, store one iteration later, flush behind the wave's last tile of a group -- was built and
measured with this test; CHANGELOG).  Stage 1-3 outputs byte for byte against the XNOR-popcount kernels
(BNN_MI355X_CONV=valu) at the image counts that give a first tile with nothing pending, a ragged last tile, odd and even
tile counts per stream in layer 1 (7 / 6 at one image) and a block's second group on the 512-block grid (1 027 images in
groups of 2, 4 099 in groups of 8); with the shipped parameters and with a random set that has never-firing,
always-firing and exactly-at-threshold rows (the AND pool's edge: an accumulator of exactly +0 in one row, a negative one
in the other).  Every compared run follows a run of the same stage on other images, so a dropped store cannot hide behind
what the buffer held.  The switches are read once per process: each kernel family runs in one child process."""
import numpy as np
import pytest

from test_gpu_conv_matrix import child  # (its prelude gives the children stage_output, from test_gpu_layers)

pytestmark = pytest.mark.gpu

COUNTS = {1: (1, 2, 3, 9, 1027), 2: (1, 2, 3, 9, 4099), 3: (1, 2, 3, 9, 4099)}
SETS = ("shipped", "random")


def _dump(path, random_dir):
    return (
        "out = {}\n"
        "for name, pdir in (('shipped', SHIPPED), ('random', %r)):\n"
        "    load(pdir)\n"
        "    for stage, counts in %r.items():\n"
        "        for n in counts:\n"
        "            other = np.random.default_rng(900 + n).integers(0, 256, (n, 3072), dtype=np.uint8)\n"
        "            imgs = np.random.default_rng(800 + n).integers(0, 256, (n, 3072), dtype=np.uint8)\n"
        "            stage_output(L, other, stage)\n"
        "            out['%%s_%%d_%%d' %% (name, stage, n)] = stage_output(L, imgs, stage)\n"
        "np.savez(%r, **out)\n" % (random_dir, COUNTS, str(path)))


@pytest.fixture(scope="module")
def outputs(tmp_path_factory):
    import random_params
    d = tmp_path_factory.mktemp("epilogue")
    _, thresholds = random_params.make(str(d), "cnvW1A1", 41)
    for layer in (1, 2, 3):  # rows that never fire and rows that always do, in every layer compared here; thresholds within
        # 2.5 sigma of the popcount's mean meet their accumulator exactly in a few per cent of all compares
        assert (thresholds[layer] <= -32767).any() and (thresholds[layer] >= 32766).any(), layer
    child(_dump(d / "mfma.npz", str(d)), BNN_MI355X_CONV_MFMA_MIN=1)
    child(_dump(d / "valu.npz", str(d)), BNN_MI355X_CONV="valu")
    return dict(np.load(d / "mfma.npz")), dict(np.load(d / "valu.npz"))


@pytest.mark.parametrize("stage", sorted(COUNTS))
@pytest.mark.parametrize("pset", SETS)
def test_stage_equals_xnor_kernels(outputs, pset, stage):
    mfma, valu = outputs
    for n in COUNTS[stage]:
        a, b = mfma["%s_%d_%d" % (pset, stage, n)], valu["%s_%d_%d" % (pset, stage, n)]
        assert a.shape == b.shape and a.shape[0] == n
        bad = np.flatnonzero((a != b).any(axis=1))
        assert bad.size == 0, "stage %d, %d images, %s parameters: %d images differ, first %d" % (stage, n, pset, bad.size, bad[0])
