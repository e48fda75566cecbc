"""GPU: the group and tile paths of the matrix forms of cnvW1A1 layers 1-3 (k_conv_mfma, DESIGN.md 5 "The matrix pipe")
that the small-batch tests never reach -- a block that takes a second group (the bits of the next group requested
during the current one, the expansion's unguarded and guarded rounds and the tile loop crossing a group boundary), a
ragged last group behind a full one, idle streams in the last round, and layer 3's padded plane rows with thresholds
that fire and ones that do not.  Stage 1-3 outputs against the XNOR-popcount kernels (BNN_MI355X_CONV=valu) on the same
seeded images, byte for byte.  The switches are read once per process: each configuration runs in a child process."""
import numpy as np
import pytest

import gpu_lib as gl
from test_gpu_conv_matrix import child

pytestmark = pytest.mark.gpu

# images -> stages: 1 and 3 images: 12.25 layer-1 tiles over the streams (idle streams in the last round), then a ragged
# second group; 1 027: 514 layer-1 groups of 2 on the 512-block grid, the last of them ragged; 4 099: 513 groups of 8 for
# layers 2 and 3, a block's first group full, its second with 3 images
SIZES = ((1, (1, 2, 3)), (3, (1, 2, 3)), (1027, (1,)), (4099, (2, 3)))


def dump(path, pdir, sizes):
    return (
        "load(%r)\n"
        "out = {}\n"
        "for n, stages in %r:\n"
        "    imgs = np.random.default_rng(40 + n).integers(0, 256, (n, 3072), dtype=np.uint8)\n"
        "    for s in stages:\n"
        "        out['n%%d_s%%d' %% (n, s)] = stage_output(L, imgs, s)\n"
        "np.savez(%r, **out)\n" % (pdir, sizes, str(path)))


def both(tmp_path, pdir, sizes):
    child(dump(tmp_path / "mfma.npz", pdir, sizes), BNN_MI355X_CONV_MFMA_MIN=1)
    child(dump(tmp_path / "valu.npz", pdir, sizes), BNN_MI355X_CONV="valu")
    a, b = np.load(tmp_path / "mfma.npz"), np.load(tmp_path / "valu.npz")
    assert sorted(a.files) == sorted(b.files) and len(a.files) == sum(len(s) for _, s in sizes)
    for k in a.files:
        assert a[k].shape == b[k].shape and (a[k] == b[k]).all(), k


def test_second_group_per_block_and_ragged_groups(tmp_path):
    """shipped parameters, every size of SIZES"""
    both(tmp_path, gl.param_dir("cifar10", "cnvW1A1"), SIZES)


def test_layer3_padded_rows_random_thresholds(tmp_path):
    """layer 3 (plane rows of 13 pixels for 12 columns) with a random parameter set -- never and always firing
    thresholds among them -- on 3 and 4 099 images"""
    import random_params
    (tmp_path / "p").mkdir()
    random_params.make(str(tmp_path / "p"), "cnvW1A1", 33)
    both(tmp_path, str(tmp_path / "p"), ((3, (3,)), (4099, (3,))))
