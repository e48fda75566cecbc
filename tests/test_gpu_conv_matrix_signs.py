"""GPU: the sign collection of cnvW1A1 layers 1-3 on the matrix pipe (k_conv_mfma, DESIGN.md 5 "The matrix pipe"): which
accumulator's sign ends on which output bit (sign_nibbles, the half swap -- one for both rows in layer 2 -- and the
operand table's row order), whatever form collects them.  Written with the packed collection by
v_cvt_scalef32_pk_fp4_f32 (built, measured and not kept, CHANGELOG), which permutes the rows and converts the
accumulators; kept for any later form.  Stage 1, 2 and 3 outputs byte for byte against the XNOR-popcount kernels
(BNN_MI355X_CONV=valu) at 1 and 3 images, with parameter sets made for the two ways this can go wrong:
  * one-hot: in every 32-neuron tile of layers 1-3 neuron j always fires and no other ever does, j = 0..31.  Every
    output word is then 1 << j; a wrong row permutation shows as the bit it moved to.
  * boundary: thresholds within 3 of the match count's mean next to rows that always / never fire.  The accumulator is
    2 (t - mismatches) - 1, an odd integer: -1 and +1 (count at the threshold, one off) are its smallest values, next
    to saturating ones.  A zero arises only in the vertical pool's AND of two rows' bit patterns: +0 from +1 & +3, -0
    from -1 & -3, subnormals from other pairs (layers 1 and 3).  With random +-1 weights the count is Binomial(mw, 1/2),
    sigma = 12 / 12 / 17: a row with its threshold within 3 of the mean meets it exactly in about 3 % of its compares,
    thousands of times per image.
The switches are read once per process: each kernel family runs in one child process, which rewrites the threshold
files of its own copy of the set between loads."""
import numpy as np
import pytest

from test_gpu_conv_matrix import child  # (its prelude gives the children stage_output, from test_gpu_layers)

pytestmark = pytest.mark.gpu

COUNTS = (1, 3)
STAGES = (1, 2, 3)


def _dump(path, pdir):
    return (
        "import threshold_params as tp\n"
        "pdir = %r\n"
        "imgs = {n: np.random.default_rng(600 + n).integers(0, 256, (n, 3072), dtype=np.uint8) for n in %r}\n"
        "out = {}\n"
        "def run(name):\n"
        "    load(pdir)\n"
        "    for stage in %r:\n"
        "        for n in %r:\n"
        "            out['%%s_%%d_%%d' %% (name, stage, n)] = stage_output(L, imgs[n], stage)\n"
        "for j in range(32):\n"
        "    tp.one_hot(pdir, j); run('hot%%d' %% j)\n"
        "tp.boundary(pdir, 5); run('boundary')\n"
        "np.savez(%r, **out)\n" % (str(pdir), COUNTS, STAGES, COUNTS, str(path)))


@pytest.fixture(scope="module")
def outputs(tmp_path_factory):
    import threshold_params
    d = tmp_path_factory.mktemp("signs")
    for fam in ("mfma", "valu"):
        threshold_params.make_base(str(d / fam), 51)
    child(_dump(d / "mfma.npz", d / "mfma"), BNN_MI355X_CONV_MFMA_MIN=1)
    child(_dump(d / "valu.npz", d / "valu"), BNN_MI355X_CONV="valu")
    return dict(np.load(d / "mfma.npz")), dict(np.load(d / "valu.npz"))


@pytest.mark.parametrize("stage", STAGES)
def test_one_hot_rows(outputs, stage):
    mfma, valu = outputs
    for j in range(32):
        for n in COUNTS:
            a, b = mfma["hot%d_%d_%d" % (j, stage, n)], valu["hot%d_%d_%d" % (j, stage, n)]
            assert a.shape == b.shape and a.shape[0] == n
            words = np.unique(np.ascontiguousarray(a).view("<u4"))
            assert words.tolist() == [1 << j], "stage %d, %d images, neuron %d of every tile fires: words %s" % (
                stage, n, j, [hex(w) for w in words[:8]])
            assert (a == b).all()


@pytest.mark.parametrize("stage", STAGES)
def test_boundary_thresholds(outputs, stage):
    mfma, valu = outputs
    for n in COUNTS:
        a, b = mfma["boundary_%d_%d" % (stage, n)], valu["boundary_%d_%d" % (stage, n)]
        assert a.shape == b.shape and a.shape[0] == n
        bits = np.unpackbits(a, bitorder="little")
        assert 0.1 < bits.mean() < 0.9, "the set does not exercise both outcomes"
        bad = np.flatnonzero((a != b).any(axis=1))
        assert bad.size == 0, "stage %d, %d images: %d images differ, first %d" % (stage, n, bad.size, bad[0])
