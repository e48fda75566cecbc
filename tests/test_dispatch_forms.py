"""The restatement of the batch-size policy (dispatch_forms.py) kept honest: every constant it reads from the C++ source
is found, and the change points it derives are the ones the policy was written for.  test_gpu_forms.py runs the GPU at
these change points; if a threshold is retuned, the expected lists below are what to update, and the sweep follows."""
import pytest

import dispatch_forms as df

CNV_EDGES = [513, 1025, 5349, 8192, 14557, 20962, 29099, 32769, 58226, 130817]


def test_every_constant_is_found():
    want = {"kBlock", "kPixelLaneMax", "kCnvTailMax", "kNarrowLimitCnv", "kNarrowLimitLfc", "kFcLastWaveMax", "kLfcFusedMaxA2",
            "kForkMin", "kMaxChunk", "gpb_blocks", "l0_tile_min", "lfc_fused_max", "lfc_block_max", "lfc_fused_ipb"}
    assert want <= set(df.C)
    assert all(v for v in df.C.values())
    assert df.C["kMaxChunk"] == df.NMAX


def test_a_renamed_constant_fails_loudly():
    with pytest.raises(LookupError):
        df._find("constexpr long long kPixelLaneMaxImages = 512;", r"\bkPixelLaneMax\s*=\s*(\d+)", "kPixelLaneMax")


@pytest.mark.parametrize("net", ["cnvW1A1", "cnvW1A2", "cnvW2A2"])
def test_cnv_change_points(net):
    assert df.edges(lambda n: df.cnv_forms(n, net)) == CNV_EDGES
    if net == "cnvW2A2":  # -2-aware kernels: no one-launch tail, so nothing changes at 1 025
        assert df.edges(lambda n: df.cnv_forms(n, net, True)) == [e for e in CNV_EDGES if e != 1025]


def test_cnv_forms_of_the_table():
    f = df.cnv_forms
    assert f(1) == ("mfma", "pix", "pix", "pix", "tail", "tail", "tail", "tail", "tail")
    assert f(1, "cnvW2A2", True) == ("mfma", "pix", "pix", "pix", "n8", "n8", "n8", "n8", "wave")
    assert f(1025) == ("mfma",) + ("n8",) * 7 + ("wave",)
    assert f(20962)[1:5] == ("n32/2", "n32/4", "n32/4", "n8")
    assert f(29099)[4] == "n32/1" and f(32768)[8] == "wave" and f(32769)[8] == "fclast"
    assert f(58226)[4] == "n32/8" and f(130816)[6:8] == ("n8", "n8")
    assert f(131072, "cnvW2A2", True) == ("tile", "n32/2", "n32/4", "n32/4", "n32/8", "n8", "n32/1", "n32/1", "fclast")


def test_lfc_change_points():
    assert df.edges(lambda n: df.lfc_forms(n, "lfcW1A2")) == [257, 513, 1025, 2049, 3841, 65281]
    assert df.lfc_forms(65281, "lfcW1A2") == ("n32/1",) * 4 and df.lfc_forms(65280, "lfcW1A2")[3] == "n8"
    assert df.edges(lambda n: df.lfc_forms(n, "lfcW1A1")) == [257, 513, 1025]          # fused, then the block kernel to the end
    assert df.edges(lambda n: df.lfc_forms(n, "lfcW1A1", 0, 0)) == [3841, 65281]       # staged from the first image


def test_multi_change_points():
    assert df.edges(df.multi_forms) == [2674, 14557, 20962, 58226]
    assert df.multi_forms(1) == ("tile",) + ("n32/1",) * 7 + ("fclast",)
    assert df.multi_forms(131072) == ("tile", "n32/2", "n32/4", "n32/4", "n32/8", "n32/1", "n32/1", "n32/1", "fclast")


def test_a_forked_pass_puts_a_lane_on_each_edge():
    """m = 256 ceil(e / 256) + e images fork into lanes of 256 ceil(e / 256) and e.  The largest lane of a pass is 65 536
    images, so no forked lane reaches 130 817: that row runs unforked only (LANES=1, a captured graph)"""
    for e in CNV_EDGES:
        for x in (e - 1, e):
            h = 256 * -(-x // 256)
            if x < 8192 or h + x < df.C["kForkMin"]:
                continue                                   # (8 191: the pass does not fork)
            if h + x > df.C["kMaxChunk"]:
                assert x > df.C["kMaxChunk"] // 2
                continue
            assert df.fork_lanes(h + x) == (h, x), x
    assert df.fork_lanes(df.C["kForkMin"]) == (8192, 8192)
