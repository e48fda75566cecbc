"""The batch-size policy of csrc/kernels.hip and csrc/runtime.hip, restated in Python: which kernel form every stage of
one pass runs for a given number of images.  Test infrastructure only (the GPU sweep in test_gpu_forms.py takes its
sizes from edges()); the numeric constants are read from the C++ source, so a retuned threshold moves the sweep with it
and a renamed one fails test_dispatch_forms.py instead of leaving the sweep stale.

Form names: "n8" is the 8-neuron form of a thresholded stage, "n32/g" the 32-neuron form with g neuron groups per
block; "pix" the lane-per-output-pixel form of CNV layers 1-3; "tail" the one-launch k_cnv_tail(_a2) of CNV layers
4-8; "wave" / "fclast" CNV layer 8 as k_fclast_wave / k_fclast; "mfma" / "tile" CNV layer 0 as k_conv0_mfma /
k_conv0_tile; "fused/i" the one-launch LFC kernel with i images per block, "block" k_lfc_block_s."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bnn-pynq_amd", "csrc")
NMAX = 131072


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _find(src, pattern, what):
    m = re.search(pattern, src, re.S)
    if not m:
        raise LookupError("dispatch_forms: %s not found in the source (renamed or rewritten?)" % what)
    return m


def _constants():
    k, rt = _read("kernels.hip"), _read("runtime.hip")
    c = {}
    for name, src in (("kBlock", k), ("kLfcFusedMaxA2", k), ("kFcLastWaveMax", k), ("kPixelLaneMax", k), ("kCnvTailMax", k),
                      ("kNarrowLimitCnv", k), ("kNarrowLimitLfc", k), ("kMaxChunk", rt), ("kForkMin", rt)):
        c[name] = int(_find(src, r"\b%s\s*=\s*(\d+)" % name, name).group(1))
    for name, env in (("l0_tile_min", "L0_TILE_MIN"), ("lfc_fused_max", "LFC_FUSED_MAX"), ("lfc_block_max", "LFC_BLOCK_MAX")):
        body = _find(k, r"inline long long %s\(\) \{(.*?)\n\}" % name, name).group(1)
        _find(body, r'getenv\("BNN_MI355X_%s"\)' % env, name + "'s switch")
        c[name] = int(_find(body, r"return e \? std::atoll\(e\) : (\d+)LL;", name + "'s default").group(1))
    # gpb_for: all groups once the item blocks alone reach this many (256 CUs x 8 blocks)
    c["gpb_blocks"] = int(_find(k, r"inline int gpb_for\(long long items, int groups\) \{ return \(items \+ kBlock - 1\) / kBlock >= (\d+) \? groups : 1; \}",
                                "gpb_for").group(1))
    _find(k, r"inline bool narrow_for\(long long items, int groups32, long long limit\) \{ return \(\(items \+ kBlock - 1\) / kBlock\) \* groups32 < limit; \}",
          "narrow_for")
    m = _find(k, r"const int ipb = n <= (\d+) \? 1 : n <= (\d+) \? 2 : n <= (\d+) \? 4 : 8;", "the fused LFC kernel's images per block")
    c["lfc_fused_ipb"] = tuple(int(x) for x in m.groups())
    _find(rt, r"const int h = \(\(m / 2\) \+ 255\) & ~255;", "the fork's first-lane size")
    return c


C = _constants()


def gpb_for(items, groups):
    return groups if (items + C["kBlock"] - 1) // C["kBlock"] >= C["gpb_blocks"] else 1


def _stage(items, groups32, limit):
    """BNN_STAGE: the 8-neuron form while the 32-neuron grid is short of blocks, else 32 neurons, gpb_for groups per block"""
    if (items + C["kBlock"] - 1) // C["kBlock"] * groups32 < limit:
        return "n8"
    return "n32/%d" % gpb_for(items, groups32)


# CNV thresholded stages 1..7: (work items per image, groups of 32 neurons) -- run_cnv_t's BNN_STAGE calls
CNV_STAGES = ((196, 2), (36, 4), (25, 4), (9, 8), (1, 8), (1, 16), (1, 16))


def cnv_forms(n, net="cnvW1A1", two=False):
    """forms of CNV layers 0..8 for one pass of n images (run_cnv_t, default switches: MFMA layer 0, no stage events)"""
    assert net in ("cnvW1A1", "cnvW1A2", "cnvW2A2") and (not two or net == "cnvW2A2")
    lim = C["kNarrowLimitCnv"]
    f = ["tile" if n >= C["l0_tile_min"] else "mfma"]
    for ipi, g in CNV_STAGES[:3]:
        f.append("pix" if n <= C["kPixelLaneMax"] else _stage(n * ipi, g, lim))
    if not two and n <= C["kCnvTailMax"]:  # (the -2-aware kernels have no one-launch tail)
        return tuple(f + ["tail"] * 5)
    for ipi, g in CNV_STAGES[3:]:
        f.append(_stage(n * ipi, g, lim))
    f.append("wave" if n <= C["kFcLastWaveMax"] else "fclast")
    return tuple(f)


def lfc_forms(n, net, fused_max=None, block_max=None):
    """forms of one LFC pass of n images (run_lfc); fused_max / block_max: BNN_MI355X_LFC_FUSED_MAX / _BLOCK_MAX (lfcW1A1)"""
    assert net in ("lfcW1A1", "lfcW1A2")
    fused_max = C["lfc_fused_max"] if fused_max is None else fused_max
    block_max = C["lfc_block_max"] if block_max is None else block_max
    if n <= (fused_max if net == "lfcW1A1" else C["kLfcFusedMaxA2"]):
        a, b, c = C["lfc_fused_ipb"]
        return ("fused/%d" % (1 if n <= a else 2 if n <= b else 4 if n <= c else 8),)
    if net == "lfcW1A1" and n <= block_max:
        return ("block",)
    lim = C["kNarrowLimitLfc"]
    return tuple([_stage(n, 32, lim)] * 3 + [_stage(n, 2, lim)])


# multi-run launches (run_cnv_multi_t, BNN_MULTI): stages 1..7 always 32 neurons, groups per block from the launch total
def multi_forms(total, net="cnvW1A1"):
    assert net in ("cnvW1A1", "cnvW1A2", "cnvW2A2")
    return ("tile",) + tuple("n32/%d" % gpb_for(total * ipi, g) for ipi, g in CNV_STAGES) + ("fclast",)


def fork_lanes(m):
    """the two lane sizes of a device-pointer CNV pass that forks (m >= kForkMin images, at most kMaxChunk)"""
    assert C["kForkMin"] <= m <= C["kMaxChunk"]
    h = ((m // 2) + 255) & ~255
    return h, m - h


def edges(forms, nmax=NMAX):
    """every n in 2..nmax whose tuple of forms differs from n - 1's (forms: n -> tuple)"""
    out, prev = [], forms(1)
    for n in range(2, nmax + 1):
        cur = forms(n)
        if cur != prev:
            out.append(n)
        prev = cur
    return out
