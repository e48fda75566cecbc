"""CPU: the saturated parameter sets of tests/saturated_params.py are what they claim to be.

The generator's closed form equals the faithful scalar restatement (Oracle.layer_ref, scores_ref / word_ref) on every
layer of all five nets in every configuration, whatever the image (CNV), and -- from the integer matrices alone, no
kernel involved -- every catalogue case occurs in every crafted layer, both outcomes of every decision occur there, and
the ends of the accumulator's range are reached in every layer.  tests/test_gpu_saturation.py relies on this: without it
the GPU comparison could pass on a set that saturates nothing."""
import hashlib
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import oracle_lib as ol
import random_params
import saturated_params as sp
from bnn import params_io

NETS = ("cnvW1A1", "cnvW1A2", "cnvW2A2", "lfcW1A1", "lfcW1A2")


def cnv_images():
    r = np.random.default_rng(3).integers(0, 256, (3, 3072), dtype=np.uint8)
    return np.concatenate([r, np.zeros((1, 3072), np.uint8), np.full((1, 3072), 255, np.uint8)])


@pytest.fixture(scope="module")
def sets(tmp_path_factory):
    """every configuration of every net, made once: {(network, config, neg2): (dir, weights, thresholds, expected)}"""
    out = {}
    for network in NETS:
        for config, neg2 in sp.variants(network):
            d = str(tmp_path_factory.mktemp("sat_%s" % network))
            out[(network, config, neg2)] = (d,) + sp.make(d, network, config, neg2)
    return out


@pytest.mark.parametrize("network", NETS)
def test_closed_form_equals_the_restatement(network, sets):
    """every layer's map and the scores / output word, on three random images, all-0 and all-255 (CNV) or the set's own
    four images (LFC)"""
    for (net, config, neg2), (d, _, _, E) in sets.items():
        if net != network:
            continue
        o = ol.Oracle(network, d)
        if o.is_cnv:
            def one(img):
                return [o.layer_ref(img, l) for l in range(8)], o.scores_ref(img)
            with ThreadPoolExecutor(5) as pool:
                for layers, scores in pool.map(one, cnv_images()):
                    for l in range(8):
                        assert layers[l].size == E["layers"][l].size and (layers[l] == E["layers"][l]).all(), (config, neg2, l)
                    assert scores.dtype == E["scores"].dtype and (scores == E["scores"]).all(), (config, neg2)
        else:
            for i, img in enumerate(E["images"]):
                for l in range(3):
                    assert (o.layer_ref(img, l) == E["layers"][l][i]).all(), (config, l, i)
                assert o.word_ref(img) == E["words"][i], (config, i)
            assert (o.words_fast(E["images"]) == np.array(E["words"], np.uint64)).all()


def layer_input(network, E, l, image=0):
    """the input vector of layer l's rows, from the expected map of layer l - 1"""
    if network.startswith("cnv"):
        ch = sp.CNV_SHAPE[l - 1][1]
        a = E["layers"][l - 1][:ch].astype(np.int64)
        return np.tile(a, 9) if l < 6 else a
    return sp.lfc_inputs(E["images"])[image] if l == 0 else E["layers"][l - 1][image].astype(np.int64)


@pytest.mark.parametrize("network", NETS)
def test_catalogue_coverage(network, sets):
    """from W, T and the input pattern: all weight and threshold cases in every crafted layer, both outcomes of every
    decision, and every layer's accumulators reach the ends of their range in some configuration"""
    lay = params_io.layout(network)
    cnv = network.startswith("cnv")
    first = 1 if cnv else 0
    reached = {l: set() for l in range(first, len(lay))}
    crafted_in = {l: 0 for l in range(first, len(lay))}
    for (net, config, neg2), (d, W, T, E) in sets.items():
        if net != network:
            continue
        for l in range(first, len(lay)):
            L, D = lay[l], E["design"][l]
            knd, mw, nthr = sp.kind(network, l), lay[l]["mw"], lay[l]["nthr"]
            image = np.full(L["mh"], sp.PRIMARY) if cnv or l else D["image"]
            # the accumulator of every row on the input it was written against, from the integer matrices
            acc = np.zeros(L["mh"], np.int64)
            for i in set(image.tolist()):
                a = layer_input(network, E, l, 0 if cnv else i)
                assert len(a) == mw
                acc[image == i] = sp.accumulate(knd, W[l][image == i], a)
            ref = D["acc"] if cnv or D["acc"].ndim == 1 else D["acc"][image, np.arange(L["mh"])]
            assert (acc == ref).all()
            reached[l] |= set(acc.tolist())
            if neg2:
                assert (W[l] == -2).any()
            else:
                assert (W[l] != -2).all()
            if not D["crafted"]:      # a saturated layer: one outcome only, by thresholds outside the reachable range
                out = sp.decide(acc, T[l], nthr)
                assert (out == out[0]).all() and out[0] != 0
                continue
            crafted_in[l] += 1
            assert set(D["weights"]) == set(sp.weight_cases(L["wbits"], neg2)), (config, l)
            if nthr == 0:
                continue
            rel, ab = sp.threshold_cases(knd, mw, nthr)
            assert set(D["thresholds"]) == {t[0] for t in rel + ab}, (config, l)
            t = np.asarray(T[l], np.int64)
            fire = t < acc[:, None]                                   # restated here, not taken from the generator
            for i in range(nthr):
                assert fire[:, i].any() and not fire[:, i].all(), (config, l, i)
            if nthr == 2:
                assert set((fire[:, 0].astype(int) + fire[:, 1]).tolist()) == {0, 1, 2}
                assert (t[:, 0] > t[:, 1]).any() and (t[:, 0] < t[:, 1]).any() and (t[:, 0] == t[:, 1]).any()
            # every weight case meets the threshold one below its accumulator (fires) and at it (does not)
            for case in set(D["weights"]):
                rows = np.array([w == case for w in D["weights"]])
                for i in range(nthr):
                    assert (rows & (t[:, i] == acc - 1) & fire[:, i]).any() and (rows & (t[:, i] == acc) & ~fire[:, i]).any(), (config, l, case)
            # the clamp neighbours and the int16 extremes are there as written (16-bit fields hold them all)
            for v in sp.absolute_thresholds(knd, mw):
                assert (t == v).any(), (config, l, v)
    for l in range(first, len(lay)):
        mw = lay[l]["mw"]
        assert crafted_in[l] >= 2, l
        if sp.kind(network, l) == "xnor":
            want = {0, 1, 2, mw // 2, mw - 2, mw - 1, mw}
        elif network == "cnvW2A2":
            want = {-2 * mw, 2 * mw, -mw, mw, 0}
        else:
            want = {-mw, mw, -mw + 2, mw - 2, 0}
        assert want <= reached[l], (network, l, sorted(want - reached[l]))
    if cnv:
        scores = set()
        for (net, config, neg2), (d, W, T, E) in sets.items():
            if net == network:
                scores |= set(E["scores"].tolist())
        assert ({0, 512} if network == "cnvW1A1" else {-512, 512}) <= scores
        if network == "cnvW2A2":
            assert {-1024, 1024} <= scores


def test_layer0_of_the_cnv_sets_mixes_the_levels(sets):
    for (network, config, neg2), (d, W, T, E) in sets.items():
        if network.startswith("cnv") and not config.startswith("sat_even"):
            want = {-1, 0, 1} if network.endswith("A2") else {-1, 1}
            assert set(E["layers"][0][:64].tolist()) == want
            if network.endswith("A2"):
                assert (E["layers"][0][:64] == 0).sum() == 21 and (T[0][:, 0] > T[0][:, 1]).any()
        elif network.startswith("cnv"):
            assert set(E["layers"][0].tolist()) == {1 if config.endswith("+") else -1}


@pytest.mark.parametrize("network", ("cnvW1A1", "cnvW1A2", "cnvW2A2"))
@pytest.mark.parametrize("layer", (1, 3))
def test_matched_filter_rows_reach_the_full_match(network, layer, tmp_path):
    """the matched-filter set: on its image, the four window rows of every pool position reach the full match, its
    mirror and one column off either, exactly at that position of the layer's input"""
    img = np.random.default_rng(40 + layer).integers(0, 256, 3072, dtype=np.uint8)
    W, T = sp.make_matched(str(tmp_path), network, 60 + layer, layer, img)
    o = ol.Oracle(network, str(tmp_path))
    py, px, width, ch = sp.MATCHED_CELL[layer]
    prev = o.layer_ref(img, layer - 1).astype(np.int64).reshape(width, width, ch)
    knd, mw = sp.kind(network, layer), params_io.layout(network)[layer]["mw"]
    rows = list(sp.MATCHED_ROWS)
    for k, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        a = prev[2 * py + dy:2 * py + dy + 3, 2 * px + dx:2 * px + dx + 3, :].reshape(-1)
        acc = sp.accumulate(knd, W[layer][rows[4 * k:4 * k + 4]], a)
        full = mw if knd == "xnor" else int(np.abs(a).sum())
        lo = 0 if knd == "xnor" else -full
        step = 1 if knd == "xnor" else 2
        assert acc[0] == full and acc[1] == lo and acc[2] == full - step and acc[3] == lo + step
        t = np.asarray(T[layer])[rows[4 * k:4 * k + 4]]
        assert t[0, 0] == full - 1 and t[1, 0] == lo


def test_random_params_is_unchanged():
    """the files random_params.make writes for seed 7, hashed before its dead condition was removed"""
    want = {"cnvW1A1": "d286675edf420b49142310017c2e5ce4cc2765fdd6344daf3a2b660846d1f24b",
            "cnvW1A2": "09e3d0e7f4f92a857bc3948c4bdb3801ded32f6c455bd4f1666727c66a2d1aa7",
            "cnvW2A2": "33cf5aa905d175f9f0c96f424586fb799c4fc289ff1bcd50ea2dfb1c5a347baa",
            "lfcW1A1": "1740111ebf4017de5744c169b15eb5de0fb4ee4267d90209fbd38bb5b4e15487",
            "lfcW1A2": "9048a7f7a1ebaf4768d3a45a54ef868b0312ea1b6460fee0c2de4494c8e347ce"}
    import tempfile
    for network in NETS:
        with tempfile.TemporaryDirectory() as d:
            random_params.make(d, network, 7, **({"neg2": 0.03} if network == "cnvW2A2" else {}))
            h = hashlib.sha256()
            for f in sorted(os.listdir(d)):
                h.update(f.encode())
                with open(os.path.join(d, f), "rb") as fp:
                    h.update(fp.read())
            assert h.hexdigest() == want[network], network
