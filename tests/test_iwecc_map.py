"""bnn_mi355x_iwecc_layout and bnn_mi355x_iwecc_site, host side (no GPU), against the model's text restated in
tests/iwecc_ref.py: the depth of every layer of all five nets is gcd(16, code words per PE); the site map is a bijection of
a layer's data sites onto (code word, 0 ... 63) and of its check bits onto (code word, 0 ... 7) -- whole for the small layers,
group-wise sampled for the large ones --; no group straddles a PE; adjacent columns lie in different code words; with
weight_interleave 0 the map is weight_code 1's identity membership."""
from math import gcd

import numpy as np
import pytest

import gpu_lib as gl
import hardened_ref as hr
import iwecc_ref as ir
import wecc_ref as wr

NETS = ["cnvW1A1", "cnvW1A2", "cnvW2A2", "lfcW1A1", "lfcW1A2"]
SMALL = [("cnvW1A1", 1), ("cnvW1A1", 8), ("cnvW2A2", 1), ("cnvW2A2", 8), ("lfcW1A1", 3)]


@pytest.mark.parametrize("network", NETS)
def test_depths(network):
    L = gl.load(network)
    lay = hr.params_io.layout(network)
    seen = set()
    for l in range(len(lay)):
        cwpp = wr.words_per_pe(network, 1, l)
        wl = (gl.C.c_int * 3)()
        assert L.bnn_mi355x_wecc_layout(1, l, wl) == 0
        got = ir.lib_layout(L, 1, 1, l)
        assert got[:3] == list(wl) and got[3] == (gcd(16, cwpp) if cwpp else 0) == ir.depth(network, 1, 1, l)
        assert ir.lib_layout(L, 1, 0, l) == list(wl) + [1 if cwpp else 0]
        assert ir.lib_layout(L, 0, 0, l) == [0, 0, 0, 0]
        if cwpp:
            assert cwpp % 2 == 0 and cwpp % got[3] == 0 and got[3] in (2, 8, 16)  # (every coded layer of the five nets: an even count)
            assert (lay[l]["pe"] * cwpp) % 64 == 0  # the kernels' whole waves: a coded layer's code words per run
            seen.add(got[3])
    if network == "cnvW1A1":
        assert [ir.lib_layout(L, 1, 1, l)[3] for l in (0, 1, 2)] == [0, 2, 8] and wr.words_per_pe(network, 1, 1) == 18
    if network == "cnvW2A2":
        assert ir.lib_layout(L, 1, 1, 1)[1:] == [72, 8, 8]
    if network == "lfcW1A1":
        assert ir.lib_layout(L, 1, 1, 0)[1:] == [416, 8, 16]
    print(network, sorted(seen))


def check_sites(L, network, layer, sites, module):
    """the library's map of the given sites equals the text's; -> {(word, bit)}"""
    D = ir.depth(network, 1, 1, layer)
    per = (64, 8)[module]
    cwpp = wr.words_per_pe(network, 1, layer)
    out = set()
    for s in sites:
        w, b = ir.lib_site(L, 1, 1, layer, module, int(s))
        assert (w, b) == ir.site_of(network, 1, layer, module, int(s)), (layer, module, s)
        assert 0 <= b < per and w // D == s // (per * D)  # inside its group ...
        assert w // cwpp == s // (per * cwpp)  # ... and so inside its PE
        assert ir.lib_site(L, 1, 0, layer, module, int(s)) == (s // per, s % per)  # weight_interleave 0: the identity membership
        out.add((w, b))
    return out


@pytest.mark.parametrize("network,layer", SMALL, ids=str)
def test_site_map_is_a_bijection_small_layers(network, layer):
    L = gl.load(network)
    words = hr.params_io.layout(network)[layer]["pe"] * wr.words_per_pe(network, 1, layer)
    D = ir.depth(network, 1, 1, layer)
    for module, per in ((0, 64), (1, 8)):
        got = check_sites(L, network, layer, range(words * per), module)
        assert got == {(w, b) for w in range(words) for b in range(per)}
    # columns adjacent in the memory lie in different code words, D apart at the earliest
    for s in range(0, 64 * D - 1):
        a, b = ir.lib_site(L, 1, 1, layer, 0, s), ir.lib_site(L, 1, 1, layer, 0, s + 1)
        assert a[0] != b[0]
    assert len({ir.lib_site(L, 1, 1, layer, 0, s)[0] for s in range(D)}) == D


@pytest.mark.parametrize("network", NETS)
def test_site_map_group_wise_large_layers(network):
    """first, last and a few seeded groups of every coded layer, each group whole: a bijection onto the group's D code words"""
    L = gl.load(network)
    rng = np.random.default_rng(7)
    for layer in wr.coded_layers(network, 1):
        if (network, layer) in SMALL:
            continue
        F = hr.params_io.layout(network)[layer]
        cwpp = wr.words_per_pe(network, 1, layer)
        D = ir.depth(network, 1, 1, layer)
        groups = F["pe"] * cwpp // D
        per_pe = cwpp // D
        picks = {0, groups - 1, per_pe - 1, per_pe % groups} | set(rng.integers(0, groups, 3).tolist())
        for G in picks:
            for module, per in ((0, 64), (1, 8)):
                got = check_sites(L, network, layer, range(G * per * D, (G + 1) * per * D), module)
                assert got == {(G * D + w, b) for w in range(D) for b in range(per)}
