"""bnn_mi355x_wecc_exposure_mask and _wecc_layout, host side (no GPU): the weight check memory's records against the
plain-Python draw of tests/wecc_ref.py, record for record; the data memories' records are the uncoded campaign's; with
weight_code 0 the call is ecc_exposure_mask.  cnvW1A1, cnvW2A2 (2-bit fields), lfcW1A1 (layer 0 coded, kw = 13, 64-bit
elements) and lfcW1A2; bursts 1, 2 and 8."""
import ctypes as C

import numpy as np
import pytest

import ecc_ref as er
import gpu_lib as gl
import hardened_ref as hr
import wecc_ref as wr

q32 = hr.q32
NETWORKS = ["cnvW1A1", "cnvW2A2", "lfcW1A1", "lfcW1A2"]
ip = C.POINTER(C.c_int)


def layout_of(L, weight_code, layer):
    out = (C.c_int * 3)()
    assert L.bnn_mi355x_wecc_layout(weight_code, layer, out) == 0, L.bnn_mi355x_last_error()
    return list(out)


@pytest.mark.parametrize("network", NETWORKS)
def test_layout(network):
    L = gl.load(network)
    lay = hr.params_io.layout(network)
    for l, F in enumerate(lay):
        cwpp = wr.words_per_pe(network, 1, l)
        assert layout_of(L, 1, l) == ([1, cwpp, 8] if cwpp else [0, 0, 0])
        assert layout_of(L, 0, l) == [0, 0, 0]
        assert (cwpp == 0) == (network.startswith("cnv") and l == 0)
        if cwpp:  # a neuron's weights are whole code words: MW * wbits = 64 * kw * wbits sites
            assert 64 % hr.ebits(network, l, 0) == 0 and (F["wmem"] // F["tmem"] * hr.ebits(network, l, 0)) % 64 == 0
    if network == "lfcW1A1":
        assert hr.ebits(network, 0, 0) == 64 and lay[0]["wmem"] // lay[0]["tmem"] == 13
    for wc in (-1, 2):
        assert L.bnn_mi355x_wecc_layout(wc, 1, None) == -1 and b"wecc_layout: weight_code must be 0 (none) or 1" in L.bnn_mi355x_last_error()
    assert L.bnn_mi355x_wecc_layout(1, len(lay), None) == -1 and b"layer must be" in L.bnn_mi355x_last_error()


@pytest.mark.parametrize("burst", [1, 2, 8])
@pytest.mark.parametrize("network", NETWORKS)
def test_check_records_against_the_plain_python_draw(network, burst):
    """every coded layer, two epochs, 2^-5: module 1 of target 0 lists the check memory's events; module 0's records are
    exposure_mask's; paging with first / cap"""
    L = gl.load(network)
    seed, rate = (0xBEEF << 32) | 20261121, q32(2.0 ** -5)
    nl = len(hr.params_io.layout(network))
    seen = 0
    for l in range(nl):
        for epoch in (0, 3):
            if not wr.coded(network, 1, l):
                assert L.bnn_mi355x_wecc_exposure_mask(0, 0, 1, burst, seed, epoch, l, 0, 1, rate, 0, None, 0) == -1
                assert b"wecc_exposure_mask: bad burst" in L.bnn_mi355x_last_error()
                continue
            want = wr.check_events(network, burst, seed, epoch, l, rate)
            got = wr.lib_mask(L, 0, 0, 1, burst, seed, epoch, l, 0, 1, rate)
            assert got.shape == want.shape and (got == want).all(), (l, epoch)
            seen += len(want)
            cwpp = wr.words_per_pe(network, 1, l)
            assert (want[:, 4] < cwpp).all() and (want[:, 6] % burst == 0).all() and (want[:, 6] < 8).all() and (want[:, 5] == 0).all()
            if len(want) > 5:
                assert (wr.lib_mask(L, 0, 0, 1, burst, seed, epoch, l, 0, 1, rate, first=2, cap=3) == want[2:5]).all()
            data = wr.lib_mask(L, 0, 0, 1, burst, seed, epoch, l, 0, 0, rate)
            plain = er.lib_mask(L, 0, 0, burst, seed, epoch, l, 0, 0, rate)
            assert data.shape == plain.shape and (data == plain).all()
            # (the check draw is a stream of its own: module 1 in the counter word)
            assert L.bnn_mi355x_wecc_exposure_mask(0, 0, 1, burst, seed, epoch, l, 0, 2, rate, 0, None, 0) == -1
    assert seen > 100


@pytest.mark.parametrize("network,scheme,code", [("cnvW1A1", 0, 0), ("cnvW1A1", 1, 0), ("cnvW1A1", 2, 1), ("cnvW2A2", 1, 0), ("cnvW2A2", 0, 1),
                                                  ("lfcW1A1", 0, 1), ("lfcW1A2", 0, 0)], ids=str)
def test_weight_code_0_is_ecc_exposure_mask_and_the_epoch_order(network, scheme, code):
    """weight_code 0: every (layer, target, module) gives ecc_exposure_mask's records and refusals; weight_code 1 adds
    exactly module 1 of target 0 of the coded layers, everything else unchanged -- TMR included"""
    L = gl.load(network)
    seed, rate, burst, epoch = 99, q32(2.0 ** -6), 2, 1
    nl = len(hr.params_io.layout(network))
    rw, rt = [rate] * nl, [rate if hr.ebits(network, l, 1) else 0 for l in range(nl)]
    zero = wr.lib_epoch_events(L, network, scheme, code, 0, burst, seed, epoch, rw, rt)
    old = er.lib_epoch_events(L, network, scheme, code, burst, seed, epoch, rw, rt)
    assert list(zero) == list(old) and all((zero[k] == old[k]).all() for k in old)
    one = wr.lib_epoch_events(L, network, scheme, code, 1, burst, seed, epoch, rw, rt)
    extra = [k for k in one if k not in old]
    assert extra == [(l, 0, 1) for l in range(nl) if wr.coded(network, 1, l)] and all((one[k] == old[k]).all() for k in old)
    mine = wr.epoch_events(network, scheme, code, 1, burst, seed, epoch, rw, rt, lambda l, t: t == 1 or l == 0 or l == nl - 1)
    assert all((mine[k] == one[k]).all() and mine[k].shape == one[k].shape for k in mine)
    keys = list(one)
    for l in range(nl):
        if wr.coded(network, 1, l):  # data, check, then the thresholds
            assert keys.index((l, 0, 1)) == keys.index((l, 0, 0)) + 1
    for l in range(nl):
        for target in (0, 1):
            for module in (0, 1, 2, 3):
                a = L.bnn_mi355x_wecc_exposure_mask(scheme, code, 0, burst, seed, epoch, l, target, module, rate, 0, None, 0)
                b = L.bnn_mi355x_ecc_exposure_mask(scheme, code, burst, seed, epoch, l, target, module, rate, 0, None, 0)
                assert a == b


def test_refusals():
    L = gl.load("cnvW1A1")
    call = lambda scheme=0, code=0, wc=1, burst=1, epoch=0, layer=1, target=0, module=1, first=0: \
        L.bnn_mi355x_wecc_exposure_mask(scheme, code, wc, burst, 5, epoch, layer, target, module, 1 << 20, first, None, 0)
    assert call() >= 0
    for kw, reason in ((dict(wc=2), b"weight_code must be 0 (none) or 1"), (dict(wc=-1), b"weight_code must be"),
                       (dict(scheme=1, code=1), b"TMR plus a code is not modelled"), (dict(scheme=4), b"scheme must be"),
                       (dict(burst=17), b"bad burst"), (dict(epoch=1 << 16), b"bad burst"), (dict(layer=9), b"layer must be"),
                       (dict(layer=0), b"module (of those the memory has)"), (dict(wc=0), b"module (of those the memory has)"),
                       (dict(first=-1), b"or first")):
        assert call(**kw) == -1 and reason in L.bnn_mi355x_last_error() and b"wecc_exposure_mask: " in L.bnn_mi355x_last_error(), kw
