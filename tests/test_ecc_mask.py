"""Coded threshold memories, host side (no GPU): bnn_mi355x_ecc_exposure_mask with code 0 is bnn_mi355x_exposure_mask; with
code 1 module 1 of a coded layer's thresholds lists the check memory's events, which are the plain-Python restatement's
(tests/ecc_ref.py); bnn_mi355x_ecc_layout and bnn_mi355x_ecc_check_site; the ABI; and every refusal, which comes before
anything touches a device."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import ecc_ref as er
import exposure_ref as xr
import gpu_lib as gl
import hardened_ref as hr

q32 = hr.q32
ip = C.POINTER(C.c_int)
CNV = ["cnvW1A1", "cnvW1A2", "cnvW2A2"]
PAIRS = [(n, s) for n in CNV for s in (0,) + hr.SUPPORTED[n]] + [("lfcW1A1", 0), ("lfcW1A2", 0)]  # what the schemes support
CODED = [(n, s) for n, ss in er.SUPPORTED.items() for s in ss]
NEW = ["bnn_mi355x_ecc_encode", "bnn_mi355x_ecc_decode", "bnn_mi355x_ecc_layout", "bnn_mi355x_ecc_check_site", "bnn_mi355x_ecc_exposure_mask",
       "bnn_mi355x_pack_params_ecc", "bnn_mi355x_ecc_exposure_campaigns", "bnn_mi355x_ecc_exposure_params",
       "bnn_mi355x_last_ecc_exposure_counts", "bnn_mi355x_last_ecc_exposure_seeds"]


def layers_of(network):
    nl = len(hr.params_io.layout(network))
    return list(range(min(nl, 5))) + [nl - 1]


@pytest.mark.parametrize("network,scheme", PAIRS, ids=str)
def test_code_0_is_the_exposure_mask(network, scheme):
    """every supported (network, scheme), bursts 1 and 4, epochs 0 and 2, every target and module: the records and the
    layout are exposure_mask's and hardening_layout's"""
    L = gl.load(network)
    seen = 0
    for layer in layers_of(network):
        lay, old = (C.c_int * 4)(), (C.c_int * 3)()
        assert L.bnn_mi355x_ecc_layout(scheme, 0, layer, lay) == 0 and L.bnn_mi355x_hardening_layout(scheme, layer, old) == 0
        assert list(lay) == list(old) + [0]
        for target in (0, 1):
            for m in range(3):
                for burst, rate in ((1, q32(2.0 ** -7)), (4, q32(2.0 ** -5))):
                    for epoch in (0, 2):
                        if m >= lay[target]:
                            assert L.bnn_mi355x_ecc_exposure_mask(scheme, 0, burst, 77, epoch, layer, target, m, rate, 0, None, 0) == -1
                            assert L.bnn_mi355x_exposure_mask(scheme, burst, 77, epoch, layer, target, m, rate, 0, None, 0) == -1
                            continue
                        got = er.lib_mask(L, scheme, 0, burst, 77 + layer, epoch, layer, target, m, rate)
                        want = xr.lib_mask(L, scheme, burst, 77 + layer, epoch, layer, target, m, rate)
                        assert got.shape == want.shape and (got == want).all(), (layer, target, m, burst, epoch)
                        seen += len(got)
    assert seen > 100


@pytest.mark.parametrize("network,scheme", CODED, ids=str)
def test_check_events_equal_the_restatement(network, scheme):
    """code 1: module 0 of every memory is unchanged; module 1 of a coded layer's thresholds lists the check memory's
    events, equal to the restatement's for bursts 1, 2, 4 and 16, paged in sevens, with bit < 6 and word_size b; the
    check stream is not module 0's; an uncoded layer has no module 1"""
    L = gl.load(network)
    lay = hr.params_io.layout(network)
    seen = 0
    for layer in layers_of(network):
        out = (C.c_int * 4)()
        assert L.bnn_mi355x_ecc_layout(scheme, 1, layer, out) == 0
        assert tuple(out) == er.org(network, scheme, 1, layer)
        for burst in (1, 2, 4, 16):
            rate = q32(2.0 ** -4)
            for epoch in (0, 3):
                for target in (0, 1):  # the data memories draw as without the code
                    got = er.lib_mask(L, scheme, 1, burst, 5, epoch, layer, target, 0, rate)
                    assert (got == xr.lib_mask(L, scheme, burst, 5, epoch, layer, target, 0, rate)).all()
                if not er.coded(network, 1, layer):
                    assert out[3] == 0 and L.bnn_mi355x_ecc_exposure_mask(scheme, 1, burst, 5, epoch, layer, 1, 1, rate, 0, None, 0) == -1
                    continue
                assert out[1] == 2 and out[3] == 6
                want = er.check_events(network, burst, 5, epoch, layer, rate)
                got = er.lib_mask(L, scheme, 1, burst, 5, epoch, layer, 1, 1, rate)
                assert got.shape == want.shape and (got == want).all(), (layer, burst, epoch)
                pages = [er.lib_mask(L, scheme, 1, burst, 5, epoch, layer, 1, 1, rate, first, 7) for first in range(0, len(got) + 7, 7)]
                assert (np.concatenate(pages) == got).all()
                assert (got[:, 6] < 6).all() and (got[:, 6] % burst == 0).all() and (got[:, 7] == burst).all() and (got[:, 8] == 1).all()
                assert (got[:, 0] == epoch).all() and (got[:, 1] == 1).all() and (got[:, 2] == layer).all()
                F = lay[layer]
                assert (got[:, 3] < F["pe"]).all() and (got[:, 4] < F["tmem"]).all() and (got[:, 5] < F["nthr"]).all()
                seen += len(got)
                if burst == 1 and len(got) > 20:  # the same elements, another stream: not module 0's hits on bits 0 ... 5
                    data = er.lib_mask(L, scheme, 1, burst, 5, epoch, layer, 1, 0, rate)
                    low = data[data[:, 6] < 6]
                    assert low[:, 3:7].tolist() != got[:, 3:7].tolist()
                assert L.bnn_mi355x_ecc_exposure_mask(scheme, 1, burst, 5, epoch, layer, 1, 2, rate, 0, None, 0) == -1
                assert L.bnn_mi355x_ecc_exposure_mask(scheme, 1, burst, 5, epoch, layer, 0, 1, rate, 0, None, 0) == -1
    assert seen > 100


@pytest.mark.parametrize("network,scheme", CODED, ids=str)
def test_check_site(network, scheme):
    """logical -> physical for the check bits: the identity under scheme 0; under scheme 2 a bijection of each pair's 12
    positions, equal to the restatement's, an odd last line stored as is"""
    L = gl.load(network)
    lay = hr.params_io.layout(network)
    pairs = 0
    for layer in range(len(lay)):
        lines = lay[layer]["tmem"]
        pi, pb = C.c_int(-1), C.c_int(-1)
        if not er.coded(network, 1, layer):
            assert L.bnn_mi355x_ecc_check_site(scheme, 1, layer, 0, 0, C.byref(pi), C.byref(pb)) == -1
            assert b"no check memory" in L.bnn_mi355x_last_error()
            continue
        assert L.bnn_mi355x_ecc_check_site(scheme, 0, layer, 0, 0, C.byref(pi), C.byref(pb)) == -1  # (code 0: no check memory)
        for ind, bit in ((-1, 0), (lines, 0), (0, 6), (0, -1)):
            assert L.bnn_mi355x_ecc_check_site(scheme, 1, layer, ind, bit, C.byref(pi), C.byref(pb)) == -1
        some = sorted(set(range(min(lines, 4))) | set(range(max(lines - 3, 0), lines)))
        for a in sorted({ind & ~1 for ind in some}):
            image = []
            for ind in (a, a + 1):
                if ind >= lines:
                    continue
                for bit in range(6):
                    assert L.bnn_mi355x_ecc_check_site(scheme, 1, layer, ind, bit, C.byref(pi), C.byref(pb)) == 0
                    got = (pi.value, pb.value)
                    il = scheme if a + 1 < lines else 0
                    assert got == er.check_site(il, lines, ind, bit)
                    if il == 0:
                        assert got == (ind, bit)
                    image.append(got)
            if a + 1 < lines:
                assert sorted(image) == [(i, b) for i in (a, a + 1) for b in range(6)]
                pairs += 1
                if scheme == 2:  # both words of the pair hold bits of both elements
                    assert {i for i, _ in image[:6]} == {a, a + 1}
    assert pairs > 0 or all(lay[l]["tmem"] < 2 for l in range(len(lay)) if er.coded(network, 1, l))


def exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
    return {line.split()[-1] for line in out.splitlines() if " T " in line}


def test_abi_declares_and_exports_the_new_symbols(variant_libs):
    for s in NEW:
        assert s in gl.EXT
    for name in ("cnvW1A1", "lfcW1A2", "cnvW1A1-interleaved", "lfcW1A2-interleaved"):
        for rt in ("python_sw", "python_hw"):
            assert set(NEW) <= exported(gl.lib_path(name, rt)), (name, rt)
        L = gl.load(name)
        assert L.bnn_mi355x_ecc_exposure_mask.restype is C.c_long and len(L.bnn_mi355x_ecc_exposure_campaigns.argtypes) == 14
        assert L.bnn_mi355x_ecc_exposure_params.restype is C.c_size_t and len(L.bnn_mi355x_ecc_exposure_params.argtypes) == 11
        assert L.bnn_mi355x_pack_params_ecc.restype is C.c_size_t
    # the scheme and the code are arguments: a variant's library draws what the base network's draws
    a = er.lib_mask(gl.load("cnvW1A1-interleaved"), 2, 1, 4, 9, 3, 1, 1, 1, q32(0.5))
    assert len(a) > 20 and (a == er.lib_mask(gl.load("cnvW1A1"), 2, 1, 4, 9, 3, 1, 1, 1, q32(0.5))).all()


def _campaign(L, scheme, code, burst, runs, seed, rw, rt, epoch_images, scrub_every, n_rates=None, path=b"/nonexistent"):
    up = C.c_uint * max(len(rw), 1)
    cnt = C.c_int(0)
    return L.bnn_mi355x_ecc_exposure_campaigns(path, 10, scheme, code, burst, runs, seed, up(*rw), up(*rt), len(rw) if n_rates is None else n_rates,
                                               epoch_images, scrub_every, C.byref(cnt), None)


def refused_everywhere(L, scheme, code, reason, nl=9):
    """every entry point of the family refuses (scheme, code) with the reason: -1 / NULL / 0, nothing loaded, no device"""
    z, w = [0] * nl, [1 << 20] * nl
    up = C.c_uint * nl
    out = (C.c_int * 4)()
    rec = (C.c_int * 9)(0, 0, 1, 0, 0, 0, 0, 1, 0)
    calls = (lambda: L.bnn_mi355x_ecc_layout(scheme, code, 1, out) == -1,
             lambda: L.bnn_mi355x_ecc_check_site(scheme, code, 1, 0, 0, None, None) == -1,
             lambda: L.bnn_mi355x_ecc_exposure_mask(scheme, code, 1, 5, 0, 1, 1, 0, 1 << 20, 0, None, 0) == -1,
             lambda: L.bnn_mi355x_pack_params_ecc(b"/nonexistent", scheme, code, rec, 1, None, 0) == 0,
             lambda: not _campaign(L, scheme, code, 1, 2, 1, w, z, 4, 0),
             lambda: L.bnn_mi355x_ecc_exposure_params(scheme, code, 1, 1, up(*w), up(*z), nl, 1, 0, None, 0) == 0)
    for call in calls:
        assert call()
        assert reason in L.bnn_mi355x_last_error(), L.bnn_mi355x_last_error()


def test_refusals_without_a_gpu(variant_libs):
    """code 1 with scheme 1 or 3, everything the scheme alone refuses, code outside 0 ... 1: each with its reason, from
    every entry point; exposure_campaigns' own refusals reached through the new entry points with code 0 are unchanged;
    a variant's library answers the same way"""
    z, w = [0] * 9, [1 << 20] * 9
    up = C.c_uint * 9
    for name in ("cnvW1A1", "cnvW1A1-interleaved"):
        L = gl.load(name)
        refused_everywhere(L, 1, 1, b"code 1 with scheme 1 (TMR): TMR plus a code is not modelled")
        refused_everywhere(L, 3, 1, b"code 1 with scheme 3 (resilient-interleaved): the resilient patterns are defined for 32 and 48 positions only")
        for code in (-1, 2):
            for scheme in (0, 2):
                refused_everywhere(L, scheme, code, b"code must be 0 (none) or 1 (SEC-DED)")
        for scheme in (-1, 4, 5):
            for code in (0, 1):
                refused_everywhere(L, scheme, code, b"scheme must be")
        for code in (0, 1):
            for ei, every in ((0, 0), (-3, 1), (4, -1)):
                assert not _campaign(L, 2, code, 1, 2, 1, w, z, ei, every)
                assert b"ecc_exposure_campaigns: epoch_images must be at least 1 and scrub_every must not be negative" in L.bnn_mi355x_last_error()
            for epoch, every in ((-1, 0), (xr.MAX_EPOCHS, 0), (2, -1)):
                assert L.bnn_mi355x_ecc_exposure_params(2, code, 1, 1, up(*w), up(*z), 9, epoch, every, None, 0) == 0
                assert b"ecc_exposure_params: epoch must be" in L.bnn_mi355x_last_error()
            for burst in (0, 17, -1):
                assert not _campaign(L, 0, code, burst, 2, 1, w, z, 4, 0)
                assert b"burst must be 1 ... 16" in L.bnn_mi355x_last_error()
                assert L.bnn_mi355x_ecc_exposure_params(0, code, burst, 1, up(*w), up(*z), 9, 1, 0, None, 0) == 0
                assert b"burst" in L.bnn_mi355x_last_error()
                assert L.bnn_mi355x_ecc_exposure_mask(0, code, burst, 5, 0, 1, 1, 0, 1 << 20, 0, None, 0) == -1
            for n_rates in (8, 10, 0):
                assert not _campaign(L, 2, code, 4, 2, 1, w, z, 4, 0, n_rates=n_rates)
                assert b"n_rates" in L.bnn_mi355x_last_error()
            assert not _campaign(L, 2, code, 1, 2, 1, z, [0] * 8 + [5], 4, 0)
            assert b"layer 8 has no threshold memory" in L.bnn_mi355x_last_error()
            for runs in (0, 4097):
                assert not _campaign(L, 0, code, 1, runs, 1, w, z, 4, 0)
                assert b"num_runs" in L.bnn_mi355x_last_error()
            assert not _campaign(L, 2, code, 1, 2, 1, w, z, 4, 2)  # (nothing wrong with the arguments: no parameters are loaded)
            assert b"load_parameters" in L.bnn_mi355x_last_error()
            assert L.bnn_mi355x_ecc_exposure_params(2, code, 1, 1, up(*w), up(*z), 9, 3, 2, None, 0) == 0
            assert b"load_parameters" in L.bnn_mi355x_last_error()
            for key, args in (("layer", (0, code, 1, 5, 0, 9, 1, 0)), ("target", (0, code, 1, 5, 0, 1, 2, 0)), ("epoch", (0, code, 1, 5, -1, 1, 1, 0)),
                              ("epoch", (0, code, 1, 5, xr.MAX_EPOCHS, 1, 1, 0))):
                assert L.bnn_mi355x_ecc_exposure_mask(*args, 1 << 20, 0, None, 0) == -1, key
                assert b"ecc_exposure_mask" in L.bnn_mi355x_last_error()
            assert L.bnn_mi355x_ecc_exposure_mask(0, code, 1, 5, 0, 1, 1, 0, 1 << 20, -1, None, 0) == -1
        assert L.bnn_mi355x_last_ecc_exposure_counts(None, 0) == 0 and L.bnn_mi355x_last_ecc_exposure_seeds(None, 0) == 0
    W = gl.load("cnvW2A2")
    for code in (0, 1):
        refused_everywhere(W, 2, code, b"cnvW2A2 with scheme 2")
    refused_everywhere(W, 1, 1, b"TMR plus a code is not modelled")
    F = gl.load("lfcW1A1")
    for scheme in (1, 2, 3):
        for code in (0, 1):
            refused_everywhere(F, scheme, code, b"LFC", nl=4)
    out = (C.c_int * 4)()
    assert F.bnn_mi355x_ecc_layout(0, 1, 0, out) == 0 and list(out) == [1, 2, 0, 6]  # (the LFC nets' layer 0 holds 16-bit thresholds)
    C1 = gl.load("cnvW1A1")
    for layer, want in ((0, [1, 1, 2, 0]), (1, [1, 2, 2, 6]), (8, [1, 1, 0, 0])):  # (24-bit thresholds; coded; no thresholds)
        assert C1.bnn_mi355x_ecc_layout(2, 1, layer, out) == 0 and list(out) == want, layer
