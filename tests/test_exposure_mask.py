"""Exposure campaigns, host side (no GPU): bnn_mi355x_exposure_mask is the hardened draw with the epoch in the fourth
Philox counter word (csrc/mem_org.h).  Epoch 0 against bnn_mi355x_hardened_mem_noise_mask, later epochs against the
plain-Python restatement (tests/exposure_ref.py), paging and bad arguments like the hardened mask's; the ABI; and the
refusals of the device entry points, which come before anything touches a device."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import exposure_ref as xr
import gpu_lib as gl
import hardened_ref as hr

q32 = hr.q32
CNV = ["cnvW1A1", "cnvW1A2", "cnvW2A2"]
PAIRS = [(n, s) for n in CNV for s in (0,) + hr.SUPPORTED[n]] + [("lfcW1A1", 0), ("lfcW1A2", 0)]
NEW = ["bnn_mi355x_exposure_mask", "bnn_mi355x_exposure_campaigns", "bnn_mi355x_exposure_params", "bnn_mi355x_last_exposure_counts",
       "bnn_mi355x_last_exposure_seeds"]
CASES = ((1, q32(2.0 ** -7), 77), (4, q32(2.0 ** -5), (5 << 40) + 3))


def layers_of(network):
    nl = len(hr.params_io.layout(network))
    return list(range(min(nl, 5))) + [nl - 1]


@pytest.mark.parametrize("network,scheme", PAIRS, ids=str)
def test_epoch_0_is_the_hardened_mask(network, scheme):
    """every supported (network, scheme), bursts 1 and 4, every target and module: all fields but the image field (which
    holds the epoch: 0 here as well) equal hardened_mem_noise_mask's"""
    L = gl.load(network)
    seen = 0
    for layer in layers_of(network):
        for target in (0, 1):
            for m in range(hr.org(network, scheme, layer)[target]):
                for burst, rate, seed in CASES:
                    got = xr.lib_mask(L, scheme, burst, seed + layer, 0, layer, target, m, rate)
                    want = hr.lib_mask(L, scheme, burst, seed + layer, layer, target, m, rate)
                    assert got.shape == want.shape and (got[:, 1:] == want[:, 1:]).all() and (got[:, 0] == 0).all(), (layer, target, m, burst)
                    seen += len(got)
    assert seen > 100


@pytest.mark.parametrize("network,scheme", PAIRS, ids=str)
def test_later_epochs_equal_the_restatement(network, scheme):
    """epochs 1 ... 3 (and one near the cap): the library's records are the events whose Philox word -- epoch in the fourth
    counter word -- is below the rate, in event order, the image field holding the epoch; masks of different epochs differ"""
    L = gl.load(network)
    for layer in layers_of(network):
        for target in (0, 1):
            for m in range(hr.org(network, scheme, layer)[target]):
                for burst, rate, seed in CASES:
                    masks = []
                    for epoch in (1, 2, 3, xr.MAX_EPOCHS - 1):
                        got = xr.lib_mask(L, scheme, burst, seed, epoch, layer, target, m, rate)
                        want = xr.events(network, burst, seed, epoch, layer, target, m, rate)
                        assert got.shape == want.shape and (got == want).all(), (layer, target, m, burst, epoch)
                        assert (got[:, 0] == epoch).all()
                        masks.append(got[:, 1:].tolist())
                    masks.append(hr.events(network, burst, seed, layer, target, m, rate)[:, 1:].tolist())  # (epoch 0)
                    if min(len(x) for x in masks) > 20:
                        assert all(masks[i] != masks[j] for i in range(len(masks)) for j in range(i))
    # the restatement at epoch 0 is the hardened restatement
    assert (xr.events(network, 4, 9, 0, 1, 0, 0, q32(2.0 ** -4)) == hr.events(network, 4, 9, 1, 0, 0, q32(2.0 ** -4))).all()


def test_paging_and_bad_arguments():
    """`first` / `cap_records` page like hardened_mem_noise_mask; the same bad arguments give -1 + last_error, and so does
    an epoch outside 0 ... 65 535"""
    L = gl.load("cnvW1A1")
    rate = q32(2.0 ** -2)
    whole = xr.lib_mask(L, 1, 4, 5, 2, 1, 1, 2, rate)
    assert len(whole) > 30  # (several pages of 7)
    pages = [xr.lib_mask(L, 1, 4, 5, 2, 1, 1, 2, rate, first, 7) for first in range(0, len(whole) + 7, 7)]
    assert (np.concatenate(pages) == whole).all()
    assert len(xr.lib_mask(L, 1, 4, 5, 2, 1, 1, 2, rate, len(whole) + 3, 7)) == 0
    assert L.bnn_mi355x_exposure_mask(1, 4, 5, 2, 1, 1, 2, 0, 0, None, 0) == 0  # (rate 0)
    assert L.bnn_mi355x_exposure_mask(1, 4, 5, 2, 8, 1, 0, rate, 0, None, 0) == 0  # (layer 8 has no thresholds)
    good = dict(scheme=1, burst=1, seed=5, epoch=2, layer=1, target=1, module=0, rate=rate, first=0)
    assert L.bnn_mi355x_exposure_mask(*good.values(), None, 0) > 0
    for key, value in (("burst", 0), ("burst", 17), ("scheme", 5), ("scheme", -1), ("layer", 9), ("layer", -1), ("target", 2), ("module", 3),
                       ("first", -1), ("epoch", -1), ("epoch", xr.MAX_EPOCHS)):
        bad = dict(good)
        bad[key] = value
        assert L.bnn_mi355x_exposure_mask(*bad.values(), None, 0) == -1, (key, value)
        assert b"exposure_mask" in L.bnn_mi355x_last_error()
        if key != "epoch":  # the hardened mask refuses the same
            del bad["epoch"]
            assert L.bnn_mi355x_hardened_mem_noise_mask(*bad.values(), None, 0) == -1, (key, value)
    bad = dict(good, layer=1, target=0, module=1)  # (layer 1's weights have one module)
    assert L.bnn_mi355x_exposure_mask(*bad.values(), None, 0) == -1
    W = gl.load("cnvW2A2")
    assert W.bnn_mi355x_exposure_mask(2, 1, 5, 1, 0, 0, 0, rate, 0, None, 0) == -1 and b"cnvW2A2 with scheme 2" in W.bnn_mi355x_last_error()
    F = gl.load("lfcW1A1")
    assert F.bnn_mi355x_exposure_mask(1, 1, 5, 1, 0, 0, 0, rate, 0, None, 0) == -1 and b"LFC" in F.bnn_mi355x_last_error()


def exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
    return {line.split()[-1] for line in out.splitlines() if " T " in line}


def test_abi_declares_and_exports_the_new_symbols(variant_libs):
    """in the header's list (bnn/abi.py), declared with argument types, and exported by a base and by a variant build"""
    for s in NEW:
        assert s in gl.EXT
    for name in ("cnvW1A1", "lfcW1A2", "cnvW1A1-TMR", "lfcW1A2-interleaved"):
        for rt in ("python_sw", "python_hw"):
            assert set(NEW) <= exported(gl.lib_path(name, rt)), (name, rt)
        L = gl.load(name)
        assert L.bnn_mi355x_exposure_mask.restype is C.c_long and len(L.bnn_mi355x_exposure_campaigns.argtypes) == 13
        assert L.bnn_mi355x_exposure_params.restype is C.c_size_t and len(L.bnn_mi355x_exposure_params.argtypes) == 10
    # the scheme is the argument: a variant's library draws what the base network's draws
    a = xr.lib_mask(gl.load("cnvW1A1-TMR"), 3, 4, 9, 3, 1, 1, 0, q32(2.0 ** -3))
    assert len(a) > 20 and (a == xr.lib_mask(gl.load("cnvW1A1"), 3, 4, 9, 3, 1, 1, 0, q32(2.0 ** -3))).all()


def _campaign(L, scheme, burst, runs, seed, rw, rt, epoch_images, scrub_every, n_rates=None, path=b"/nonexistent"):
    up = C.c_uint * max(len(rw), 1)
    cnt = C.c_int(0)
    return L.bnn_mi355x_exposure_campaigns(path, 10, scheme, burst, runs, seed, up(*rw), up(*rt), len(rw) if n_rates is None else n_rates,
                                           epoch_images, scrub_every, C.byref(cnt), None)


def test_campaign_argument_checks_without_a_gpu(variant_libs):
    """bad arguments return NULL / 0 + last_error before any device is touched (the image file does not even exist, no
    parameters are loaded); a variant's library answers the same way"""
    z, w = [0] * 9, [1 << 20] * 9
    up = C.c_uint * 9
    for name in ("cnvW1A1", "cnvW1A1-TMR"):
        L = gl.load(name)
        for ei, every in ((0, 0), (-3, 1), (4, -1)):
            assert not _campaign(L, 1, 1, 2, 1, w, z, ei, every)
            assert b"epoch_images must be at least 1 and scrub_every must not be negative" in L.bnn_mi355x_last_error()
        for epoch, every in ((-1, 0), (xr.MAX_EPOCHS, 0), (2, -1)):
            assert L.bnn_mi355x_exposure_params(1, 1, 1, up(*w), up(*z), 9, epoch, every, None, 0) == 0
            assert b"exposure_params: epoch must be" in L.bnn_mi355x_last_error()
        for burst in (0, 17, -1):
            assert not _campaign(L, 1, burst, 2, 1, w, z, 4, 0)
            assert b"burst must be 1 ... 16" in L.bnn_mi355x_last_error()
            assert L.bnn_mi355x_exposure_params(1, burst, 1, up(*w), up(*z), 9, 1, 0, None, 0) == 0
            assert b"burst" in L.bnn_mi355x_last_error()
        for scheme in (-1, 4):
            assert not _campaign(L, scheme, 1, 2, 1, w, z, 4, 0)
            assert b"scheme must be" in L.bnn_mi355x_last_error()
        for n_rates in (8, 10, 0):
            assert not _campaign(L, 2, 4, 2, 1, w, z, 4, 0, n_rates=n_rates)
            assert b"n_rates" in L.bnn_mi355x_last_error()
        assert not _campaign(L, 3, 1, 2, 1, z, [0] * 8 + [5], 4, 0)
        assert b"layer 8 has no threshold memory" in L.bnn_mi355x_last_error()
        for runs in (0, 4097):
            assert not _campaign(L, 1, 1, runs, 1, w, z, 4, 0)
            assert b"num_runs" in L.bnn_mi355x_last_error()
        assert not _campaign(L, 1, 1, 2, 1, w, z, 4, 2)  # (nothing wrong with the arguments: no parameters are loaded)
        assert b"load_parameters" in L.bnn_mi355x_last_error()
        assert L.bnn_mi355x_exposure_params(1, 1, 1, up(*w), up(*z), 9, 3, 2, None, 0) == 0
        assert b"load_parameters" in L.bnn_mi355x_last_error()
        assert L.bnn_mi355x_last_exposure_counts(None, 0) == 0 and L.bnn_mi355x_last_exposure_seeds(None, 0) == 0
    L = gl.load("cnvW2A2")
    assert not _campaign(L, 2, 1, 2, 1, w, z, 4, 0)
    assert b"cnvW2A2 with scheme 2" in L.bnn_mi355x_last_error()
    L = gl.load("lfcW1A1")
    assert not _campaign(L, 1, 1, 2, 1, [1] * 4, [0] * 4, 4, 0)
    assert b"LFC" in L.bnn_mi355x_last_error()
