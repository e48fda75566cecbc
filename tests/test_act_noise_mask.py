"""Datapath upset-rate campaigns, host side (no GPU): bnn_mi355x_act_noise_mask -- the upset sites of one (run seed,
image, layer) -- is exactly what an independent numpy restatement of Philox4x32-10 (tests/act_noise_ref.py) draws, and
bnn_mi355x_act_noise_campaigns refuses bad arguments, the hardened variants and a machine without a GPU."""
import ctypes as C

import numpy as np
import pytest

import act_noise_ref as ref
import gpu_lib as gl

NETS = [("cnvW1A1", "cifar10"), ("cnvW1A2", "cifar10"), ("cnvW2A2", "cifar10"), ("lfcW1A1", "mnist"), ("lfcW1A2", "mnist")]
ip = C.POINTER(C.c_int)
RATES = [0, 1, 1 << 20, 1 << 24, 1 << 29, 1 << 31, 2 ** 32 - 1]
SEEDS = [1, 5, 0xDEADBEEF, 0x123456789ABCDEF0, 2 ** 64 - 1]


def lib_mask(L, seed, image, layer, rate, first=0, cap=None):
    total = L.bnn_mi355x_act_noise_mask(seed, image, layer, rate, 0, None, 0)
    assert total >= 0, L.bnn_mi355x_last_error()
    cap = total if cap is None else cap
    rec = np.full((max(cap, 1) + 1, 5), -7, np.int32)
    assert L.bnn_mi355x_act_noise_mask(seed, image, layer, rate, first, rec.ctypes.data_as(ip), cap) == total
    return total, rec


def test_philox_known_answers():
    """the restatement itself against the known-answer vectors of Random123 (kat_vectors: philox4x32 10) for the
    all-zero counter and key, the all-ones one and the digits of pi.  torch and rocRAND ship Philox code but not its
    test vectors, so the three lines are quoted from the published list."""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
           ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
           ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))]
    for ctr, key, want in kat:
        assert ref.philox4x32_10(ctr, key).tolist() == list(want)


@pytest.mark.parametrize("network,dataset", NETS, ids=lambda x: x)
def test_mask_equals_restatement(network, dataset):
    """records, order, shifts and total for every layer, several seeds, images and rates"""
    L = gl.load(network)
    rng = np.random.default_rng(9)
    for layer in range(len(ref.maps(network))):
        for k, seed in enumerate(SEEDS):
            for image in (0, 1, 4095 + 31 * k, int(rng.integers(1 << 31))):
                for rate in RATES if image < 2 else (RATES[(k + image) % len(RATES)], 1 << 27):
                    want = ref.mask(network, seed, image, layer, rate)
                    total, rec = lib_mask(L, seed, image, layer, rate)
                    assert total == len(want), (layer, seed, image, rate)
                    assert (rec[:total] == want).all(), (layer, seed, image, rate)
                    assert (rec[total:] == -7).all()
    h, w, c = ref.maps(network)[0]
    assert lib_mask(L, 3, 0, 0, 0)[0] == 0
    total, rec = lib_mask(L, 3, 0, 0, 2 ** 32 - 1)
    assert h * w * c - 2 <= total <= h * w * c  # (u = 2^32 - 1 is the only draw that rate misses)
    if ref.levels(network) == 3:
        assert set(rec[:total, 4].tolist()) == {1, 2}
    else:
        assert set(rec[:total, 4].tolist()) == {1}


def test_paging():
    L = gl.load("cnvW2A2")
    seed, image, layer, rate = 77, 12, 2, 1 << 28
    k, full = lib_mask(L, seed, image, layer, rate)
    assert k > 500
    for first, cap in ((0, 1), (7, 100), (k - 3, 10), (k - 1, 1), (k, 5), (k + 9, 5), (123, 0)):
        total, buf = lib_mask(L, seed, image, layer, rate, first, cap)
        got = max(0, min(cap, k - first))
        assert total == k and (buf[:got] == full[first:first + got]).all()
        assert (buf[got:] == -7).all(), (first, cap)  # nothing written past the window
    assert L.bnn_mi355x_act_noise_mask(seed, image, layer, rate, 5, None, 10) == k


@pytest.mark.parametrize("network,dataset", NETS, ids=lambda x: x)
def test_half_rate_count(network, dataset):
    """rate 2^31: the upsets of a whole layer lie within 5 standard deviations of sites / 2 (binomial, sigma =
    sqrt(sites) / 2) -- a property of the hash, for a seed list fixed beforehand"""
    L = gl.load(network)
    for layer, (h, w, c) in enumerate(ref.maps(network)):
        sites = h * w * c
        for seed in SEEDS:
            for image in (0, 3, 9999):
                total = L.bnn_mi355x_act_noise_mask(seed, image, layer, 1 << 31, 0, None, 0)
                assert abs(total - sites / 2) <= 5 * np.sqrt(sites) / 2, (layer, seed, image, total)


@pytest.mark.parametrize("network,last", [("cnvW1A1", 8), ("cnvW1A2", 8), ("cnvW2A2", 8), ("lfcW1A1", 3), ("lfcW1A2", 3)])
def test_mask_refusals(network, last):
    L = gl.load(network)
    for layer in (last, last + 1, -1, 100):
        assert L.bnn_mi355x_act_noise_mask(1, 0, layer, 1 << 20, 0, None, 0) == -1
        assert b"act_noise_mask" in L.bnn_mi355x_last_error()
    assert L.bnn_mi355x_act_noise_mask(1, 0, 0, 1 << 20, -1, None, 0) == -1
    assert L.bnn_mi355x_act_noise_mask(1, -1, 0, 1 << 20, 0, None, 0) == -1
    assert L.bnn_mi355x_act_noise_mask(1, 0, last - 1, 1 << 31, 0, None, 0) > 0


def rates_of(n, v=1 << 20):
    return (C.c_uint * n)(*([v] * n))


def test_campaign_refusals_without_a_gpu():
    """argument checks come before anything touches the device"""
    L = gl.load("cnvW1A1")
    cnt = C.c_int(0)
    r8 = rates_of(8)
    for runs, seed, rates, nr in ((0, 5, r8, 8), (-1, 5, r8, 8), (4097, 5, r8, 8), (7, 2 ** 64 - 3, r8, 8), (2, 2 ** 64 - 1, r8, 8),
                                  (2, 5, None, 8), (2, 5, r8, 7), (2, 5, rates_of(9), 9)):
        assert not L.bnn_mi355x_act_noise_campaigns(b"/nonexistent", 10, runs, seed, rates, nr, C.byref(cnt), None)
        assert b"act_noise_campaigns" in L.bnn_mi355x_last_error()
        assert L.bnn_mi355x_last_act_noise_counts(None, 0) == 0 and L.bnn_mi355x_last_act_noise_seeds(None, 0) == 0
    assert not L.bnn_mi355x_act_noise_campaigns(None, 10, 2, 5, r8, 8, C.byref(cnt), None)
    L3 = gl.load("lfcW1A2")
    assert not L3.bnn_mi355x_act_noise_campaigns(b"/nonexistent", 10, 2, 5, r8, 8, C.byref(cnt), None)
    assert b"n_rates" in L3.bnn_mi355x_last_error()


def test_variants_refused(variant_libs):
    """the hardened overlays: "not modelled", the one rule of every fault entry point"""
    for name, nr in (("cnvW1A1-TMR", 8), ("lfcW1A2-interleaved", 3)):
        L = gl.load(name)
        cnt = C.c_int(0)
        assert not L.bnn_mi355x_act_noise_campaigns(b"/nonexistent", 10, 3, 5, rates_of(nr), nr, C.byref(cnt), None)
        assert b"not modelled" in L.bnn_mi355x_last_error()


def test_no_gpu_fails_loudly():
    """without a HIP device the campaign refuses to compute (no CPU fallback), like every entry point"""
    try:
        import torch
        if torch.cuda.is_available():
            pytest.skip("GPU present")
    except ImportError:
        pass
    import os
    L = gl.load("lfcW1A1")
    L.load_parameters(gl.param_dir("mnist", "lfcW1A1").encode())
    assert L.bnn_mi355x_last_error() != b""
    cnt = C.c_int(0)
    path = os.path.join(gl.ROOT, "tests", "golden", "3.image-idx3-ubyte").encode()
    assert not L.bnn_mi355x_act_noise_campaigns(path, 10, 2, 5, rates_of(3), 3, C.byref(cnt), None)
    assert L.bnn_mi355x_last_error() != b""
    assert L.bnn_mi355x_last_act_noise_counts(None, 0) == 0
