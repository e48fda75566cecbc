"""Input-buffer faults, host side (no GPU): bnn_mi355x_enumerate_input_faults lists every bit of the image in site
order, bnn_mi355x_input_noise_mask -- the flipped sites of one (run seed, image) -- is the documented Philox4x32-10
draw (restated here in plain Python), and the entry points refuse bad arguments and the hardened variants before any
device work."""
import ctypes as C

import numpy as np
import pytest

import gpu_lib as gl

NETS = ["cnvW1A1", "cnvW1A2", "cnvW2A2", "lfcW1A1", "lfcW1A2"]
ip = C.POINTER(C.c_int)
M32 = 0xFFFFFFFF


def philox4x32_10(ctr, key):
    """Philox4x32-10 (Salmon et al., SC'11) on Python integers"""
    c0, c1, c2, c3 = ctr
    k0, k1 = key
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def draw(seed, image, site):
    """u of the header's definition for (run seed, image, site)"""
    return philox4x32_10((image, 0xFFFFFFFF, site >> 2, 0), (seed & M32, seed >> 32))[site & 3]


def test_philox_known_answers():
    """the restatement against the known-answer vectors of Random123 (kat_vectors, philox4x32 10)"""
    assert philox4x32_10((0, 0, 0, 0), (0, 0)) == (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)
    assert philox4x32_10((M32,) * 4, (M32,) * 2) == (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)
    assert philox4x32_10((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0)) == (
        0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)


def enumerate_sites(L, first=0, cap=None):
    total = L.bnn_mi355x_enumerate_input_faults(0, None, 0)
    cap = total if cap is None else cap
    rec = np.full((max(cap, 1) + 1, 2), -7, np.int32)
    assert L.bnn_mi355x_enumerate_input_faults(first, rec.ctypes.data_as(ip), cap) == total
    return total, rec


def lib_mask(L, seed, image, rate, first=0, cap=None):
    total = L.bnn_mi355x_input_noise_mask(seed, image, rate, 0, None, 0)
    assert total >= 0, L.bnn_mi355x_last_error()
    cap = total if cap is None else cap
    rec = np.full((max(cap, 1) + 1, 2), -7, np.int32)
    assert L.bnn_mi355x_input_noise_mask(seed, image, rate, first, rec.ctypes.data_as(ip), cap) == total
    return total, rec


@pytest.mark.parametrize("network", NETS)
def test_enumerate(network):
    """image_bytes * 8 records {byte, bit} in site order; paging reassembles the list; NULL returns the total"""
    L = gl.load(network)
    bits = L.bnn_mi355x_image_bytes() * 8
    assert bits == (24576 if network.startswith("cnv") else 6272)
    total, rec = enumerate_sites(L)
    assert total == bits
    s = np.arange(bits)
    assert (rec[:bits, 0] == s >> 3).all() and (rec[:bits, 1] == (s & 7)).all()
    assert (rec[bits:] == -7).all()
    assert L.bnn_mi355x_enumerate_input_faults(11, None, 100) == bits
    pages, first = [], 0
    while first < bits:
        cap = 1000 + 37 * len(pages)
        t, page = enumerate_sites(L, first, cap)
        got = min(cap, bits - first)
        assert t == bits and (page[got:] == -7).all()  # nothing written past the window
        pages.append(page[:got])
        first += got
    assert (np.concatenate(pages) == rec[:bits]).all()
    for first, cap in ((bits - 3, 10), (bits, 5), (bits + 9, 5), (123, 0)):
        t, page = enumerate_sites(L, first, cap)
        got = max(0, min(cap, bits - first))
        assert t == bits and (page[:got] == rec[first:first + got]).all() and (page[got:] == -7).all()
    assert L.bnn_mi355x_enumerate_input_faults(-1, None, 0) == -1
    assert b"enumerate_input_faults" in L.bnn_mi355x_last_error()


def test_mask_deterministic_paged_and_nested():
    L = gl.load("cnvW2A2")
    seed, image = 77, 12
    k, full = lib_mask(L, seed, image, 1 << 26)
    assert k > 200
    k2, again = lib_mask(L, seed, image, 1 << 26)
    assert k2 == k and (again == full).all()
    sites = full[:k, 0] * 8 + full[:k, 1]
    assert (np.diff(sites) > 0).all()  # site order
    for first, cap in ((0, 1), (7, 100), (k - 3, 10), (k - 1, 1), (k, 5), (k + 9, 5), (123, 0)):
        total, buf = lib_mask(L, seed, image, 1 << 26, first, cap)
        got = max(0, min(cap, k - first))
        assert total == k and (buf[:got] == full[first:first + got]).all()
        assert (buf[got:] == -7).all(), (first, cap)
    assert L.bnn_mi355x_input_noise_mask(seed, image, 1 << 26, 5, None, 10) == k
    assert lib_mask(L, seed, image, 0)[0] == 0
    # the sites at a rate are a subset of those at any higher rate
    prev = set()
    for rate in (1 << 20, 1 << 24, 1 << 26, 1 << 29, 2 ** 32 - 1):
        t, rec = lib_mask(L, seed, image, rate)
        now = set((rec[:t, 0] * 8 + rec[:t, 1]).tolist())
        assert prev <= now and len(now) == t
        prev = now
    assert 24576 - 2 <= len(prev) <= 24576  # (u = 2^32 - 1 is the only draw the highest rate misses)


def test_mask_differs_between_images_and_seeds():
    L = gl.load("lfcW1A1")
    a = lib_mask(L, 5, 0, 1 << 27)[1].tolist()
    assert a != lib_mask(L, 5, 1, 1 << 27)[1].tolist()
    assert a != lib_mask(L, 6, 0, 1 << 27)[1].tolist()
    assert a != lib_mask(L, 5 + (1 << 32), 0, 1 << 27)[1].tolist()  # (the key's high word counts)


def test_mask_count_is_binomial():
    """cnvW1A1, 64 images at 2^-6: the flips lie within 6 standard deviations of bits x rate"""
    L = gl.load("cnvW1A1")
    bits, p = 64 * 24576, 2.0 ** -6
    total = sum(L.bnn_mi355x_input_noise_mask(9, i, 1 << 26, 0, None, 0) for i in range(64))
    assert abs(total - bits * p) <= 6 * np.sqrt(bits * p * (1 - p)), total


@pytest.mark.parametrize("network", ["cnvW1A1", "lfcW1A2"])
def test_mask_equals_the_philox_definition(network):
    """a flagged site has u < rate by the definition restated in this file, its neighbours do not; and a whole mask
    recomputed site by site"""
    L = gl.load(network)
    bits = L.bnn_mi355x_image_bytes() * 8
    for seed, image, rate in ((3, 0, 1 << 24), (0xDEADBEEF12345678, 4099, 1 << 25), (2 ** 64 - 1, 2 ** 31 - 1, 1 << 24)):
        t, rec = lib_mask(L, seed, image, rate)
        assert t > 0
        flagged = set((rec[:t, 0] * 8 + rec[:t, 1]).tolist())
        for s in sorted(flagged)[:: max(1, t // 6)]:
            assert draw(seed, image, s) < rate, (seed, image, s)
            for nb in (s - 1, s + 1):
                if 0 <= nb < bits:
                    assert (draw(seed, image, nb) < rate) == (nb in flagged), (seed, image, nb)
    seed, image, rate = 41, 7, 1 << 27
    t, rec = lib_mask(L, seed, image, rate)
    want = [s for s in range(0, bits, 1) if s < 4096 and draw(seed, image, s) < rate]
    got = [s for s in (rec[:t, 0] * 8 + rec[:t, 1]).tolist() if s < 4096]
    assert got == want and len(want) > 50


def test_mask_refusals():
    L = gl.load("cnvW1A2")
    assert L.bnn_mi355x_input_noise_mask(1, -1, 1 << 20, 0, None, 0) == -1
    assert b"input_noise_mask" in L.bnn_mi355x_last_error()
    assert L.bnn_mi355x_input_noise_mask(1, 0, 1 << 20, -1, None, 0) == -1
    assert L.bnn_mi355x_input_noise_mask(1, 0, 1 << 31, 0, None, 0) > 0


def test_sweep_refusals_without_a_gpu():
    """records are validated on the host, before anything touches the device: the message names the record"""
    for network, nbytes in (("cnvW1A1", 3072), ("lfcW1A1", 784)):
        L = gl.load(network)
        ch = (C.c_int * 4)()
        for bad, where in (([0, 0, nbytes, 0], 1), ([-1, 3], 0), ([5, 8, 0, 0], 0), ([1, 1, 2, 2, 3, -1], 2)):
            rec = (C.c_int * len(bad))(*bad)
            assert L.bnn_mi355x_input_fault_sweep(b"/nonexistent", 10, rec, len(bad) // 2, ch, None, 0, None, None) == -1
            err = L.bnn_mi355x_last_error().decode()
            assert "input_fault_sweep: record %d {%d, %d}" % (where, bad[2 * where], bad[2 * where + 1]) in err, err
            assert L.bnn_mi355x_last_input_sweep_stages(None, 0) == 0
        ok = (C.c_int * 2)(0, 0)
        for args in ((None, 10, ok, 1, ch, None, 0), (b"/nonexistent", 10, None, 1, ch, None, 0), (b"/nonexistent", 10, ok, 1, None, None, 0),
                     (b"/nonexistent", 10, ok, -1, ch, None, 0), (b"/nonexistent", 10, ok, 1, ch, None, 5), (b"/nonexistent", 0, ok, 1, ch, None, 0)):
            assert L.bnn_mi355x_input_fault_sweep(*args, None, None) == -1
            assert b"input_fault_sweep: bad arguments" in L.bnn_mi355x_last_error()


def test_campaign_refusals_without_a_gpu():
    L = gl.load("cnvW1A1")
    cnt = C.c_int(0)
    for runs, seed in ((0, 5), (-1, 5), (4097, 5), (7, 2 ** 64 - 3), (2, 2 ** 64 - 1)):
        assert not L.bnn_mi355x_input_noise_campaigns(b"/nonexistent", 10, runs, seed, 1 << 20, C.byref(cnt), None)
        assert b"input_noise_campaigns" in L.bnn_mi355x_last_error()
        assert L.bnn_mi355x_last_input_noise_counts(None, 0) == 0 and L.bnn_mi355x_last_input_noise_seeds(None, 0) == 0
    assert b"wraps to 0" in L.bnn_mi355x_last_error()
    assert not L.bnn_mi355x_input_noise_campaigns(None, 10, 2, 5, 1 << 20, C.byref(cnt), None)
    assert not L.bnn_mi355x_input_noise_campaigns(b"/nonexistent", 65, 2, 5, 1 << 20, C.byref(cnt), None)
    assert b"input_noise_campaigns: bad arguments" in L.bnn_mi355x_last_error()


def test_variants_refused(variant_libs):
    """the hardened overlays: "not modelled", the one rule of every fault entry point"""
    for name in ("cnvW1A1-TMR", "lfcW1A2-interleaved"):
        L = gl.load(name)
        cnt = C.c_int(0)
        assert not L.bnn_mi355x_input_noise_campaigns(b"/nonexistent", 10, 3, 5, 1 << 20, C.byref(cnt), None)
        assert b"not modelled" in L.bnn_mi355x_last_error()
        rec, ch = (C.c_int * 2)(0, 0), (C.c_int * 1)()
        assert L.bnn_mi355x_input_fault_sweep(b"/nonexistent", 10, rec, 1, ch, None, 0, None, None) == -1
        assert b"not modelled" in L.bnn_mi355x_last_error()
        # the host-only helpers have nothing to model: they answer for the base network's image
        assert L.bnn_mi355x_enumerate_input_faults(0, None, 0) == L.bnn_mi355x_image_bytes() * 8


def test_no_gpu_fails_loudly():
    """without a HIP device the entry points refuse to compute (no CPU fallback), like every entry point"""
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
    assert not L.bnn_mi355x_input_noise_campaigns(path, 10, 2, 5, 1 << 20, C.byref(cnt), None)
    assert L.bnn_mi355x_last_error() != b""
    assert L.bnn_mi355x_last_input_noise_counts(None, 0) == 0
    rec, ch = (C.c_int * 2)(0, 7), (C.c_int * 1)()
    assert L.bnn_mi355x_input_fault_sweep(path, 10, rec, 1, ch, None, 0, None, None) == -1
