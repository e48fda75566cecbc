"""Memory upset-rate campaigns, host side (no GPU): bnn_mi355x_mem_noise_mask -- the statement of which parameter bits a
run flips -- against a numpy restatement (tests/act_noise_ref.py's Philox4x32-10 with the counter {layer, target,
site >> 2, 1} over the records bnn_mi355x_enumerate_faults lists), its paging, edge rates and statistics, the way the
records go through bnn_mi355x_pack_params_faulty, and the refusals of the campaign's entry points, which come before
anything touches a device."""
import ctypes as C
import struct
import sys

import numpy as np
import pytest

import act_noise_ref as ref
import gpu_lib as gl

sys.path.insert(0, gl.ROOT + "/bnn-pynq_amd")
from bnn import params_io  # noqa: E402

NETS = [("cnvW1A1", "cifar10"), ("cnvW1A2", "cifar10"), ("cnvW2A2", "cifar10"), ("lfcW1A1", "mnist"), ("lfcW1A2", "mnist")]
ip = C.POINTER(C.c_int)
_sites = {}


def q32(p):
    return int(np.floor(p * 4294967296.0))


def sites_of(network, layer, target):
    """the site list: every word_size-1 record of the layer's memory, in the library's order (cached)"""
    key = (network, layer, target)
    if key not in _sites:
        L = gl.load(network)
        k = L.bnn_mi355x_enumerate_faults(layer, target, 1, 0, None, 0)
        assert k >= 0
        rec = np.zeros((max(k, 1), 8), np.int32)
        assert L.bnn_mi355x_enumerate_faults(layer, target, 1, 0, rec.ctypes.data_as(ip), k) == k
        _sites[key] = rec[:k]
    return _sites[key]


def draw(seed, layer, target, nsites, tag=1):
    """u of every site, in site order"""
    blocks = np.arange((nsites + 3) // 4)
    return ref.philox4x32_10((layer, target, blocks, tag), (seed & 0xFFFFFFFF, seed >> 32)).reshape(-1)[:nsites]


def ref_mask(network, seed, layer, target, rate):
    recs = sites_of(network, layer, target)
    u = draw(seed, layer, target, len(recs))
    return recs[u.astype(np.uint64) < np.uint64(rate)]


def lib_mask(L, seed, layer, target, rate, first=0, cap=None):
    total = L.bnn_mi355x_mem_noise_mask(seed, layer, target, rate, 0, None, 0)
    assert total >= 0, L.bnn_mi355x_last_error()
    cap = max(total - first, 0) if cap is None else cap
    rec = np.zeros((max(cap, 1), 8), np.int32)
    assert L.bnn_mi355x_mem_noise_mask(seed, layer, target, rate, first, rec.ctypes.data_as(ip), cap) == total
    return rec[:max(min(cap, total - first), 0)]


def all_masks(L, network, seed, rates_w, rates_t):
    """the records of a run: layer-major, per layer weights then thresholds, in site order"""
    out = [np.zeros((0, 8), np.int32)]
    for l in range(len(params_io.layout(network))):
        out.append(lib_mask(L, seed, l, 0, rates_w[l]))
        out.append(lib_mask(L, seed, l, 1, rates_t[l]))
    return np.concatenate(out)


def pack_faulty(L, pdir, recs):
    flat = np.ascontiguousarray(np.asarray(recs, np.int32).reshape(-1))
    fp = flat.ctypes.data_as(ip)
    size = L.bnn_mi355x_pack_params_faulty(pdir.encode(), fp, len(recs), None, 0)
    assert size > 0, L.bnn_mi355x_last_error()
    blob = np.zeros(size, np.uint8)
    assert L.bnn_mi355x_pack_params_faulty(pdir.encode(), fp, len(recs), blob.ctypes.data, size) == size
    return blob


def rows_named(network, recs):
    """apply_fault's row formula: weights (ind / (WMEM / TMEM)) * PE + mem, thresholds ind * PE + mem"""
    lay = params_io.layout(network)
    out = set()
    for _, target, layer, mem, ind, _, _, _ in np.asarray(recs).tolist():
        F = lay[layer]
        out.add((layer, (ind // (F["wmem"] // F["tmem"])) * F["pe"] + mem if target == 0 else ind * F["pe"] + mem))
    return out


@pytest.mark.parametrize("network,dataset", NETS, ids=lambda x: x)
def test_mask_equals_the_restatement(network, dataset):
    """every layer, both targets, rates 2^-6 and 2^-12: the library's records are the sites whose Philox word is below
    the rate, in site order"""
    L = gl.load(network)
    for layer, F in enumerate(params_io.layout(network)):
        for target in (0, 1):
            for rate, seed in ((q32(2.0 ** -6), 77 + layer), (q32(2.0 ** -12), (5 << 40) + 3)):
                got = lib_mask(L, seed, layer, target, rate)
                want = ref_mask(network, seed, layer, target, rate)
                assert got.shape == want.shape and (got == want).all(), (layer, target, rate)
                if target == 1 and F["nthr"] == 0:
                    assert len(got) == 0
                elif rate == q32(2.0 ** -6):
                    assert len(got) > 0


def test_pad_columns_are_sites():
    """lfcW1A1 layer 0: columns 784 ... 831 of a neuron's 832 lie inside the memory words' 64 SIMD bits"""
    recs = sites_of("lfcW1A1", 0, 0)
    assert len(recs) == 32 * 416 * 64 and recs[:, 6].max() == 63
    L = gl.load("lfcW1A1")
    hit = lib_mask(L, 9, 0, 0, q32(2.0 ** -4))
    col = (hit[:, 4] % 13) * 64 + hit[:, 6]  # (13 memory words of 64 columns per neuron)
    assert (col >= 784).any() and (col < 784).any()


@pytest.mark.parametrize("network,layer,target", [("cnvW1A1", 1, 0), ("cnvW2A2", 0, 1), ("lfcW1A2", 3, 1)])
def test_paging(network, layer, target):
    L = gl.load(network)
    rate, seed = q32(2.0 ** -5), 4711
    whole = lib_mask(L, seed, layer, target, rate)
    assert len(whole) > 20
    for cap in (1, 7, len(whole) // 2 + 1):
        pages = [lib_mask(L, seed, layer, target, rate, first, cap) for first in range(0, len(whole) + cap, cap)]
        assert (np.concatenate(pages) == whole).all() and len(pages[-1]) == 0
    assert len(lib_mask(L, seed, layer, target, rate, len(whole) + 5, 3)) == 0


@pytest.mark.parametrize("network,layer,target", [("cnvW1A1", 0, 0), ("cnvW1A2", 8, 0), ("lfcW1A1", 3, 1), ("cnvW2A2", 0, 1)])
def test_edge_rates(network, layer, target):
    """rate 0: nothing; rate 2^32 - 1: every site but those whose word is 0xffffffff"""
    L = gl.load(network)
    assert L.bnn_mi355x_mem_noise_mask(5, layer, target, 0, 0, None, 0) == 0
    recs = sites_of(network, layer, target)
    u = draw(5, layer, target, len(recs))
    got = lib_mask(L, 5, layer, target, 0xFFFFFFFF)
    assert (got == recs[u != 0xFFFFFFFF]).all() and len(recs) - len(got) <= 2


def test_statistics():
    """a fixed seed, lfcW1A1 layer 1 (1 048 576 weight sites) and cnvW2A2 layer 5 (1 179 648): the count lies within six
    binomial standard deviations of N p"""
    for network, layer in (("lfcW1A1", 1), ("cnvW2A2", 5)):
        L = gl.load(network)
        N = L.bnn_mi355x_enumerate_faults(layer, 0, 1, 0, None, 0)
        assert N >= 100000
        for p in (2.0 ** -6, 2.0 ** -12):
            k = L.bnn_mi355x_mem_noise_mask(20261018, layer, 0, q32(p), 0, None, 0)
            assert abs(k - N * p) < 6 * np.sqrt(N * p * (1 - p)), (network, p, k, N * p)


def test_stream_separation():
    """the block of (L, target, b) has 1 in the fourth counter word: it differs from the activation draw's block with
    the same first three words (image L, layer target, block b) -- in the restatement and in the two libraries' masks"""
    b = np.arange(4096)
    for layer, target in ((0, 0), (1, 0), (1, 1), (7, 1)):
        mem = ref.philox4x32_10((layer, target, b, 1), (123, 456))
        act = ref.philox4x32_10((layer, target, b, 0), (123, 456))
        assert (mem != act).any(axis=1).all()
    L = gl.load("cnvW1A1")
    seed, rate = 99, q32(2.0 ** -6)
    mem = lib_mask(L, seed, 1, 0, rate)  # layer 1's weights: 36 864 sites, counter {1, 0, s >> 2, 1}
    F = params_io.layout("cnvW1A1")[1]
    mem_sites = (mem[:, 3].astype(np.int64) * F["wmem"] + mem[:, 4]) * F["simd"] + mem[:, 6]
    k = L.bnn_mi355x_act_noise_mask(seed, 1, 0, rate, 0, None, 0)  # image 1, layer 0: counter {1, 0, s >> 2, 0}
    act = np.zeros((k, 5), np.int32)
    L.bnn_mi355x_act_noise_mask(seed, 1, 0, rate, 0, act.ctypes.data_as(ip), k)
    act_sites = (act[:, 1].astype(np.int64) * 30 + act[:, 2]) * 64 + act[:, 3]
    act_sites = act_sites[act_sites < 36864]
    assert len(mem_sites) > 300 and len(act_sites) > 300
    assert len(np.intersect1d(mem_sites, act_sites)) < 60  # (independent draws at 2^-6 share ~9 of 36 864 sites)


def test_mask_refusals():
    L = gl.load("cnvW1A1")
    for layer, target, first in ((-1, 0, 0), (9, 0, 0), (0, 2, 0), (0, -1, 0), (3, 1, -1)):
        assert L.bnn_mi355x_mem_noise_mask(1, layer, target, 1 << 20, first, None, 0) == -1
        assert b"mem_noise_mask" in L.bnn_mi355x_last_error()
    assert L.bnn_mi355x_mem_noise_mask(1, 8, 1, 0xFFFFFFFF, 0, None, 0) == 0  # (layer 8 has no thresholds)
    Lf = gl.load("lfcW1A1")
    assert Lf.bnn_mi355x_mem_noise_mask(1, 4, 0, 1, 0, None, 0) == -1
    assert Lf.bnn_mi355x_mem_noise_mask(1, 3, 1, 0xFFFFFFFF, 0, None, 0) > 0


@pytest.mark.parametrize("network,dataset", NETS, ids=lambda x: x)
def test_mask_and_packing_agree(network, dataset):
    """a run's records go through pack_params_faulty; the faulted blob differs from the clean one only inside the rows the
    records name by apply_fault's row formula (and layer 0's matrix-pipe tables) -- and in EVERY row a weight record or a
    record of a threshold stored injectively names (a flipped weight field always changes its value; T -> MW - T and
    T -> T are one to one, unlike the halving forms of CNV layer 0 and lfcW1A2 layer 0)"""
    L = gl.load(network)
    pdir = gl.param_dir(dataset, network)
    lay = params_io.layout(network)
    rw = [q32(2.0 ** -8)] * len(lay)
    rt = [q32(2.0 ** -5) if F["nthr"] else 0 for F in lay]
    recs = all_masks(L, network, 31, rw, rt)
    assert len(recs) > 1000
    blob, clean = pack_faulty(L, pdir, recs), gl.pack_params(network, pdir)
    named = rows_named(network, recs)
    inj = lambda r: r[1] == 0 or not ((network.startswith("cnv") and r[2] == 0) or (network == "lfcW1A2" and r[2] == 0))
    must = rows_named(network, [r for r in recs.tolist() if inj(r)])
    changed = set()
    for l in range(len(lay)):
        off, rd, rows, kw = struct.unpack_from("<4I", blob, 32 + 16 * l)
        a = blob[off: off + rows * rd * 4].reshape(rows, rd * 4)
        b = clean[off: off + rows * rd * 4].reshape(rows, rd * 4)
        changed |= {(l, int(n)) for n in np.nonzero((a != b).any(axis=1))[0]}
    assert changed <= named and must <= changed
    same = np.ones(len(blob), bool)
    l0m = struct.unpack_from("<I", blob, 24)[0]
    if l0m:
        same[l0m: l0m + 2 * 64 * 32 + 4096] = False
    for l, n in named:
        off, rd, rows, kw = struct.unpack_from("<4I", blob, 32 + 16 * l)
        same[off + n * rd * 4: off + (n + 1) * rd * 4] = False
    assert (blob[same] == clean[same]).all()


def _campaign(L, runs, seed, rw, rt, n_rates=None, path=b"/nonexistent"):
    up = C.c_uint * max(len(rw), 1)
    cnt = C.c_int(0)
    return L.bnn_mi355x_mem_noise_campaigns(path, 10, runs, seed, up(*rw) if rw is not None else None,
                                            up(*rt) if rt is not None else None, len(rw) if n_rates is None else n_rates,
                                            C.byref(cnt), None)


def test_campaign_argument_checks_without_a_gpu():
    """bad arguments return NULL + last_error before any device is touched (the image file does not even exist)"""
    L = gl.load("cnvW1A1")
    z = [0] * 9
    w = [1 << 20] * 9
    for runs in (0, -1, 4097):
        assert not _campaign(L, runs, 1, w, z)
        assert b"num_runs" in L.bnn_mi355x_last_error()
    assert not _campaign(L, 3, (1 << 64) - 2, w, z)
    assert b"wraps" in L.bnn_mi355x_last_error()
    for n_rates in (8, 10, 0):
        assert not _campaign(L, 2, 1, w, z, n_rates=n_rates)
        assert b"n_rates" in L.bnn_mi355x_last_error()
    up = C.c_uint * 9
    assert not L.bnn_mi355x_mem_noise_campaigns(b"/nonexistent", 10, 2, 1, None, up(*z), 9, None, None)
    assert b"bad arguments" in L.bnn_mi355x_last_error()
    assert not _campaign(L, 2, 1, z, [0] * 8 + [5])
    assert b"layer 8 has no threshold memory" in L.bnn_mi355x_last_error()
    buf = np.zeros(16, np.uint8)
    assert L.bnn_mi355x_mem_noise_params(1, up(*z), up(*([0] * 8 + [5])), 9, buf.ctypes.data, 16) == 0
    assert b"layer 8 has no threshold memory" in L.bnn_mi355x_last_error()
    assert L.bnn_mi355x_mem_noise_params(1, up(*z), up(*z), 4, None, 0) == 0
    assert b"n_rates" in L.bnn_mi355x_last_error()
    assert L.bnn_mi355x_last_mem_noise_counts(None, 0) == 0 and L.bnn_mi355x_last_mem_noise_seeds(None, 0) == 0


def test_variant_refused(variant_libs):
    """the hardened overlays' memory organisation is not modelled: refused like every fault entry point"""
    for network, nl in (("cnvW1A1-TMR", 9), ("lfcW1A2-interleaved", 4)):
        L = gl.load(network)
        up = C.c_uint * nl
        w, z = [1 << 20] * nl, [0] * nl
        assert not _campaign(L, 2, 1, w, z)
        assert b"not modelled" in L.bnn_mi355x_last_error()
        assert L.bnn_mi355x_mem_noise_params(1, up(*w), up(*z), nl, None, 0) == 0
        assert b"not modelled" in L.bnn_mi355x_last_error()
