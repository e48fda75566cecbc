"""bnn_mi355x_pack_params_ecc, host side (no GPU), on the shipped cnvW1A1, cnvW2A2 (scheme 0 only) and lfcW1A1 parameter
sets: load the physical state (data and check memories), apply physical records in order, de-interleave, decode, pack.
Code 0 is pack_params_hardened; without records the blob is pack_params'; a single upset of a code word -- data bit or
check bit -- never shows; an aligned burst of 2 never shows under scheme 2 (the interleave turns it into single errors
of two code words) and is left as stored under scheme 0 (a detected double); whole seeded runs over epochs with a scrub
give the blob of the plain-Python route (tests/ecc_ref.py).  All comparisons are byte for byte.

A call of the single-record tests holds one record per coded layer (code words of different layers are independent), so
that every record is still the only error of its code word."""
import itertools

import numpy as np
import pytest

import ecc_ref as er
import gpu_lib as gl
import hardened_ref as hr

q32 = hr.q32
NETS = {"cnvW1A1": "cifar10", "cnvW2A2": "cifar10", "lfcW1A1": "mnist"}
CODED = [(n, s) for n in NETS for s in er.SUPPORTED[n]]


def pdir_of(network):
    return gl.param_dir(NETS[network], network)


def coded_layers(network):
    return [l for l in range(len(hr.params_io.layout(network))) if er.coded(network, 1, l)]


def elements(F):
    """8 elements (pe, line, threshold) of a threshold memory, the first and last PE and line among them"""
    edge = lambda n, k: list(dict.fromkeys(x for i in range(k) for x in (i, n - 1 - i) if 0 <= x < n))
    combos = sorted(itertools.product(enumerate(edge(F["tmem"], 4)), enumerate(edge(F["pe"], 2 if F["tmem"] >= 4 else 4))),
                    key=lambda c: c[0][0] + c[1][0])[:8]
    out = [(pe, line, j % F["nthr"]) for j, ((_, line), (_, pe)) in enumerate(combos)]
    assert len(set(out)) == 8 and {0, F["pe"] - 1} <= {e[0] for e in out} and {0, F["tmem"] - 1} <= {e[1] for e in out}
    return out


def rec9(layer, mem, ind, thresh, bit, ws, module):
    return [0, 1, layer, mem, ind, thresh, bit, ws, module]


@pytest.mark.parametrize("network", list(NETS))
def test_code_0_is_pack_params_hardened(network):
    """every scheme the network supports, records of every memory (bursts 1 and 4, two epochs): the same bytes"""
    L = gl.load(network)
    pdir = pdir_of(network)
    nl = len(hr.params_io.layout(network))
    for scheme in (0,) + hr.SUPPORTED.get(network, ()):
        rw, rt = [q32(2.0 ** -9)] * nl, [q32(2.0 ** -4) if hr.ebits(network, l, 1) else 0 for l in range(nl)]
        for burst in (1, 4):
            recs = np.concatenate([er.flat(er.lib_epoch_events(L, network, scheme, 0, burst, 31, t, rw, rt)) for t in (0, 1)])
            assert len(recs) > 100
            assert (er.lib_pack(L, pdir, scheme, 0, recs) == hr.pack_hardened(L, pdir, scheme, recs)).all(), (scheme, burst)
    # a check record needs the code
    l = coded_layers(network)[0]
    bad = np.array(rec9(l, 0, 0, 0, 0, 1, 1), np.int32)
    assert L.bnn_mi355x_pack_params_ecc(pdir.encode(), 0, 0, bad.ctypes.data_as(er.ip), 1, None, 0) == 0
    assert b"pack_params_ecc: fault record out of range" in L.bnn_mi355x_last_error()
    for field, value in ((6, 6), (6, -1), (3, 10 ** 6), (4, -1), (5, 2), (7, 0), (8, 2)):  # a check record outside the check memory
        bad = np.array(rec9(l, 0, 0, 0, 0, 1, 1), np.int32)
        bad[field] = value
        assert L.bnn_mi355x_pack_params_ecc(pdir.encode(), 0, 1, bad.ctypes.data_as(er.ip), 1, None, 0) == 0, (field, value)


@pytest.mark.parametrize("network,scheme", CODED, ids=str)
def test_single_upsets_never_show(network, scheme):
    """no records: pack_params' blob.  Every single data-bit and check-bit record (burst 1) of 8 elements of every coded
    layer: the fault-free blob -- where the same data record without the code changes it"""
    L = gl.load(network)
    pdir = pdir_of(network)
    clean = gl.pack_params(network, pdir)
    assert (er.lib_pack(L, pdir, scheme, 1, np.zeros((0, 9), np.int32)) == clean).all()
    lay = hr.params_io.layout(network)
    layers = coded_layers(network)
    assert layers == [l for l in range(len(lay)) if lay[l]["nthr"] and not (l == 0 and network.startswith("cnv"))]
    els = {l: elements(lay[l]) for l in layers}
    shown = 0
    for k in range(8):
        for module, width in ((0, 16), (1, 6)):
            for bit in range(width):
                recs = [rec9(l, *els[l][k], bit, 1, module) for l in layers]
                assert (er.lib_pack(L, pdir, scheme, 1, recs) == clean).all(), (k, module, bit)
                if module == 0 and bit in (0, 15):
                    shown += int((er.lib_pack(L, pdir, scheme, 0, recs) != clean).any())
    assert shown == 16  # (uncoded, every one of those calls changes the blob)


@pytest.mark.parametrize("network", list(NETS))
def test_aligned_bursts_of_2(network):
    """every aligned burst-2 data record of the same elements.  Scheme 2: the two bits belong to two code words, both are
    corrected: the fault-free blob.  Scheme 0: a double error of one code word, detected, the data as stored: the blob
    pack_params_hardened gives for the same records"""
    L = gl.load(network)
    pdir = pdir_of(network)
    clean = gl.pack_params(network, pdir)
    lay = hr.params_io.layout(network)
    layers = coded_layers(network)
    els = {l: elements(lay[l]) for l in layers}
    for k in range(8):
        for bit in range(0, 16, 2):
            recs = [rec9(l, *els[l][k], bit, 2, 0) for l in layers]
            if 2 in er.SUPPORTED[network]:
                assert (er.lib_pack(L, pdir, 2, 1, recs) == clean).all(), (k, bit)
            stored = hr.pack_hardened(L, pdir, 0, recs)
            assert (stored != clean).any() and (er.lib_pack(L, pdir, 0, 1, recs) == stored).all(), (k, bit)
    # a burst-2 CHECK record under scheme 2 is two single errors as well; under scheme 0 a detected double, the data untouched
    for bit in (0, 2, 4):
        recs = [rec9(l, *els[l][0], bit, 2, 1) for l in layers]
        for scheme in er.SUPPORTED[network]:
            assert (er.lib_pack(L, pdir, scheme, 1, recs) == clean).all()


@pytest.mark.parametrize("network,scheme", CODED, ids=str)
def test_seeded_runs_against_the_independent_route(network, scheme, tmp_path):
    """rates 2^-3 and 2^-8 per epoch on every threshold memory, bursts 1 and 4, 3 epochs, scrub_every 2: the blob of epoch 1 (epochs
    0 and 1 accumulated) and of epoch 2 (that epoch alone) equal the plain-Python route's; at 2^-3 its counts show every
    decode status in every coded layer, and data left wrong behind an accepted correction"""
    L = gl.load(network)
    pdir = pdir_of(network)
    nl = len(hr.params_io.layout(network))
    for p, burst in ((2.0 ** -3, 1), (2.0 ** -8, 4)):
        # (the weights, uncoded and through hardened_ref's route, at 2^-10 to keep its record loop short)
        rw, rt = [q32(2.0 ** -10)] * nl, [q32(p) if hr.ebits(network, l, 1) else 0 for l in range(nl)]
        per_epoch = [er.lib_epoch_events(L, network, scheme, 1, burst, 4242, t, rw, rt) for t in range(3)]
        for t in range(3):  # (the restatement of the draw, check memories included)
            for key, mine in er.epoch_events(network, scheme, 1, burst, 4242, t, rw, rt, lambda l, target: target == 1).items():
                assert mine.shape == per_epoch[t][key].shape and (mine == per_epoch[t][key]).all(), (t, key)
        for t in (1, 2):
            recs = er.since_scrub(per_epoch, t, 2)
            assert len(recs) == sum(len(er.flat(e)) for e in per_epoch[(0 if t == 1 else 2): t + 1])
            want, counts, detail = er.pack(network, scheme, 1, pdir, recs, str(tmp_path / ("p%d" % t)))
            assert (er.lib_pack(L, pdir, scheme, 1, recs) == want).all(), (p, burst, t)
            assert sum(counts[l, 2] for l in coded_layers(network)) > 0
            for l in coded_layers(network):
                if p == 2.0 ** -3:
                    assert counts[l, 2] > 0 and counts[l, 3] > 0 and counts[l, 4] > 0 and counts[l, 5] > 0, l
                    assert any(st == 1 and residual for st, residual, _, _ in detail[l]), l
