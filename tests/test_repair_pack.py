"""bnn_mi355x_pack_params_repair, host side (no GPU): pack_params_ecc with two marker records among the 9-int records
(layer -1: repair all memories now; layer -2: rewrite all memories from the loaded parameters now), against the
plain-Python route of tests/repair_ref.py for every supported (network, scheme, code).  Without markers it is
pack_params_ecc byte for byte; a -2 marker equals dropping every record before it; a -1 marker under a (scheme, code)
without redundancy is a no-op; a bad marker is refused by record number; and hand-made sequences whose outcome with and
without the marker differs.  All comparisons are byte for byte."""
import numpy as np
import pytest

import ecc_ref as er
import gpu_lib as gl
import hardened_ref as hr
import repair_ref as rr

q32 = hr.q32
DATASET = {"cnvW1A1": "cifar10", "cnvW1A2": "cifar10", "cnvW2A2": "cifar10", "lfcW1A1": "mnist", "lfcW1A2": "mnist"}
REPAIR, REWRITE = rr.marker(rr.REPAIR), rr.marker(rr.REWRITE)


def pdir_of(network):
    return gl.param_dir(DATASET[network], network)


def redundant(network, scheme, code):
    nl = len(hr.params_io.layout(network))
    return any(er.org(network, scheme, code, l)[0] == 3 or er.org(network, scheme, code, l)[1] > 1 for l in range(nl))


def rec(target, layer, mem, ind, thresh, bit, ws, module):
    return np.array([[0, target, layer, mem, ind, thresh, bit, ws, module]], np.int32)


def cat(*parts):
    return np.concatenate([np.zeros((0, 9), np.int32)] + [np.asarray(p, np.int32).reshape(-1, 9) for p in parts])


def seeded(L, network, scheme, code, burst, p, epochs=3):
    nl = len(hr.params_io.layout(network))
    # (the weights of layers >= 1 through hardened_ref's record loop: a low rate keeps it short)
    rw = [q32(p) if er.org(network, scheme, code, l)[0] == 3 else q32(2.0 ** -11) for l in range(nl)]
    rt = [q32(p) if hr.ebits(network, l, 1) else 0 for l in range(nl)]
    return [er.lib_epoch_events(L, network, scheme, code, burst, 777, t, rw, rt) for t in range(epochs)]


def test_supported_list():
    assert len(rr.SUPPORTED) == 5 + 3 + 3 + 2 + 7 and ("cnvW2A2", 2, 0) not in rr.SUPPORTED and ("cnvW1A1", 1, 1) not in rr.SUPPORTED


@pytest.mark.parametrize("network,scheme,code", rr.SUPPORTED, ids=str)
def test_against_the_independent_route(network, scheme, code, tmp_path):
    """three seeded epochs at 2^-3 (burst 1) and 2^-6 (burst 4) on the memories with redundancy: no marker is
    pack_params_ecc; a rewrite marker equals dropping what came before it; a repair marker before epochs 1 and 2, and a
    repair then a rewrite, give the plain-Python route's blob; without redundancy a repair marker changes nothing, with
    it (at 2^-3) it does"""
    L = gl.load(network)
    pdir = pdir_of(network)
    for p, burst in ((2.0 ** -3, 1), (2.0 ** -6, 4)):
        e = [er.flat(x) for x in seeded(L, network, scheme, code, burst, p)]
        what = (p, burst)
        plain = cat(*e)
        assert len(plain) > 50
        bare = er.lib_pack(L, pdir, scheme, code, plain)
        assert (rr.lib_pack(L, pdir, scheme, code, plain) == bare).all(), what
        assert (rr.lib_pack(L, pdir, scheme, code, cat(e[0], e[1], REWRITE, e[2])) == er.lib_pack(L, pdir, scheme, code, e[2])).all(), what
        assert (rr.lib_pack(L, pdir, scheme, code, cat(e[0], REPAIR, REWRITE)) == gl.pack_params(network, pdir)).all(), what
        repaired = cat(e[0], REPAIR, e[1], REPAIR, e[2])
        got = rr.lib_pack(L, pdir, scheme, code, repaired)
        if not redundant(network, scheme, code):
            assert (got == bare).all(), what
            continue
        assert (got == rr.pack(network, scheme, code, pdir, repaired, str(tmp_path / "a"))).all(), what
        mixed = cat(e[0], REPAIR, e[1], REWRITE, e[2], REPAIR, e[1], REPAIR)
        assert (rr.lib_pack(L, pdir, scheme, code, mixed) == rr.pack(network, scheme, code, pdir, mixed, str(tmp_path / "b"))).all(), what
        # a trailing repair never changes the delivered parameters
        assert (rr.lib_pack(L, pdir, scheme, code, cat(repaired, REPAIR)) == got).all(), what
        if p == 2.0 ** -3:
            assert (got != bare).any(), what
            assert (rr.pack(network, scheme, code, pdir, plain, str(tmp_path / "c")) == bare).all(), what


@pytest.mark.parametrize("network,scheme,code", [("cnvW1A1", 2, 1), ("lfcW1A1", 0, 1), ("cnvW1A2", 1, 0)], ids=str)
def test_bad_markers_are_refused_by_record_number(network, scheme, code):
    L = gl.load(network)
    pdir = pdir_of(network)
    ok = rec(0, 1, 0, 0, 0, 0, 1, 0)
    for bad in (-3, -100, -(1 << 31)):
        m = rr.marker(rr.REPAIR)
        m[0, 2] = bad
        rr.lib_pack(L, pdir, scheme, code, cat(ok, REPAIR, m, ok), expect_error=b"pack_params_repair: record 2: layer %d is no marker" % bad)
    rr.lib_pack(L, pdir, scheme, code, cat(ok, REWRITE, rec(0, 99, 0, 0, 0, 0, 1, 0)), expect_error=b"pack_params_repair: record 2: fault record out of range")
    rr.lib_pack(L, pdir, 1, 1, ok, expect_error=b"TMR plus a code is not modelled" if network.startswith("cnv") else b"LFC networks")
    # (the other eight ints of a marker are not read)
    m = np.full((1, 9), 12345, np.int32)
    m[0, 2] = rr.REPAIR
    assert (rr.lib_pack(L, pdir, scheme, code, cat(ok, m)) == rr.lib_pack(L, pdir, scheme, code, ok)).all()


def test_tmr_sequences():
    """layers 0 (weights, 24-bit thresholds) and 2 (16-bit thresholds) of cnvW1A1 under scheme 1"""
    network, scheme = "cnvW1A1", 1
    L = gl.load(network)
    pdir = pdir_of(network)
    clean = gl.pack_params(network, pdir)
    pack = lambda *parts: rr.lib_pack(L, pdir, scheme, 0, cat(*parts))
    assert hr.ebits(network, 0, 0) == 3 and hr.ebits(network, 0, 1) == 24 and hr.ebits(network, 2, 1) == 16
    for target, layer, bit in ((0, 0, 0), (0, 0, 2), (1, 2, 3), (1, 2, 15), (1, 0, 9), (1, 0, 15)):
        hit = lambda module: rec(target, layer, 1, 1, 0, bit, 1, module)
        flipped = pack(hit(0), hit(1))
        assert (flipped != clean).any() and (pack(hit(0)) == clean).all()
        # one module hit, repair, a second module hit on the same bit: clean; without the repair the bit is flipped
        assert (pack(hit(0), REPAIR, hit(1)) == clean).all(), (target, layer, bit)
        assert (pack(hit(2), REPAIR, hit(0), REPAIR, hit(1)) == clean).all()
        # two modules hit on one bit, repair, then any single later hit on that bit: still flipped (locked in)
        for later in range(3):
            assert (pack(hit(0), hit(1), REPAIR, hit(later)) == flipped).all(), (target, layer, bit, later)
        # ... until two modules are hit again, or the memories are rewritten
        assert (pack(hit(0), hit(1), REPAIR, hit(0), REPAIR, hit(1)) == flipped).all()
        assert (pack(hit(0), hit(1), REPAIR, REWRITE) == clean).all()
        if (target, layer) != (1, 0):  # (a pure XOR; an event of layer 0's 24-bit thresholds rewrites the word as its integer part)
            assert (pack(hit(0), hit(1), hit(0)) == clean).all() and (pack(hit(0), hit(1), REPAIR, hit(0), hit(1)) == clean).all()
            assert (pack(hit(0), hit(1), REPAIR, hit(0), hit(2)) == clean).all()
    # a single-module threshold memory (layer 6) is not repaired: two hits of a bit cancel with or without the marker
    one = rec(1, 6, 0, 0, 0, 4, 1, 0)
    assert (pack(one) != clean).any() and (pack(one, REPAIR) == pack(one)).all() and (pack(one, REPAIR, one) == clean).all()
    # nor are the weights of a layer >= 1
    w = rec(0, 3, 0, 0, 0, 1, 1, 0)
    assert (pack(w, REPAIR) == pack(w)).all() and (pack(w) != clean).any() and (pack(w, REPAIR, w) == clean).all()


@pytest.mark.parametrize("network,scheme", [("cnvW1A1", 0), ("cnvW1A1", 2), ("lfcW1A1", 0)], ids=str)
def test_coded_sequences(network, scheme):
    L = gl.load(network)
    pdir = pdir_of(network)
    clean = gl.pack_params(network, pdir)
    pack = lambda *parts: rr.lib_pack(L, pdir, scheme, 1, cat(*parts))
    layer = 2 if network.startswith("cnv") else 1
    F = hr.params_io.layout(network)[layer]
    assert F["tmem"] >= 4

    def hit(logical_bit, ind=2, pe=1):
        """a burst-1 record of the physical bit that holds logical bit 0 ... 15 (data) or 16 ... 21 (check) of line ind's word"""
        if logical_bit < 16:
            p_ind, p_bit = hr.site(scheme, 16, F["tmem"], ind, logical_bit)
            return rec(1, layer, pe, p_ind, 0, p_bit, 1, 0)
        p_ind, p_bit = er.check_site(scheme, F["tmem"], ind, logical_bit - 16)
        return rec(1, layer, pe, p_ind, 0, p_bit, 1, 1)

    for a, b in ((3, 9), (0, 17), (20, 21), (15, 16)):
        double = pack(hit(a), hit(b))
        assert (pack(hit(a)) == clean).all() and (pack(hit(b)) == clean).all()
        if a < 16 or b < 16:
            assert (double != clean).any()  # detected, the data as stored
        # single, repair, single: clean; without the repair it is a double
        assert (pack(hit(a), REPAIR, hit(b)) == clean).all(), (a, b)
        # a double is left as stored by the repair: a third hit makes it a triple, taking one back a single
        assert (pack(hit(a), hit(b), REPAIR) == double).all()
        assert (pack(hit(a), hit(b), REPAIR, hit(a)) == clean).all()
    # an accepted triple, repair: status 0 with wrong data from then on
    triple = next(t for t in ((0, 1, 2), (0, 1, 3), (0, 2, 5), (1, 2, 4), (0, 1, 16), (3, 4, 5), (0, 4, 7)) if rr.repair_word(*er_stored(t))[0] == 1)
    st, nd, nc = rr.repair_word(*er_stored(triple))
    fourth = [k for k in range(22) if ((nd | nc << 16) >> k) & 1 and k not in triple]
    assert st == 1 and nd != 0 and len(fourth) == 1  # (in error-pattern terms: the nearest code word, of weight 4)
    wrong = pack(hit(triple[0]), hit(triple[1]), hit(triple[2]))
    assert (wrong != clean).any()
    locked = pack(hit(triple[0]), hit(triple[1]), hit(triple[2]), REPAIR)
    assert (locked == wrong).all()
    # before the repair, taking one of the three hits back leaves a double whose data error is the other two's; after it, the
    # same hit meets a valid wrong word and is corrected back to it
    undone = [k for k in triple if k < 16][0]
    assert (pack(hit(triple[0]), hit(triple[1]), hit(triple[2]), REPAIR, hit(undone)) == wrong).all()
    assert (pack(hit(triple[0]), hit(triple[1]), hit(triple[2]), hit(undone)) != wrong).any()
    assert (pack(hit(triple[0]), hit(triple[1]), hit(triple[2]), REPAIR, hit(undone), REPAIR, hit(fourth[0])) == wrong).all()
    assert (pack(hit(triple[0]), hit(triple[1]), hit(triple[2]), REPAIR, REWRITE) == clean).all()
    # the 24-bit thresholds of CNV layer 0 are not coded and not repaired
    if network.startswith("cnv"):
        one = rec(1, 0, 0, 0, 0, 12, 1, 0)
        assert (pack(one) != clean).any() and (pack(one, REPAIR) == pack(one)).all()


def er_stored(positions):
    m = sum(1 << p for p in positions)
    return m & 0xFFFF, m >> 16


def test_scheme_2_pair_only_one_elements_bits_change():
    """lines 2 and 3 of one PE share two physical lines.  Line 2's word holds a single error, line 3's a double: a repair
    rewrites line 2's bits alone -- a later hit of line 2's word is again a single, and line 3's double is still there"""
    network, scheme = "cnvW1A1", 2
    L = gl.load(network)
    pdir = pdir_of(network)
    clean = gl.pack_params(network, pdir)
    layer = 2
    F = hr.params_io.layout(network)[layer]
    pack = lambda *parts: rr.lib_pack(L, pdir, scheme, 1, cat(*parts))

    def hit(ind, bit):
        p_ind, p_bit = hr.site(scheme, 16, F["tmem"], ind, bit)
        assert {p_ind} <= {2, 3}
        return rec(1, layer, 0, p_ind, 0, p_bit, 1, 0)

    # (the two words' bits alternate in both physical lines)
    assert {hr.site(scheme, 16, F["tmem"], 2, b)[0] for b in range(16)} == {2, 3} == {hr.site(scheme, 16, F["tmem"], 3, b)[0] for b in range(16)}
    double3 = pack(hit(3, 1), hit(3, 6))
    assert (double3 != clean).any()
    assert (pack(hit(2, 4), hit(3, 1), hit(3, 6)) == double3).all()
    assert (pack(hit(2, 4), hit(3, 1), hit(3, 6), REPAIR) == double3).all()
    assert (pack(hit(2, 4), hit(3, 1), hit(3, 6), REPAIR, hit(2, 11)) == double3).all()   # line 2: a single again
    assert (pack(hit(2, 4), hit(3, 1), hit(3, 6), hit(2, 11)) != double3).any()           # without the repair: a double there too
    assert (pack(hit(2, 4), hit(3, 1), hit(3, 6), REPAIR, hit(3, 1)) == clean).all()      # line 3's double was left: back to a single
    # a burst of 2 on the shared line is one bit of each word: both corrected, both cleared by the repair
    p_ind, p_bit = hr.site(scheme, 16, F["tmem"], 2, 4)
    burst = rec(1, layer, 0, p_ind, 0, p_bit & ~1, 2, 0)
    assert (pack(burst, REPAIR, burst, REPAIR, hit(2, 0), hit(3, 0)) == clean).all()
