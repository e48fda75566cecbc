"""bnn_mi355x_pack_params_wecc, host side (no GPU): pack_params_repair plus weight_code, against the plain-Python route of
tests/wecc_ref.py, byte for byte, for cnvW1A1, cnvW2A2 (-2 fields and row flags), lfcW1A1 (layer 0 coded, kw = 13, 64-bit
elements) and lfcW1A2, bursts 1, 2 and 8, with and without markers; weight_code 0 is pack_params_repair byte for byte;
hand-made sequences on one code word; and the COVERAGE CONDITION of tests/test_gpu_wecc_exposure.py: for its seeds and
rates the plain-Python route alone shows, in the smallest tested layers, a code word at status 1, one at status 2, an
accepted triple and a repair that locks in a wrong word."""
import struct

import numpy as np
import pytest

import gpu_lib as gl
import hardened_ref as hr
import repair_ref as rr
import wecc_ref as wr

q32 = hr.q32
REPAIR, REWRITE = rr.marker(rr.REPAIR), rr.marker(rr.REWRITE)
CASES = [(n, s, c, b) for n, cases in sorted(wr.GPU_CASES.items()) for s, c, b in cases] + \
        [("cnvW1A1", 1, 0, 8), ("cnvW2A2", 0, 0, 8), ("lfcW1A1", 0, 0, 8), ("lfcW1A2", 0, 1, 8)]


def pdir_of(network):
    return gl.param_dir(wr.GPU_DATASET[network], network)


def rec(target, layer, mem, ind, thresh, bit, ws, module):
    return np.array([[0, target, layer, mem, ind, thresh, bit, ws, module]], np.int32)


def cat(*parts):
    return np.concatenate([np.zeros((0, 9), np.int32)] + [np.asarray(p, np.int32).reshape(-1, 9) for p in parts])


@pytest.mark.parametrize("network,scheme,code,burst", CASES, ids=str)
def test_against_the_independent_route(network, scheme, code, burst, tmp_path):
    """three seeded epochs at the GPU test's rates: without markers, with a repair before epochs 1 and 2, and with repairs
    and a rewrite mixed, pack_params_wecc gives the plain-Python route's blob; weight_code 0 gives pack_params_repair's; the
    code changes the blob, and a repair changes what later upsets make of it"""
    L = gl.load(network)
    pdir = pdir_of(network)
    rw, rt = wr.gpu_rates(network, code)
    e = [wr.flat(wr.lib_epoch_events(L, network, scheme, code, 1, burst, 4242, t, rw, rt)) for t in range(3)]
    plain = cat(*e)
    assert wr.mine(network, 1, plain).sum() > 200 and (plain[wr.mine(network, 1, plain)][:, 8] == 1).sum() > 20
    uncoded = plain[~(wr.mine(network, 1, plain) & (plain[:, 8] == 1))]  # (without the check memories' records)
    bare = wr.lib_pack(L, pdir, scheme, code, 1, plain)
    assert (bare == wr.pack(network, scheme, code, 1, pdir, plain, str(tmp_path / "a"))).all()
    assert (wr.lib_pack(L, pdir, scheme, code, 0, uncoded) == rr.lib_pack(L, pdir, scheme, code, uncoded)).all()
    # (an aligned burst of 2 in a memory whose elements -- and the 8 check bits -- are an even number of bits wide flips an
    # even number of bits of a code word, always: the overall parity never fires, nothing is ever corrected, and the delivered
    # data is the stored data)
    corrects = burst == 1 or any(hr.ebits(network, l, 0) == 1 for l in wr.coded_layers(network, 1))
    assert (bare != rr.lib_pack(L, pdir, scheme, code, uncoded)).any() == corrects
    wr.lib_pack(L, pdir, scheme, code, 0, plain, expect_error=b"pack_params_wecc: record")  # (weight_code 0 has no such module)
    repaired = cat(e[0], REPAIR, e[1], REPAIR, e[2])
    got = wr.lib_pack(L, pdir, scheme, code, 1, repaired)
    assert (got == wr.pack(network, scheme, code, 1, pdir, repaired, str(tmp_path / "b"))).all()
    assert (got != bare).any() == corrects
    mixed = cat(e[0], REPAIR, e[1], REWRITE, e[2], REPAIR, e[1], REPAIR)
    assert (wr.lib_pack(L, pdir, scheme, code, 1, mixed) == wr.pack(network, scheme, code, 1, pdir, mixed, str(tmp_path / "c"))).all()
    assert (wr.lib_pack(L, pdir, scheme, code, 1, cat(repaired, REPAIR)) == got).all()  # a trailing repair never changes what is delivered
    assert (wr.lib_pack(L, pdir, scheme, code, 1, cat(e[0], e[1], REWRITE, e[2])) == wr.lib_pack(L, pdir, scheme, code, 1, e[2])).all()
    assert (wr.lib_pack(L, pdir, scheme, code, 1, cat(e[0], REPAIR, REWRITE)) == gl.pack_params(network, pdir)).all()
    with_marker = cat(uncoded[: len(uncoded) // 2], REPAIR, uncoded[len(uncoded) // 2:])
    assert (wr.lib_pack(L, pdir, scheme, code, 0, with_marker) == rr.lib_pack(L, pdir, scheme, code, with_marker)).all()


def flags(blob, layer):
    off, rd, rows, kw = struct.unpack_from("<4I", blob, 32 + 16 * layer)
    return blob[off: off + rows * rd * 4].view(np.uint32).reshape(rows, rd)[:, 2 + 6 * kw]


@pytest.mark.parametrize("network,layer", [("cnvW1A1", 2), ("cnvW2A2", 3), ("lfcW1A1", 0), ("lfcW1A2", 3)], ids=str)
def test_sequences_on_one_code_word(network, layer):
    L = gl.load(network)
    pdir = pdir_of(network)
    clean = gl.pack_params(network, pdir)
    F = hr.params_io.layout(network)[layer]
    eb = hr.ebits(network, layer, 0)
    cwpp = wr.words_per_pe(network, 1, layer)
    pe, cw = F["pe"] - 1, cwpp - 1  # (the last code word of the last PE)
    pack = lambda *parts, wc=1: wr.lib_pack(L, pdir, 0, 0, wc, cat(*parts))

    def hit(k):
        """a burst-1 record of data bit 0 ... 63 or check bit 64 ... 71 of the code word"""
        if k < 64:
            return rec(0, layer, pe, (cw * 64 + k) // eb, 0, (cw * 64 + k) % eb, 1, 0)
        return rec(0, layer, pe, cw, 0, k - 64, 1, 1)

    for a, b in ((3, 40), (0, 65), (70, 71), (63, 64)):
        assert (pack(hit(a)) == clean).all() and (pack(hit(b)) == clean).all()
        double = pack(hit(a), hit(b))
        data_only = cat(*[hit(k) for k in (a, b) if k < 64])
        assert (double == pack(data_only, wc=0)).all()  # detected, the data as stored
        if a < 64:
            assert (double != clean).any()
        assert (pack(hit(a), REPAIR, hit(b)) == clean).all()  # single, repair, single: without the repair it is a double
        assert (pack(hit(a), hit(b), REPAIR) == double).all()
        assert (pack(hit(a), hit(b), REPAIR, hit(a)) == clean).all()
    # the neighbouring code word is another word: two singles
    if cwpp > 1:
        other = rec(0, layer, pe, ((cw - 1) * 64 + 5) // eb, 0, ((cw - 1) * 64 + 5) % eb, 1, 0)
        assert (pack(hit(7), other) == clean).all()
    # an accepted triple: wrong data with status 1; repaired, a valid wrong word that later singles are corrected back to
    triple = next(t for t in ((0, 1, 2), (0, 1, 3), (0, 2, 5), (1, 2, 4), (3, 4, 5), (0, 4, 7)) if wr.decode(sum(1 << k for k in t), 0)[0] == 1)
    st, nd, nc = wr.repair_word(sum(1 << k for k in triple), 0)
    fourth = [k for k in range(72) if ((nd | nc << 64) >> k) & 1 and k not in triple]
    assert st == 1 and nd != 0 and len(fourth) == 1
    three = [hit(k) for k in triple]
    wrong = pack(*three)
    assert (wrong != clean).any() and (pack(*three, REPAIR) == wrong).all()
    assert (pack(*three, REPAIR, hit(triple[0])) == wrong).all() and (pack(*three, hit(triple[0])) != wrong).any()
    assert (pack(*three, REPAIR, hit(triple[0]), REPAIR, hit(fourth[0])) == wrong).all()
    assert (pack(*three, REPAIR, REWRITE) == clean).all()
    # bursts: clipped to the element and to the 8 check bits
    assert (pack(rec(0, layer, pe, cw, 0, 6, 4, 1)) == pack(hit(68), hit(69), hit(70), hit(71))).all()
    if eb >= 2:
        assert (pack(rec(0, layer, pe, (cw * 64) // eb, 0, 0, 2, 0)) == pack(hit(0), hit(1))).all()


def test_two_bit_fields_and_row_flags():
    """cnvW2A2 layer 6: a single hit that would make a -2 (the high bit of a 0 field) is corrected and the row's flag stays
    0; two such hits in one code word are delivered as stored and set it; a later hit that makes the word a single again
    clears it"""
    network, layer = "cnvW2A2", 6
    L = gl.load(network)
    pdir = pdir_of(network)
    clean = gl.pack_params(network, pdir)
    F = hr.params_io.layout(network)[layer]
    eb = hr.ebits(network, layer, 0)
    w0 = hr.read_words(pdir, network)[0][layer]
    pack = lambda *parts, wc=1: wr.lib_pack(L, pdir, 0, 0, wc, cat(*parts))
    assert (flags(clean, layer) == 0).all()
    # two 0 fields (both bits clear) inside one code word of PE 0
    sites = [s for s in range(0, 64 * 8, 2) if not (w0[0][s // eb] >> (s % eb)) & 3]
    a, b = next((x, y) for x in sites for y in sites if x < y and x // 64 == y // 64)
    hi = lambda s: rec(0, layer, 0, (s + 1) // eb, 0, (s + 1) % eb, 1, 0)
    assert (pack(hi(a), wc=0) != clean).any() and flags(pack(hi(a), wc=0), layer).sum() == 1
    assert (pack(hi(a)) == clean).all()
    double = pack(hi(a), hi(b))
    assert flags(double, layer).sum() == 1 and (double == pack(hi(a), hi(b), wc=0)).all()
    assert (pack(hi(a), hi(b), hi(a)) == clean).all()
    row = int(np.nonzero(flags(double, layer))[0][0])
    assert row % F["pe"] == 0


@pytest.mark.parametrize("network,layer,words", [("cnvW1A1", 8, 512), ("lfcW1A1", 3, 1024), ("lfcW1A2", 3, 1024)], ids=str)
def test_coverage_condition_of_the_gpu_test(network, layer, words):
    """the GPU test's seeds and rates, the plain-Python draw and route alone, repair every epoch: the smallest tested layer
    shows a code word at status 1, one at status 2, an accepted triple (status 1 with wrong data) and a repair that locks in
    a wrong word -- so the GPU test's equalities cover those cases"""
    F = hr.params_io.layout(network)[layer]
    assert F["pe"] * wr.words_per_pe(network, 1, layer) == words
    w0 = hr.read_words(pdir_of(network), network)[0][layer]
    rate = q32(wr.GPU_RATE)
    seen = {}
    for burst in sorted({b for _, _, b in wr.GPU_CASES[network]}):
        flags_ = dict()
        for r in range(wr.GPU_RUNS):
            mem = wr.WCoded(network, layer, w0)
            for t in range(wr.GPU_EPOCHS):
                if t > 0:
                    mem.repair()
                mem.apply(np.concatenate([wr.events(network, 0, 0, 1, burst, wr.GPU_SEED + r, t, layer, 0, m, rate) for m in (0, 1)]))
                mem.logical()
            for k, v in mem.flags.items():
                flags_[k] = flags_.get(k, False) or v
        seen[burst] = flags_
        if burst % 2 == 0 and hr.ebits(network, layer, 0) % 2 == 0:
            # an aligned even burst in even-width elements (and in the 8 check bits) flips an even number of a code word's bits:
            # the overall parity never fires, so status 1 cannot occur at any rate or seed -- every hit word is detected
            assert flags_["w_status2"] and not (flags_["w_status1"] or flags_["w_accepted_triple"] or flags_["w_locked"] or flags_["w_cleared"]), (burst, flags_)
            continue
        assert flags_["w_status1"] and flags_["w_status2"] and flags_["w_accepted_triple"] and flags_["w_locked"] and flags_["w_cleared"], (burst, flags_)
    print(seen)


def test_refusals():
    L = gl.load("cnvW1A1")
    pdir = pdir_of("cnvW1A1")
    ok = rec(0, 1, 0, 0, 0, 0, 1, 1)
    assert wr.lib_pack(L, pdir, 0, 0, 1, ok) is not None
    for wc in (-1, 2, 7):
        wr.lib_pack(L, pdir, 0, 0, wc, ok, expect_error=b"pack_params_wecc: weight_code must be 0 (none) or 1")
    wr.lib_pack(L, pdir, 1, 1, 1, ok, expect_error=b"pack_params_wecc: code 1 with scheme 1 (TMR)")
    wr.lib_pack(L, pdir, 0, 0, 1, rec(0, 0, 0, 0, 0, 0, 1, 1), expect_error=b"pack_params_wecc: record 0: fault record out of range")  # (CNV layer 0 is not coded)
    wr.lib_pack(L, pdir, 0, 0, 1, rec(0, 1, 0, 0, 0, 8, 1, 1), expect_error=b"record 0: fault record out of range")  # (check bit 8)
    wr.lib_pack(L, pdir, 0, 0, 1, rec(0, 1, 0, wr.words_per_pe("cnvW1A1", 1, 1), 0, 0, 1, 1), expect_error=b"record 0: fault record out of range")
    bad = rr.marker(-3)
    wr.lib_pack(L, pdir, 0, 0, 1, cat(ok, bad), expect_error=b"pack_params_wecc: record 1: layer -3 is no marker")
