"""bnn_mi355x_pack_params_iwecc, host side (no GPU): pack_params_wecc plus weight_interleave, against the plain-Python route
of tests/iwecc_ref.py, blobs byte for byte.
  consequence 1  a single event of any width <= D, at every position of a group, in either memory, is corrected: the blob
                 is the loaded one and no code word is at status 2
  consequence 2  an aligned burst of 2 D in an element that wide leaves all D code words at status 2, nothing corrected
  the difference from weight_code 1, which fails without the feature: one burst-2 event in cnvW1A1 layer 1
  accepted triples and repairs that lock in a wrong code word whose bits lie on other physical words than the events
  seeded streams with markers under scheme 1, scheme 0 + code 1 and scheme 2 + code 1; weight_interleave 0 is pack_params_wecc
  the COVERAGE CONDITION of tests/test_gpu_iwecc_exposure.py, from the Python route alone."""
import itertools

import numpy as np
import pytest

import gpu_lib as gl
import hardened_ref as hr
import iwecc_ref as ir
import repair_ref as rr
import wecc_ref as wr

q32 = hr.q32
REPAIR, REWRITE = rr.marker(rr.REPAIR), rr.marker(rr.REWRITE)
NETS = ["cnvW1A1", "cnvW1A2", "cnvW2A2", "lfcW1A1", "lfcW1A2"]


def pdir_of(network):
    return gl.param_dir("cifar10" if network.startswith("cnv") else "mnist", network)


def cat(*parts):
    return np.concatenate([np.zeros((0, 9), np.int32)] + [np.asarray(p, np.int32).reshape(-1, 9) for p in parts])


def data_hit(network, layer, site, ws=1):
    """a record of the data memory: the aligned group of `ws` bits that starts at site `site` of the layer"""
    F = hr.params_io.layout(network)[layer]
    eb = hr.ebits(network, layer, 0)
    el = site // eb
    return np.array([[0, 0, layer, el // F["wmem"], el % F["wmem"], 0, site % eb, ws, 0]], np.int32)


def check_hit(network, layer, r, ws=1):
    """a record of the check memory: bit r = 8 * element + bit of the layer's check bits"""
    cwpp = wr.words_per_pe(network, 1, layer)
    el = r // 8
    return np.array([[0, 0, layer, el // cwpp, el % cwpp, 0, r % 8, ws, 1]], np.int32)


def pairs():
    """one layer per distinct (element width, depth) of the five nets: the one with the most groups"""
    best = {}
    for n in NETS:
        for l in wr.coded_layers(n, 1):
            key = (hr.ebits(n, l, 0), ir.depth(n, 1, 1, l))
            groups = hr.params_io.layout(n)[l]["pe"] * wr.words_per_pe(n, 1, l) // key[1]
            if key not in best or groups > best[key][2]:
                best[key] = (n, l, groups)
    return sorted((n, l, eb, D, g) for (eb, D), (n, l, g) in best.items())


PAIRS = pairs()


def test_the_pairs_cover_every_depth():
    assert {D for _, _, _, D, _ in PAIRS} == {2, 8, 16}, PAIRS


@pytest.mark.parametrize("network,layer,eb,D,groups", PAIRS, ids=str)
def test_consequence_1_every_single_event_is_corrected(network, layer, eb, D, groups):
    """every aligned event position of ONE group's storage, bursts 1 ... D, data and check memory.  The groups of a layer are
    independent, so the k-th position is placed in group k % groups at the same offset: one blob holds up to `groups` single
    events, each alone in its group.  The blob is the loaded one; the Python route sees exactly one status-1 code word per
    flipped bit and none at status 2."""
    L = gl.load(network)
    pdir = pdir_of(network)
    clean = gl.pack_params(network, pdir)
    w0 = hr.read_words(pdir, network)[0][layer]
    calls = 0
    for b in range(1, D + 1):
        events = []  # (module, offset in the group, bits flipped)
        for width, module in ((eb, 0), (8, 1)):
            per_group = (64, 8)[module] * D
            for el in range(per_group // width):
                for g in range(-(-width // b)):
                    events.append((module, el * width + g * b, min(b, width - g * b)))
        for at in range(0, len(events), groups):
            chunk = events[at: at + groups]
            recs = cat(*[(data_hit(network, layer, G * 64 * D + off, b) if m == 0 else check_hit(network, layer, G * 8 * D + off, b))
                         for G, (m, off, _) in enumerate(chunk)])
            assert (ir.lib_pack(L, pdir, 0, 0, 1, 1, recs) == clean).all(), (b, at)
            calls += 1
            mem = ir.IWCoded(network, layer, w0)
            assert mem.apply(recs) == sum(n for _, _, n in chunk)
            _, differ, st1, st2 = mem.logical()
            assert (differ, st1, st2) == (0, sum(n for _, _, n in chunk), 0), (b, at)
            assert mem.repair() == (st1, 0)
    print(network, layer, "calls", calls)


def test_consequence_2_the_depths_limit():
    """an aligned burst of 2 D: two flipped bits in each of the group's D code words, status 2 for all, nothing corrected --
    what is delivered is what the uncoded memory would deliver.  D = 2: cnvW1A1 layer 1 at burst 4; D = 8: cnvW1A1 layer 2
    at burst 16.  D = 16 would need a burst of 32 in a 64-bit element of LFC layer 0: bursts end at 16 (kMaxBurst), so that
    case cannot be reached and is not asserted."""
    network = "cnvW1A1"
    L = gl.load(network)
    pdir = pdir_of(network)
    clean = gl.pack_params(network, pdir)
    w0 = hr.read_words(pdir, network)[0]
    for layer, D in ((1, 2), (2, 8)):
        assert ir.depth(network, 1, 1, layer) == D and hr.ebits(network, layer, 0) >= 2 * D
        for site in (0, 64 * D * 3 + 2 * D):
            r = data_hit(network, layer, site, 2 * D)
            got = ir.lib_pack(L, pdir, 0, 0, 1, 1, r)
            assert (got != clean).any() and (got == wr.lib_pack(L, pdir, 0, 0, 0, r)).all()
            mem = ir.IWCoded(network, layer, w0[layer])
            assert mem.apply(r) == 2 * D
            assert mem.logical()[1:] == (2 * D, 0, D)
            assert (ir.lib_pack(L, pdir, 0, 0, 1, 1, cat(r, REPAIR)) == got).all() and mem.repair() == (0, D)
    assert ir.depth("lfcW1A1", 1, 1, 0) == 16 and 2 * 16 > ir.MAX_BURST
    assert L.bnn_mi355x_wecc_exposure_mask(0, 0, 1, 32, 1, 0, 1, 0, 0, 1, 0, None, 0) == -1  # (a burst of 32 is refused)


def test_the_difference_from_weight_code_1():
    """ONE burst-2 event in cnvW1A1 layer 1 (32-bit elements, D = 2).  Not interleaved, both bits fall into one code word:
    status 2, the data delivered as stored, two weights wrong, and a repair writes nothing.  Interleaved, they fall into two
    code words: both corrected, the loaded weights delivered, and a repair returns the state to the loaded one."""
    network, layer = "cnvW1A1", 1
    L = gl.load(network)
    pdir = pdir_of(network)
    clean = gl.pack_params(network, pdir)
    w0 = hr.read_words(pdir, network)[0][layer]
    ev = data_hit(network, layer, 64 * 7 + 10, 2)
    stored = wr.lib_pack(L, pdir, 0, 0, 0, ev)  # the uncoded memory
    assert (stored != clean).any()
    plain = wr.lib_pack(L, pdir, 0, 0, 1, ev)
    assert (plain == stored).all() and (ir.lib_pack(L, pdir, 0, 0, 1, 0, ev) == stored).all()
    old = wr.WCoded(network, layer, w0)
    old.apply(ev)
    assert old.logical()[1:] == (2, 0, 1)  # two weights wrong, one code word at status 2
    new = ir.IWCoded(network, layer, w0)
    new.apply(ev)
    assert new.logical()[1:] == (0, 2, 0)
    assert (ir.lib_pack(L, pdir, 0, 0, 1, 1, ev) == clean).all()
    # a repair marker: the interleaved state returns to the loaded one, the other stays as it was
    assert new.repair() == (2, 0) and (new.data == new.files).all() and (new.check == new.files_check).all()
    assert old.repair() == (0, 1) and (old.data != old.files).sum() == 1
    # seen from outside: a later single in one of the two code words meets a clean word (with the repair) or a hit one
    later = data_hit(network, layer, 64 * 7 + 20, 1)  # the same code word as site 64 * 7 + 10 (an even offset: word 0 of the group)
    assert ir.site_of(network, 1, layer, 0, 64 * 7 + 20)[0] == ir.site_of(network, 1, layer, 0, 64 * 7 + 10)[0]
    assert (ir.lib_pack(L, pdir, 0, 0, 1, 1, cat(ev, REPAIR, later)) == clean).all()
    assert (ir.lib_pack(L, pdir, 0, 0, 1, 1, cat(ev, later)) != clean).any()
    assert (wr.lib_pack(L, pdir, 0, 0, 1, cat(ev, REPAIR, later)) == wr.lib_pack(L, pdir, 0, 0, 1, cat(ev, later))).all()


@pytest.mark.parametrize("network,layer", [("cnvW1A1", 2), ("cnvW2A2", 1), ("lfcW1A1", 0)], ids=str)
def test_accepted_triples_lock_in_bits_on_other_physical_words(network, layer):
    """three single hits in ONE code word, chosen so that the decoder accepts them as a correction of a data bit that lies
    in ANOTHER physical 64-site word than any of the three: the delivered data is
    wrong there, a repair locks it in (a valid wrong code word), later repairs leave it, a rewrite clears it"""
    L = gl.load(network)
    pdir = pdir_of(network)
    clean = gl.pack_params(network, pdir)
    D = ir.depth(network, 1, 1, layer)
    G, c = 5, D - 1
    base = G * 64 * D
    site = lambda k: base + k * D + c
    triple = fourth = None
    for t in itertools.combinations(range(8), 3):  # the code word's first data bits: the group's first one or two physical words
        st, out = wr.decode(sum(1 << k for k in t), 0)
        extra = out ^ sum(1 << k for k in t)
        if st == 1 and extra and site(extra.bit_length() - 1) // 64 not in {site(k) // 64 for k in t}:
            triple, fourth = t, extra.bit_length() - 1
            break
    assert triple is not None
    assert site(fourth) // 64 not in {site(k) // 64 for k in triple} and site(fourth) < base + 64 * D
    assert all(ir.site_of(network, 1, layer, 0, site(k)) == (G * D + c, k) for k in triple + (fourth,))
    three = cat(*[data_hit(network, layer, site(k)) for k in triple])
    pack = lambda *parts: ir.lib_pack(L, pdir, 0, 0, 1, 1, cat(*parts))
    wrong = pack(three)
    assert (wrong != clean).any()
    assert (wrong == wr.lib_pack(L, pdir, 0, 0, 0, cat(three, data_hit(network, layer, site(fourth))))).all()  # four weights wrong, one elsewhere
    assert (pack(three, REPAIR) == wrong).all() and (pack(three, REPAIR, REPAIR) == wrong).all()
    # locked in: a later single in that code word is corrected back to the WRONG word; without the repair it makes a quadruple
    again = data_hit(network, layer, site(triple[0]))
    assert (pack(three, REPAIR, again) == wrong).all() and (pack(three, again) != wrong).any()
    assert (pack(three, REPAIR, REWRITE) == clean).all()
    mem = ir.IWCoded(network, layer, hr.read_words(pdir, network)[0][layer], track=True)
    mem.apply(three)
    assert mem.logical()[1:] == (4, 1, 0) and mem.flags["w_accepted_triple"] and mem.flags["w_elsewhere"]
    assert mem.repair() == (1, 1) and mem.flags["w_locked"]


@pytest.mark.parametrize("network,scheme,code,burst", [("cnvW1A1", 1, 0, 2), ("cnvW1A1", 0, 1, 4), ("cnvW1A1", 2, 1, 2), ("cnvW2A2", 0, 1, 4),
                                                       ("lfcW1A1", 0, 1, 2), ("lfcW1A2", 0, 0, 3)], ids=str)
def test_against_the_independent_route(network, scheme, code, burst, tmp_path):
    """three seeded epochs at the GPU test's rates: without markers, with repairs, and with repairs and a rewrite mixed,
    pack_params_iwecc gives the plain-Python route's blob; weight_interleave 0 gives pack_params_wecc's; the interleave
    changes the blob"""
    L = gl.load(network)
    pdir = pdir_of(network)
    rw, rt = wr.gpu_rates(network, code)
    e = [wr.flat(wr.lib_epoch_events(L, network, scheme, code, 1, burst, 4343, t, rw, rt)) for t in range(3)]
    plain = cat(*e)
    bare = ir.lib_pack(L, pdir, scheme, code, 1, 1, plain)
    assert (bare == ir.pack(network, scheme, code, 1, 1, pdir, plain, str(tmp_path / "a"))).all()
    assert (bare != wr.lib_pack(L, pdir, scheme, code, 1, plain)).any()
    mixed = cat(e[0], REPAIR, e[1], REWRITE, e[2], REPAIR, e[1], REPAIR, e[0])
    got = ir.lib_pack(L, pdir, scheme, code, 1, 1, mixed)
    assert (got == ir.pack(network, scheme, code, 1, 1, pdir, mixed, str(tmp_path / "b"))).all()
    for stream in (plain, mixed):
        assert (ir.lib_pack(L, pdir, scheme, code, 1, 0, stream) == wr.lib_pack(L, pdir, scheme, code, 1, stream)).all()
    uncoded = plain[~(wr.mine(network, 1, plain) & (plain[:, 8] == 1))]
    assert (ir.lib_pack(L, pdir, scheme, code, 0, 0, uncoded) == rr.lib_pack(L, pdir, scheme, code, uncoded)).all()
    assert (ir.lib_pack(L, pdir, scheme, code, 1, 1, cat(e[0], REPAIR, REWRITE)) == gl.pack_params(network, pdir)).all()


@pytest.mark.parametrize("network,layer", [("cnvW1A1", 1), ("cnvW2A2", 1), ("lfcW1A1", 3)], ids=str)
def test_coverage_condition_of_the_gpu_test(network, layer):
    """the GPU test's shape -- 3 runs, 4 epochs, rate 2^-7, bursts 1, 2, 4, its schedules -- through the plain-Python draw and
    route alone: over those seeds the layer shows (a) a burst whose bits were corrected in two or more different code words,
    (b) a status-2 code word, (c) an accepted triple, (d) a repair that locks in a wrong word, (e) a correction whose
    scattered bit changes a physical word no event of that epoch touched -- so the GPU test's equalities cover those cases"""
    w0 = hr.read_words(pdir_of(network), network)[0][layer]
    rate = q32(wr.GPU_RATE)
    seen = {}
    for burst in (1, 2, 4):
        for every, repair in wr.GPU_SCHEDULES:
            for r in range(wr.GPU_RUNS):
                mem = ir.IWCoded(network, layer, w0, track=True)
                for t in range(wr.GPU_EPOCHS):
                    if rr.rewrites(t, every):
                        mem.rewrite()
                    elif rr.repairs(t, every, repair):
                        mem.repair()
                    mem.apply(np.concatenate([wr.events(network, 0, 0, 1, burst, wr.GPU_SEED + r, t, layer, 0, m, rate) for m in (0, 1)]))
                    mem.logical()
                for k, v in mem.flags.items():
                    seen[k] = seen.get(k, False) or v
    print(network, layer, seen)
    assert seen["w_burst_in_words"] and seen["w_status2"] and seen["w_accepted_triple"] and seen["w_locked"] and seen["w_elsewhere"], seen
