"""Hardened memory schemes in the memory upset campaigns, host side (no GPU): the memory-organisation model of
csrc/mem_org.h.  bnn_mi355x_hardened_site against the table the reference's interleave.h prints
(tests/golden/interleave_maps.json), bnn_mi355x_hardening_layout against the reference's tables restated in
tests/hardened_ref.py, the draw against its plain-Python restatement, bnn_mi355x_pack_params_hardened's voter and
de-interleaver against pack_params_faulty and against a route of its own, and the refusals of the device entry points,
which come before anything touches a device."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import gpu_lib as gl
import hardened_ref as hr
import test_mem_noise_mask as mm

ip = C.POINTER(C.c_int)
q32 = hr.q32
CNV = ["cnvW1A1", "cnvW1A2", "cnvW2A2"]
PAIRS = [(n, s) for n in CNV for s in hr.SUPPORTED[n]]


def lib_site(L, scheme, layer, target, ind, bit):
    a, b = C.c_int(-1), C.c_int(-1)
    assert L.bnn_mi355x_hardened_site(scheme, layer, target, ind, bit, C.byref(a), C.byref(b)) == 0, L.bnn_mi355x_last_error()
    return a.value, b.value


def pdir_of(network):
    return gl.param_dir("cifar10" if network.startswith("cnv") else "mnist", network)


def test_site_equals_the_golden_map():
    """schemes 2 and 3, T = 16 (layer 1) and 24 (layer 0), both lines of a pair, every pair of a PE: the library's
    logical -> physical map is the table the reference's interleave.h gives"""
    with open(os.path.join(gl.ROOT, "tests", "golden", "interleave_maps.json")) as f:
        golden = json.load(f)
    assert sorted(golden) == ["2/16", "2/24", "3/16", "3/24"]
    L = gl.load("cnvW1A1")
    for scheme in (2, 3):
        for layer, T in ((0, 24), (1, 16)):
            table = golden["%d/%d" % (scheme, T)]
            lines = hr.params_io.layout("cnvW1A1")[layer]["tmem"]
            seen = set()
            for ind in range(lines):
                for bit in range(T):
                    off, pbit = table[ind & 1][bit]
                    assert lib_site(L, scheme, layer, 1, ind, bit) == ((ind & ~1) + off, pbit), (scheme, layer, ind, bit)
                    assert hr.site(scheme, T, lines, ind, bit) == ((ind & ~1) + off, pbit)
                    seen.add(((ind & ~1) + off, pbit))
            assert len(seen) == lines * T  # (a permutation)
    # the examples of the header: scheme 3, T = 16
    assert lib_site(L, 3, 1, 1, 0, 15) == (0, 15) and lib_site(L, 3, 1, 1, 1, 15) == (1, 0) and lib_site(L, 3, 1, 1, 1, 0) == (0, 14)
    # weights are not interleaved, nor are thresholds without the scheme
    assert lib_site(L, 3, 1, 0, 5, 7) == (5, 7) and lib_site(L, 1, 1, 1, 1, 7) == (1, 7) and lib_site(L, 0, 0, 1, 3, 23) == (3, 23)
    for bad in ((2, 8, 1, 0, 0), (2, 1, 1, 2, 0), (2, 1, 1, 0, 16), (2, 1, 2, 0, 0), (4, 1, 1, 0, 0), (2, 9, 1, 0, 0)):
        assert L.bnn_mi355x_hardened_site(*bad, None, None) == -1
        assert b"hardened_site" in L.bnn_mi355x_last_error()


def test_mapping_function_with_an_odd_line_count(tmp_path):
    """no CNV threshold memory has an odd number of lines: the shared mapping function itself (csrc/mem_org.h), compiled
    into a stand-alone host program.  With 5 lines, lines 0-3 pair up as ever and line 4 is stored as is; the inverse
    function inverts it everywhere."""
    import shutil
    import subprocess
    cxx = [shutil.which("g++")] if shutil.which("g++") else ["/opt/rocm/bin/hipcc", "-x", "c++"]
    src = tmp_path / "odd.cpp"
    src.write_text('#include <cstdio>\n#include "mem_org.h"\nint main() {\n  for (int il : {0, 2, 3}) for (int T : {16, 24}) for (int ind = 0; ind < 5; ind++) '
                   'for (int bit = 0; bit < T; bit++) {\n    int a, b, c, d;\n    bnn::interleave_site(il, T, 5, ind, bit, &a, &b);\n'
                   '    bnn::interleave_source(il, T, 5, a, b, &c, &d);\n    std::printf("%d %d %d %d %d %d %d %d\\n", il, T, ind, bit, a, b, c, d);\n  }\n}\n')
    exe = tmp_path / "odd"
    subprocess.run(cxx + ["-std=c++17", "-I", os.path.join(gl.ROOT, "bnn-pynq_amd", "csrc"), str(src), "-o", str(exe)], check=True)
    rows = [tuple(map(int, line.split())) for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n") if line]
    assert len(rows) == 3 * (16 + 24) * 5
    for il, T, ind, bit, a, b, c, d in rows:
        assert (c, d) == (ind, bit)
        assert (a, b) == hr.site(il, T, 5, ind, bit)
        if ind == 4 or il == 0:
            assert (a, b) == (ind, bit)
    assert any((a, b) != (ind, bit) for il, T, ind, bit, a, b, c, d in rows if il and ind < 4)


@pytest.mark.parametrize("network", CNV + ["lfcW1A1", "lfcW1A2"])
def test_layout_and_refusals(network):
    L = gl.load(network)
    out = (C.c_int * 3)()
    nl = len(hr.params_io.layout(network))
    assert L.bnn_mi355x_hardening_scheme() == 0
    for layer in range(nl):
        assert L.bnn_mi355x_hardening_layout(0, layer, out) == 0 and list(out) == [1, 1, 0]
    for scheme in (1, 2, 3):
        if scheme in hr.SUPPORTED.get(network, ()):
            for layer in range(nl):
                assert L.bnn_mi355x_hardening_layout(scheme, layer, out) == 0
                assert tuple(out) == hr.org(network, scheme, layer), (scheme, layer)
            continue
        assert L.bnn_mi355x_hardening_layout(scheme, 0, out) == -1
        err = L.bnn_mi355x_last_error()
        assert (b"cnvW2A2 with scheme 2" in err and b"no defined layout" in err) if network == "cnvW2A2" else (b"LFC" in err and network.encode() in err)
        assert L.bnn_mi355x_hardened_mem_noise_mask(scheme, 1, 5, 0, 0, 0, 1 << 28, 0, None, 0) == -1
        assert L.bnn_mi355x_pack_params_hardened(pdir_of(network).encode(), scheme, None, 0, None, 0) == 0
    for scheme, layer in ((-1, 0), (4, 0), (1, -1), (1, nl)):
        assert L.bnn_mi355x_hardening_layout(scheme, layer, out) == -1
    if network == "cnvW1A1":  # the tables, spelled out once
        tmr = [hr.org(network, 1, l) for l in range(9)]
        assert tmr == [(3, 3, 0)] + [(1, 3, 0)] * 4 + [(1, 1, 0)] * 4
        assert [hr.org(network, 3, l) for l in range(9)] == [(1, 1, 3)] * 8 + [(1, 1, 0)]


def test_scheme_of_the_variant_libraries(variant_libs):
    for name, scheme in (("cnvW1A1-TMR", 1), ("cnvW1A2-interleaved", 2), ("cnvW2A2-resilient-interleaved", 3), ("lfcW1A2-interleaved", 2)):
        assert gl.load(name).bnn_mi355x_hardening_scheme() == scheme
    # the same code in a variant's library: the scheme is the argument
    L = gl.load("cnvW1A1-TMR")
    out = (C.c_int * 3)()
    assert L.bnn_mi355x_hardening_layout(3, 2, out) == 0 and list(out) == [1, 1, 3]
    assert (hr.lib_mask(L, 1, 4, 9, 0, 1, 2, q32(2.0 ** -3)) == hr.events("cnvW1A1", 4, 9, 0, 1, 2, q32(2.0 ** -3))).all()


@pytest.mark.parametrize("network,scheme", PAIRS + [("lfcW1A2", 0)], ids=str)
def test_mask_equals_the_restatement(network, scheme):
    """every layer, target and module, bursts 1, 3, 4 and 16: the library's records are the events whose Philox word is below
    the rate, in event order; module 0 with burst 1 lists mem_noise_mask's sites"""
    L = gl.load(network)
    nl = len(hr.params_io.layout(network))
    for layer in list(range(min(nl, 5))) + [nl - 1]:
        for target in (0, 1):
            for m in range(hr.org(network, scheme, layer)[target]):
                for burst, rate, seed in ((1, q32(2.0 ** -7), 77 + layer), (4, q32(2.0 ** -5), 3), (3, q32(2.0 ** -5), (5 << 40) + 3), (16, q32(2.0 ** -4), 8)):
                    got = hr.lib_mask(L, scheme, burst, seed, layer, target, m, rate)
                    want = hr.events(network, burst, seed, layer, target, m, rate)
                    assert got.shape == want.shape and (got == want).all(), (layer, target, m, burst)
                    if burst == 1 and m == 0:
                        assert (got[:, :8] == mm.lib_mask(L, seed, layer, target, rate)).all()
                    if len(got) > 3:  # groups are aligned; the modules' and the bursts' streams differ
                        assert (got[:, 6] % burst == 0).all() and (got[:, 6] < hr.ebits(network, layer, target)).all()
    a = hr.lib_mask(L, scheme, 2, 5, 1, 0, 0, q32(2.0 ** -4))
    assert len(a) > 50 and a.tolist() != hr.lib_mask(L, scheme, 2, 6, 1, 0, 0, q32(2.0 ** -4)).tolist()
    whole = hr.lib_mask(L, scheme, 4, 5, 1, 0, 0, q32(2.0 ** -4))
    pages = [hr.lib_mask(L, scheme, 4, 5, 1, 0, 0, q32(2.0 ** -4), first, 7) for first in range(0, len(whole) + 7, 7)]
    assert (np.concatenate(pages) == whole).all()
    for bad in ((scheme, 0), (scheme, 17), (5, 1)):
        assert L.bnn_mi355x_hardened_mem_noise_mask(bad[0], bad[1], 5, 1, 0, 0, 1, 0, None, 0) == -1
    assert L.bnn_mi355x_hardened_mem_noise_mask(scheme, 1, 5, 1, 0, 1, 1, 0, None, 0) == -1  # (layer 1's weights have one module)
    assert L.bnn_mi355x_hardened_mem_noise_mask(scheme, 1, 5, 1, 2, 0, 1, 0, None, 0) == -1
    assert L.bnn_mi355x_hardened_mem_noise_mask(scheme, 1, 5, 1, 0, 0, 1, -1, None, 0) == -1


def test_modules_draw_from_different_streams():
    L = gl.load("cnvW1A1")
    m = [hr.lib_mask(L, 1, 1, 5, 1, 1, k, q32(2.0 ** -3))[:, 3:7].tolist() for k in range(3)]
    assert all(len(x) > 60 for x in m) and m[0] != m[1] and m[1] != m[2] and m[0] != m[2]


def rec9(layer, target, mem, ind, thresh, bit, ws, module):
    return [0, target, layer, mem, ind, thresh, bit, ws, module]


@pytest.mark.parametrize("network", CNV)
def test_scheme_0_is_pack_params_faulty(network):
    L, pdir = gl.load(network), pdir_of(network)
    nl = 9
    rw, rt = [q32(2.0 ** -8)] * nl, [q32(2.0 ** -5)] * 8 + [0]
    recs = mm.all_masks(L, network, 31, rw, rt)
    recs9 = np.concatenate([recs, np.zeros((len(recs), 1), np.int32)], axis=1)
    assert (hr.pack_hardened(L, pdir, 0, recs9) == mm.pack_faulty(L, pdir, recs)).all()
    assert (hr.lib_run_events(L, network, 0, 1, 31, rw, rt) == recs9).all()
    bad = recs9[:1].copy()
    bad[0, 8] = 1
    assert L.bnn_mi355x_pack_params_hardened(pdir.encode(), 0, bad.ctypes.data_as(ip), 1, None, 0) == 0
    assert b"module" in L.bnn_mi355x_last_error()


@pytest.mark.parametrize("network", CNV)
def test_tmr_votes(network):
    """any set of faults confined to one module of a word gives the fault-free blob (layer 0's weights and 24-bit thresholds
    included); the same bit in two modules is the logical fault (layers 1-4); three modules as well; layer 5 has one module"""
    L, pdir = gl.load(network), pdir_of(network)
    clean = gl.pack_params(network, pdir)
    rng = np.random.default_rng(5)
    lay = hr.params_io.layout(network)
    single = []
    for layer in range(5):
        F = lay[layer]
        for _ in range(40):  # one module per WORD: the module follows from the word's position
            mem, ind, thresh = int(rng.integers(F["pe"])), int(rng.integers(F["tmem"])), int(rng.integers(F["nthr"]))
            for _ in range(3):
                single.append(rec9(layer, 1, mem, ind, thresh, int(rng.integers(hr.ebits(network, layer, 1))), int(rng.integers(1, 5)),
                                   (mem + ind + thresh) % 3))
    F = lay[0]
    for _ in range(60):
        mem, ind = int(rng.integers(F["pe"])), int(rng.integers(F["wmem"]))
        single.append(rec9(0, 0, mem, ind, 0, int(rng.integers(hr.ebits(network, 0, 0))), 1, (mem + ind) % 3))
    assert (hr.pack_hardened(L, pdir, 1, single) == clean).all()
    for layer in range(1, 5):
        F = lay[layer]
        for mods in ((0, 1), (1, 2), (0, 2), (0, 1, 2)):
            mem, ind, thresh, bit = int(rng.integers(F["pe"])), int(rng.integers(F["tmem"])), int(rng.integers(F["nthr"])), int(rng.integers(16))
            got = hr.pack_hardened(L, pdir, 1, [rec9(layer, 1, mem, ind, thresh, bit, 1, m) for m in mods])
            want = mm.pack_faulty(L, pdir, [rec9(layer, 1, mem, ind, thresh, bit, 1, 0)[:8]])
            assert (got == want).all() and (got != clean).any(), (layer, mods)
    # layer 0's weights: two modules outvote the third
    got = hr.pack_hardened(L, pdir, 1, [rec9(0, 0, 3, 7, 0, 1, 1, 0), rec9(0, 0, 3, 7, 0, 1, 1, 2)])
    assert (got == mm.pack_faulty(L, pdir, [rec9(0, 0, 3, 7, 0, 1, 1, 0)[:8]])).all() and (got != clean).any()
    # not replicated: layer 5's thresholds, layer 1's weights
    for r in (rec9(5, 1, 0, 9, 0, 3, 1, 0), rec9(1, 0, 2, 5, 0, 3, 1, 0)):
        assert (hr.pack_hardened(L, pdir, 1, [r]) == mm.pack_faulty(L, pdir, [r[:8]])).all()
        r[8] = 1
        assert L.bnn_mi355x_pack_params_hardened(pdir.encode(), 1, np.array(r, np.int32).ctypes.data_as(ip), 1, None, 0) == 0


@pytest.mark.parametrize("network,scheme", [p for p in PAIRS if p[1] != 1], ids=str)
def test_interleaved_burst_2(network, scheme):
    """a burst-2 event on a 16-bit threshold line is two 1-bit faults at the bits the golden map gives -- every aligned
    position of both lines of a pair; scheme 2: always one in each neuron of the pair; scheme 3: positions 0 and 1 of line
    ind + 1 hit e2 bit 15 and e1 bit 0"""
    with open(os.path.join(gl.ROOT, "tests", "golden", "interleave_maps.json")) as f:
        table = json.load(f)["%d/16" % scheme]
    inverse = {(off, pbit): (half, bit) for half in (0, 1) for bit, (off, pbit) in enumerate(table[half])}
    L, pdir = gl.load(network), pdir_of(network)
    layer, mem, ind, thresh = 2, 3, 4, 0
    for line in (0, 1):
        for g in range(8):
            hit = [inverse[(line, 2 * g)], inverse[(line, 2 * g + 1)]]
            if scheme == 2 or (line, g) == (1, 0):  # (the resilient pattern has runs: some of its groups hit one neuron twice)
                assert sorted(h[0] for h in hit) == [0, 1]
            got = hr.pack_hardened(L, pdir, scheme, [rec9(layer, 1, mem, ind + line, thresh, 2 * g, 2, 0)])
            want = mm.pack_faulty(L, pdir, [rec9(layer, 1, mem, ind + half, thresh, bit, 1, 0)[:8] for half, bit in hit])
            assert (got == want).all(), (line, g)
    if scheme == 3:
        assert sorted([inverse[(1, 0)], inverse[(1, 1)]]) == [(0, 0), (1, 15)]
    # without interleave the same event hits one neuron twice
    assert (hr.pack_hardened(L, pdir, 0, [rec9(layer, 1, mem, ind, thresh, 0, 2, 0)]) ==
            mm.pack_faulty(L, pdir, [rec9(layer, 1, mem, ind, thresh, 0, 2, 0)[:8]])).all()


WHOLE = [(n, s, b) for n, s in PAIRS for b in (1, 4)]


@pytest.mark.parametrize("network,scheme,burst", WHOLE, ids=str)
def test_whole_run_against_the_independent_route(network, scheme, burst, tmp_path):
    """a run's events (the restatement's, which the library's equal) applied by tests/hardened_ref.py to the parameter
    files' words -- interleave, read-modify-write, vote, de-interleave -- and written as a parameter directory:
    pack_params of it is pack_params_hardened of the events.  cnvW2A2: the threshold memories (the route works on memory
    words, and the 1-bit nets cover the weights)."""
    L, pdir = gl.load(network), pdir_of(network)
    w = 0.0 if network == "cnvW2A2" else 2.0 ** -9
    rw = [q32(2.0 ** -4), q32(w)] + [q32(w)] * 7
    if network == "cnvW2A2":
        rw[0] = 0
    rt = [q32(2.0 ** -3)] * 8 + [0]
    recs = hr.run_events(network, scheme, burst, 97, rw, rt)
    assert (hr.lib_run_events(L, network, scheme, burst, 97, rw, rt) == recs).all()
    want, physical, logical = hr.blob_by_the_independent_route(network, scheme, pdir, recs, str(tmp_path / "p"))
    got = hr.pack_hardened(L, pdir, scheme, recs)
    assert (got == want).all()
    assert (got != gl.pack_params(network, pdir)).any()
    assert (physical[:8, 1] > 0).all() and (logical[1:8, 1] > 0).all()
    if scheme == 1:  # the voter removes most of what hits the replicated memories
        assert logical[1:5, 1].sum() < physical[1:5, 1].sum() / 3


def _campaign(L, scheme, burst, runs, seed, rw, rt, n_rates=None, path=b"/nonexistent"):
    up = C.c_uint * max(len(rw), 1)
    cnt = C.c_int(0)
    return L.bnn_mi355x_hardened_mem_noise_campaigns(path, 10, scheme, burst, runs, seed, up(*rw), up(*rt),
                                                     len(rw) if n_rates is None else n_rates, C.byref(cnt), None)


def test_campaign_argument_checks_without_a_gpu(variant_libs):
    """bad arguments return NULL + last_error before any device is touched (the image file does not even exist); a
    variant's library answers the same way (no "not modelled" here: the scheme is the argument)"""
    z, w = [0] * 9, [1 << 20] * 9
    up = C.c_uint * 9
    for name in ("cnvW1A1", "cnvW1A1-TMR"):
        L = gl.load(name)
        for burst in (0, 17, -1):
            assert not _campaign(L, 1, burst, 2, 1, w, z)
            assert b"burst must be 1 ... 16" in L.bnn_mi355x_last_error()
            assert L.bnn_mi355x_hardened_mem_noise_params(1, burst, 1, up(*w), up(*z), 9, None, 0) == 0
            assert b"burst" in L.bnn_mi355x_last_error()
        for scheme in (-1, 4):
            assert not _campaign(L, scheme, 1, 2, 1, w, z)
            assert b"scheme must be" in L.bnn_mi355x_last_error()
        for n_rates in (8, 10, 0):
            assert not _campaign(L, 2, 4, 2, 1, w, z, n_rates=n_rates)
            assert b"n_rates" in L.bnn_mi355x_last_error()
        assert not _campaign(L, 3, 1, 2, 1, z, [0] * 8 + [5])
        assert b"layer 8 has no threshold memory" in L.bnn_mi355x_last_error()
        for runs in (0, 4097):
            assert not _campaign(L, 1, 1, runs, 1, w, z)
            assert b"num_runs" in L.bnn_mi355x_last_error()
        assert not _campaign(L, 1, 1, 2, 1, w, z)  # (nothing wrong with the arguments: no parameters are loaded)
        assert b"load_parameters" in L.bnn_mi355x_last_error()
        assert L.bnn_mi355x_last_hardened_mem_noise_counts(None, 0) == 0 and L.bnn_mi355x_last_hardened_mem_noise_seeds(None, 0) == 0
    L = gl.load("cnvW2A2")
    assert not _campaign(L, 2, 1, 2, 1, w, z)
    assert b"cnvW2A2 with scheme 2" in L.bnn_mi355x_last_error()
    L = gl.load("lfcW1A1")
    assert not _campaign(L, 1, 1, 2, 1, [1] * 4, [0] * 4)
    assert b"LFC" in L.bnn_mi355x_last_error()
