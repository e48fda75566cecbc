"""Plain-Python restatement of the hardened memory organisation and its upset model (csrc/mem_org.h), shared by
tests/test_hardened_mem_noise.py and tests/test_gpu_hardened_mem_noise.py: the tables, the interleave formula as the
header states it (walking the pattern, where the library searches it), the draw (tests/act_noise_ref.py's Philox), and a
route of its own from a run's events to a parameter directory: interleave the files' words, apply the events word by
word, vote, de-interleave, write files."""
import ctypes as C
import os

import numpy as np

import act_noise_ref as ref
import gpu_lib as gl

from bnn import params_io

ip = C.POINTER(C.c_int)
SUPPORTED = {"cnvW1A1": (1, 2, 3), "cnvW1A2": (1, 2, 3), "cnvW2A2": (1, 3)}
PATTERN = {(2, 16): 0x55555555, (2, 24): 0x555555555555, (3, 16): 0b10001000101010101010101011101110,
           (3, 24): 0b100010001000101010101010101010101010111011101110}
M64 = (1 << 64) - 1


def q32(p):
    return int(np.floor(p * 4294967296.0))


def org(network, scheme, layer):
    """-> (weight modules, threshold modules, threshold interleave)"""
    nthr = params_io.layout(network)[layer]["nthr"]
    if scheme == 1:
        return (3 if layer == 0 else 1), (3 if layer <= 4 and nthr else 1), 0
    return 1, 1, (scheme if scheme in (2, 3) and nthr else 0)


def ebits(network, layer, target):
    F = params_io.layout(network)[layer]
    if target == 0:
        return F["simd"] * F["wbits"]
    return 0 if F["nthr"] == 0 else (24 if layer == 0 and network.startswith("cnv") else 16)


def pair_table(il, T):
    """position q of a pair -> (element 0 / 1, its bit): e1's bit o1[popcount(pattern[0..q))] where pattern[q] is set,
    else e2's bit o2[q - popcount]; o1 the identity, o2 the identity (2) or reversed (3)"""
    pat, ones, out = PATTERN[(il, T)], 0, []
    for q in range(2 * T):
        if (pat >> q) & 1:
            out.append((0, ones))
            ones += 1
        else:
            j = q - ones
            out.append((1, j if il == 2 else T - 1 - j))
    return out


def site(il, T, lines, ind, bit):
    """logical (line, bit) -> physical (line, bit): line ind stores positions T ... 2T-1, line ind + 1 positions 0 ... T-1"""
    a = ind & ~1
    if il == 0 or a + 1 >= lines:
        return ind, bit
    q = pair_table(il, T).index((ind - a, bit))
    return (a, q - T) if q >= T else (a + 1, q)


def events(network, burst, seed, layer, target, module, rate):
    """the 9-int physical records of one (layer, target, module) in event order, from the draw's own statement"""
    F = params_io.layout(network)[layer]
    eb = ebits(network, layer, target)
    if eb == 0:
        return np.zeros((0, 9), np.int32)
    per = -(-eb // burst)
    inds, thr = (F["wmem"], 1) if target == 0 else (F["tmem"], F["nthr"])
    n = F["pe"] * inds * thr * per
    word = target | module << 1 | (burst - 1) << 8
    u = ref.philox4x32_10((layer, word, np.arange((n + 3) // 4), 1), (seed & 0xFFFFFFFF, seed >> 32)).reshape(-1)[:n]
    e = np.nonzero(u.astype(np.uint64) < np.uint64(rate))[0]
    el, g = e // per, e % per
    rec = np.zeros((len(e), 9), np.int32)
    rec[:, 1], rec[:, 2], rec[:, 7], rec[:, 8] = target, layer, burst, module
    rec[:, 5], rec[:, 4], rec[:, 3], rec[:, 6] = el % thr, (el // thr) % inds, el // thr // inds, g * burst
    return rec


def run_events(network, scheme, burst, seed, rw, rt):
    """a run's records: layer-major, weights then thresholds, module-major, event order"""
    out = [np.zeros((0, 9), np.int32)]
    for l in range(len(rw)):
        for target in (0, 1):
            for m in range(org(network, scheme, l)[target]):
                out.append(events(network, burst, seed, l, target, m, (rw, rt)[target][l]))
    return np.concatenate(out)


def lib_mask(L, scheme, burst, seed, layer, target, module, rate, first=0, cap=None):
    total = L.bnn_mi355x_hardened_mem_noise_mask(scheme, burst, seed, layer, target, module, rate, 0, None, 0)
    assert total >= 0, L.bnn_mi355x_last_error()
    cap = max(total - first, 0) if cap is None else cap
    rec = np.zeros((max(cap, 1), 9), np.int32)
    assert L.bnn_mi355x_hardened_mem_noise_mask(scheme, burst, seed, layer, target, module, rate, first, rec.ctypes.data_as(ip), cap) == total
    return rec[:max(min(cap, total - first), 0)]


def lib_run_events(L, network, scheme, burst, seed, rw, rt):
    out = [np.zeros((0, 9), np.int32)]
    for l in range(len(rw)):
        lay = (C.c_int * 3)()
        assert L.bnn_mi355x_hardening_layout(scheme, l, lay) == 0
        for target in (0, 1):
            for m in range(lay[target]):
                out.append(lib_mask(L, scheme, burst, seed, l, target, m, (rw, rt)[target][l]))
    return np.concatenate(out)


def pack_hardened(L, pdir, scheme, recs):
    flat = np.ascontiguousarray(np.asarray(recs, np.int32).reshape(-1))
    fp = flat.ctypes.data_as(ip)
    n = len(flat) // 9
    size = L.bnn_mi355x_pack_params_hardened(pdir.encode(), scheme, fp, n, None, 0)
    assert size > 0, L.bnn_mi355x_last_error()
    blob = np.zeros(size, np.uint8)
    assert L.bnn_mi355x_pack_params_hardened(pdir.encode(), scheme, fp, n, blob.ctypes.data, size) == size
    return blob


# ---- the independent route: files -> physical words -> events -> vote -> de-interleave -> files ------------------------

def read_words(pdir, network):
    """-> (w[l][pe], t[l][pe]): lists of Python ints, the files' 64-bit words"""
    w, t = [], []
    for l, F in enumerate(params_io.layout(network)):
        w.append([np.fromfile(os.path.join(pdir, "%d-%d-weights.bin" % (l, p)), "<u8").tolist() for p in range(F["pe"])])
        t.append([np.fromfile(os.path.join(pdir, "%d-%d-thres.bin" % (l, p)), "<u8").tolist() if F["nthr"] else [] for p in range(F["pe"])])
    return w, t


def write_words(directory, network, w, t):
    os.makedirs(directory, exist_ok=True)
    for l, F in enumerate(params_io.layout(network)):
        for p in range(F["pe"]):
            np.array(w[l][p], "<u8").tofile(os.path.join(directory, "%d-%d-weights.bin" % (l, p)))
            if F["nthr"]:
                np.array(t[l][p], "<u8").tofile(os.path.join(directory, "%d-%d-thres.bin" % (l, p)))


def permute(words, F, il, T, forward):
    """interleave (forward) or de-interleave the threshold words of one PE; words: a list of ints"""
    out = list(words)
    if il == 0:
        return out
    tab = pair_table(il, T)
    for a in range(0, F["tmem"] - 1, 2):
        for i in range(F["nthr"]):
            e = [words[a * F["nthr"] + i], words[(a + 1) * F["nthr"] + i]]
            if forward:
                v = 0
                for q, (which, bit) in enumerate(tab):
                    v |= ((e[which] >> bit) & 1) << q
                res = [v >> T, v & ((1 << T) - 1)]
            else:
                v = ((e[0] & ((1 << T) - 1)) << T) | (e[1] & ((1 << T) - 1))
                res = [0, 0]
                for q, (which, bit) in enumerate(tab):
                    res[which] |= ((v >> q) & 1) << bit
            out[a * F["nthr"] + i], out[(a + 1) * F["nthr"] + i] = res
    return out


def sext(v, bits):
    v &= (1 << bits) - 1
    return v - (1 << bits) if v >> (bits - 1) else v


def logical_after(network, scheme, pdir, recs, only=None):
    """-> (w, t, physical[l][target], logical[l][target]): the words the network computes with after the physical
    records, the bits the events flipped (clipped to the element) and the element bits that differ from the files'.
    only: the layers to work on (the others' entries are None; records of other layers must not be given)"""
    lay = params_io.layout(network)
    w0, t0 = read_words(pdir, network)
    phys_w, phys_t = [], []
    for l, F in enumerate(lay):
        if only is not None and l not in only:
            phys_w.append(None)
            phys_t.append(None)
            continue
        wm, tm, il = org(network, scheme, l)
        T = ebits(network, l, 1)
        phys_w.append([[list(x) for x in w0[l]] for _ in range(wm)])
        phys_t.append([[permute(x, F, il, T, True) for x in t0[l]] for _ in range(tm)])
    physical = np.zeros((len(lay), 2), np.int64)
    for _, target, l, mem, ind, thresh, bit, ws, module in np.asarray(recs).reshape(-1, 9).tolist():
        F, eb = lay[l], ebits(network, l, target)
        flip = ((1 << ws) - 1) << (bit // ws * ws)
        physical[l, target] += min(ws, eb - bit // ws * ws)
        if target == 0:
            x = phys_w[l][module][mem]
            x[ind] = ((x[ind] & ((1 << eb) - 1)) ^ flip) & ((1 << eb) - 1)
        else:
            x = phys_t[l][module][mem]
            k = ind * F["nthr"] + thresh
            v = sext(x[k], 24) >> 8 if eb == 24 else sext(x[k], 16)  # (layer 0 is read back as its integer part)
            x[k] = (v ^ flip) & M64
    maj = lambda a, b, c, eb: ((a & b) | (a & c) | (b & c)) & ((1 << eb) - 1)
    w, t = [], []
    logical = np.zeros((len(lay), 2), np.int64)
    for l, F in enumerate(lay):
        if phys_w[l] is None:
            w.append(None)
            t.append(None)
            continue
        wm, tm, il = org(network, scheme, l)
        ew, T = ebits(network, l, 0), ebits(network, l, 1)
        w.append([[maj(*x, ew) for x in zip(*[phys_w[l][m][p] for m in range(3)])] if wm == 3 else phys_w[l][0][p] for p in range(F["pe"])])
        tv = [[maj(*x, T) for x in zip(*[phys_t[l][m][p] for m in range(3)])] if tm == 3 else phys_t[l][0][p] for p in range(F["pe"])]
        t.append([permute(x, F, il, T, False) for x in tv])
        for p in range(F["pe"]):
            logical[l, 0] += sum(bin((a ^ b) & ((1 << ew) - 1)).count("1") for a, b in zip(w[l][p], w0[l][p]))
            if T:
                logical[l, 1] += sum(bin((a ^ b) & ((1 << T) - 1)).count("1") for a, b in zip(t[l][p], t0[l][p]))
    return w, t, physical, logical


def blob_by_the_independent_route(network, scheme, pdir, recs, out_dir):
    w, t, physical, logical = logical_after(network, scheme, pdir, recs)
    write_words(out_dir, network, w, t)
    return gl.pack_params(network, out_dir), physical, logical
