"""Plain-Python restatement of the SEC-DED coded threshold memories (csrc/ecc.h; csrc/mem_org.h, "coded threshold
memories"), on top of tests/hardened_ref.py and tests/exposure_ref.py: encode / decode from the definition (positions,
not masks), the check memory's layout and draw, and a route of its own from a list of physical records to a blob and
the six counts: the files' words -> data and check words -> (scheme 2) both interleaved -> the records word by word ->
de-interleaved -> decoded -> files.  The uncoded memories (weights, CNV layer 0, code 0) go through hardened_ref's route.
Shared by tests/test_ecc_code.py, test_ecc_mask.py, test_ecc_pack.py and test_gpu_ecc_exposure.py."""
import ctypes as C

import numpy as np

import act_noise_ref as ref
import exposure_ref as xr
import gpu_lib as gl
import hardened_ref as hr

from bnn import params_io

ip = C.POINTER(C.c_int)
CHECK_POS = (1, 2, 4, 8, 16)
DATA_POS = tuple(p for p in range(1, 22) if p not in CHECK_POS)  # data bit k sits at DATA_POS[k]
SUPPORTED = {"cnvW1A1": (0, 2), "cnvW1A2": (0, 2), "cnvW2A2": (0,), "lfcW1A1": (0,), "lfcW1A2": (0,)}  # schemes with code 1


def parity(v):
    return bin(v).count("1") & 1


def encode(d):
    """the 6 check bits: c_j = XOR of the data bits whose position has bit j set, c5 = XOR of all data bits and c0..c4"""
    bits = [(d >> k) & 1 for k in range(16)]
    c = 0
    for j in range(5):
        c |= (sum(bits[k] for k in range(16) if DATA_POS[k] >> j & 1) & 1) << j
    return c | ((sum(bits) + parity(c)) & 1) << 5


def decode(d, c):
    """-> (status, data)"""
    s = (encode(d) ^ c) & 31
    P = parity(d & 0xFFFF) ^ parity(c & 0x3F)
    if P == 0:
        return (0, d) if s == 0 else (2, d)
    if s == 0 or s in CHECK_POS:
        return 1, d
    if s in DATA_POS:
        return 1, d ^ (1 << DATA_POS.index(s))
    return 2, d


def coded(network, code, layer):
    return code == 1 and hr.ebits(network, layer, 1) == 16


def org(network, scheme, code, layer):
    """-> (weight modules, threshold modules, interleave, check bits)"""
    wm, tm, il = hr.org(network, scheme, layer)
    return (wm, 2, il, 6) if coded(network, code, layer) else (wm, tm, il, 0)


def check_site(il, lines, ind, bit):
    """scheme 2 at width 6: position q of a pair holds bit q // 2 of line ind's word (q even) or of line ind + 1's (q
    odd); line ind stores positions 6 ... 11, line ind + 1 positions 0 ... 5"""
    a = ind & ~1
    if il == 0 or a + 1 >= lines:
        return ind, bit
    q = 2 * bit + (ind - a)
    return (a, q - 6) if q >= 6 else (a + 1, q)


def check_events(network, burst, seed, epoch, layer, rate):
    """the check memory's records: element width 6, module 1 in the counter word"""
    F = params_io.layout(network)[layer]
    per = -(-6 // burst)
    n = F["pe"] * F["tmem"] * F["nthr"] * per
    word = 1 | 1 << 1 | (burst - 1) << 8
    u = ref.philox4x32_10((layer, word, np.arange((n + 3) // 4), 1 + (epoch << 8)), (seed & 0xFFFFFFFF, seed >> 32)).reshape(-1)[:n]
    e = np.nonzero(u.astype(np.uint64) < np.uint64(rate))[0]
    el, g = e // per, e % per
    rec = np.zeros((len(e), 9), np.int32)
    rec[:, 0], rec[:, 1], rec[:, 2], rec[:, 7], rec[:, 8] = epoch, 1, layer, burst, 1
    rec[:, 5], rec[:, 4], rec[:, 3], rec[:, 6] = el % F["nthr"], (el // F["nthr"]) % F["tmem"], el // F["nthr"] // F["tmem"], g * burst
    return rec


def memories(network, scheme, code, only=None):
    """(layer, target, module) in the in-epoch order: layer-major, weights then thresholds, module-major (data, check)"""
    nl = len(params_io.layout(network))
    return [(l, t, m) for l in range(nl) for t in (0, 1) for m in range(org(network, scheme, code, l)[t]) if only is None or only(l, t)]


def events(network, scheme, code, burst, seed, epoch, layer, target, module, rate):
    if target == 1 and module == 1 and coded(network, code, layer):
        return check_events(network, burst, seed, epoch, layer, rate)
    return xr.events(network, burst, seed, epoch, layer, target, module, rate)


def epoch_events(network, scheme, code, burst, seed, epoch, rw, rt, only=None):
    return {(l, t, m): events(network, scheme, code, burst, seed, epoch, l, t, m, (rw, rt)[t][l]) for l, t, m in memories(network, scheme, code, only)}


def lib_mask(L, scheme, code, burst, seed, epoch, layer, target, module, rate, first=0, cap=None):
    total = L.bnn_mi355x_ecc_exposure_mask(scheme, code, burst, seed, epoch, layer, target, module, rate, 0, None, 0)
    assert total >= 0, L.bnn_mi355x_last_error()
    cap = max(total - first, 0) if cap is None else cap
    rec = np.zeros((max(cap, 1), 9), np.int32)
    assert L.bnn_mi355x_ecc_exposure_mask(scheme, code, burst, seed, epoch, layer, target, module, rate, first, rec.ctypes.data_as(ip), cap) == total
    return rec[:max(min(cap, total - first), 0)]


def lib_epoch_events(L, network, scheme, code, burst, seed, epoch, rw, rt):
    return {(l, t, m): lib_mask(L, scheme, code, burst, seed, epoch, l, t, m, (rw, rt)[t][l]) for l, t, m in memories(network, scheme, code)}


def lib_pack(L, pdir, scheme, code, recs):
    flat = np.ascontiguousarray(np.asarray(recs, np.int32).reshape(-1))
    fp = flat.ctypes.data_as(ip)
    n = len(flat) // 9
    size = L.bnn_mi355x_pack_params_ecc(pdir.encode(), scheme, code, fp, n, None, 0)
    assert size > 0, L.bnn_mi355x_last_error()
    blob = np.zeros(size, np.uint8)
    assert L.bnn_mi355x_pack_params_ecc(pdir.encode(), scheme, code, fp, n, blob.ctypes.data, size) == size
    return blob


# ---- the independent route ---------------------------------------------------------------------------------------------
# (numpy over all words of a layer; the tables below come from encode / decode above, entry by entry)

ENC = np.array([encode(d) for d in range(1 << 16)], np.int64)
PAR = np.array([parity(v) for v in range(1 << 16)], np.int64)
# syndrome s with odd overall parity -> (status, the data bit to flip or -1)
SYNDROME = [(1, -1) if s == 0 or s in CHECK_POS else (1, DATA_POS.index(s)) if s in DATA_POS else (2, -1) for s in range(32)]
SYN_STATUS = np.array([x[0] for x in SYNDROME], np.int64)
SYN_FLIP = np.array([0 if x[1] < 0 else 1 << x[1] for x in SYNDROME], np.int64)


def decode_all(d, c):
    """decode over arrays -> (status, data)"""
    s = (ENC[d] ^ c) & 31
    odd = (PAR[d] ^ PAR[c]) == 1
    status = np.where(odd, SYN_STATUS[s], np.where(s == 0, 0, 2))
    return status, np.where(odd, d ^ SYN_FLIP[s], d)


def interleave2(x, T, forward):
    """scheme 2 over threshold words [pe][line][threshold] at width T: position q of the pair (line a, line a + 1) holds
    bit q // 2 of line a's word for even q, of line a + 1's for odd q; line a stores positions T ... 2T-1, line a + 1 the
    rest; an odd last line stays as it is"""
    out = x.copy()
    pairs = x.shape[1] // 2 * 2
    a, b = x[:, 0:pairs:2] & ((1 << T) - 1), x[:, 1:pairs:2] & ((1 << T) - 1)
    if forward:
        v = sum(((a >> k) & 1) << (2 * k) | ((b >> k) & 1) << (2 * k + 1) for k in range(T))
        out[:, 0:pairs:2], out[:, 1:pairs:2] = v >> T, v & ((1 << T) - 1)
    else:
        v = a << T | b
        out[:, 0:pairs:2] = sum(((v >> (2 * k)) & 1) << k for k in range(T))
        out[:, 1:pairs:2] = sum(((v >> (2 * k + 1)) & 1) << k for k in range(T))
    return out


def coded_layer(network, scheme, layer, words, recs):
    """one coded layer.  words[pe]: the file's threshold words; recs: its threshold records (modules 0 and 1) in order.
    -> (logical words[pe], physical bits flipped, logical data bits that differ, words with status 1, with status 2,
    per-word [status, residual data mask, data hit mask, check hit mask] in (pe, line, threshold) order)"""
    F = params_io.layout(network)[layer]
    il = hr.org(network, scheme, layer)[2]
    assert il in (0, 2)
    shape = (F["pe"], F["tmem"], F["nthr"])
    files = (np.array(words, np.uint64) & np.uint64(0xFFFF)).astype(np.int64).reshape(shape)
    data, check = files.copy(), ENC[files]
    if il:
        data, check = interleave2(data, 16, True), interleave2(check, 6, True)
    loaded = (data.copy(), check.copy())
    r = np.asarray(recs, np.int64).reshape(-1, 9)
    assert (r[:, 1] == 1).all() and (r[:, 2] == layer).all() and np.isin(r[:, 8], (0, 1)).all()
    width = np.where(r[:, 8] == 1, 6, 16)
    at = r[:, 6] // r[:, 7] * r[:, 7]
    flip = (((1 << r[:, 7]) - 1) << at) & ((1 << width) - 1)
    physical = int(np.minimum(r[:, 7], width - at).sum())
    for m, mem in ((0, data), (1, check)):
        k = r[:, 8] == m
        np.bitwise_xor.at(mem, (r[k, 3], r[k, 4], r[k, 5]), flip[k])
    hit = [data ^ loaded[0], check ^ loaded[1]]
    if il:
        data, check = interleave2(data, 16, False), interleave2(check, 6, False)
        hit = [interleave2(hit[0], 16, False), interleave2(hit[1], 6, False)]
    status, out = decode_all(data, check)
    residual = out ^ files
    logical = int(sum(bin(v).count("1") for v in residual.reshape(-1).tolist() if v))
    detail = np.stack([status.reshape(-1), residual.reshape(-1), hit[0].reshape(-1), hit[1].reshape(-1)], axis=1)
    return [pe.reshape(-1).tolist() for pe in out], physical, logical, int((status == 1).sum()), int((status == 2).sum()), detail


def after(network, scheme, code, pdir, recs):
    """-> (w, t, counts [layer][6], detail {coded layer: per-word tuples}) after the physical records, in order"""
    recs = np.asarray(recs, np.int32).reshape(-1, 9)
    lay = params_io.layout(network)
    mine = np.array([r[1] == 1 and coded(network, code, r[2]) for r in recs.tolist()], bool)
    w, t, physical, logical = hr.logical_after(network, scheme, pdir, recs[~mine])
    _, t0 = hr.read_words(pdir, network)
    counts = np.zeros((len(lay), 6), np.int64)
    counts[:, 0], counts[:, 1], counts[:, 2], counts[:, 3] = physical[:, 0], logical[:, 0], physical[:, 1], logical[:, 1]
    detail = {}
    for l in range(len(lay)):
        if coded(network, code, l):
            t[l], counts[l, 2], counts[l, 3], counts[l, 4], counts[l, 5], detail[l] = coded_layer(network, scheme, l, t0[l], recs[mine & (recs[:, 2] == l)])
    return w, t, counts, detail


def pack(network, scheme, code, pdir, recs, out_dir):
    """-> (blob, counts [layer][6], detail)"""
    w, t, counts, detail = after(network, scheme, code, pdir, recs)
    hr.write_words(out_dir, network, w, t)
    return gl.pack_params(network, out_dir), counts, detail


def flat(epoch):
    return xr.flat(epoch)


def since_scrub(per_epoch, t, scrub_every):
    return xr.since_scrub(per_epoch, t, scrub_every)


_files = {}


def file_words(pdir, network):
    if (pdir, network) not in _files:
        _files[(pdir, network)] = hr.read_words(pdir, network)
    return _files[(pdir, network)]


def coded_after(network, scheme, pdir, epochs, layer):
    """coded_layer for one layer after the given epochs' records ({(layer, target, module): records} each), epoch-major,
    data then check inside an epoch"""
    recs = [np.zeros((0, 9), np.int32)] + [e[(layer, 1, m)] for e in epochs for m in (0, 1)]
    return coded_layer(network, scheme, layer, file_words(pdir, network)[1][layer], np.concatenate(recs))


def implied_counts(network, scheme, code, pdir, per_epoch, t, scrub_every):
    """[layer][6] of epoch t from the masks.  The uncoded memories: exposure_ref.implied_counts.  A coded layer's
    thresholds: physical, the bits of the epoch's own data and check events; logical and the decode status, after the
    records since the last scrub"""
    out = np.zeros((len(params_io.layout(network)), 6), np.int64)
    out[:, :4] = xr.implied_counts(network, scheme, pdir, per_epoch, t, scrub_every).reshape(-1, 4)
    for l in range(len(out)):
        if coded(network, code, l):
            out[l, 2] = coded_after(network, scheme, pdir, [per_epoch[t]], l)[1]
            out[l, 3:6] = coded_after(network, scheme, pdir, per_epoch[xr.first_epoch(t, scrub_every): t + 1], l)[2:5]
    return out


def word_hits(network, scheme, pdir, per_epoch, layer):
    """[epoch][word] the 22-bit hit mask (data bits 0 ... 15, check bits 16 ... 21) each epoch's events alone leave on each
    code word of a coded layer, in logical-image order (de-interleaved)"""
    return np.array([(lambda d: d[:, 2] | d[:, 3] << 16)(coded_after(network, scheme, pdir, [e], layer)[5]) for e in per_epoch], np.int64)


def reaches_partner(scheme, recs):
    """scheme 2: does an event of a data or check memory flip a bit of the partner line's code word?  Position q = bit +
    (T for the even line) of the pair belongs to the even line's word for even q, to the odd line's for odd q"""
    for _, _, _, _, ind, _, bit, ws, module in np.asarray(recs).reshape(-1, 9).tolist():
        T = 6 if module else 16
        for b in range(bit, min(bit + ws, T)):
            if scheme == 2 and ((b + (T if ind % 2 == 0 else 0)) & 1) != (ind & 1):
                return True
    return False
