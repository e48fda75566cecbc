"""Plain-Python restatement of the SEC-DED (72,64) coded WEIGHT memories of the exposure campaigns (csrc/wecc.h;
csrc/mem_org.h, "coded weight memories"), on top of tests/hardened_ref.py, exposure_ref.py, ecc_ref.py and repair_ref.py.
Written from the model's text: encode / decode from the positions (not from masks), the code words as runs of 64 sites
in the PE-major site order, the check memory's draw at element width 8 with module 1 in the counter word, and a route
of its own from a marker-and-record stream to the words the network computes with and to the twelve counts: the coded
weight memories are kept code word by code word (64 data bits, 8 check bits) and stepped through events, repairs and
rewrites; everything else goes through repair_ref's route.  Shared by tests/test_wecc_*.py and
tests/test_gpu_wecc_exposure.py."""
import ctypes as C

import numpy as np

import act_noise_ref as ref
import ecc_ref as er
import exposure_ref as xr
import gpu_lib as gl
import hardened_ref as hr
import repair_ref as rr

from bnn import params_io

ip = C.POINTER(C.c_int)
CHECK_POS = (1, 2, 4, 8, 16, 32, 64)
DATA_POS = tuple(p for p in range(1, 72) if p not in CHECK_POS)  # data bit k sits at DATA_POS[k]
assert len(DATA_POS) == 64
M64 = (1 << 64) - 1
U = np.uint64


def parity(v):
    return bin(v).count("1") & 1


def encode(d):
    """the 8 check bits: c_j = XOR of the data bits whose position has bit j set, c7 = XOR of all data bits and c0..c6"""
    bits = [(d >> k) & 1 for k in range(64)]
    c = 0
    for j in range(7):
        c |= (sum(bits[k] for k in range(64) if DATA_POS[k] >> j & 1) & 1) << j
    return c | ((sum(bits) + parity(c)) & 1) << 7


def decode(d, c):
    """-> (status, data)"""
    d, c = d & M64, c & 0xFF
    s = (encode(d) ^ c) & 127
    P = parity(d) ^ parity(c)
    if P == 0:
        return (0, d) if s == 0 else (2, d)
    if s == 0 or s in CHECK_POS:
        return 1, d
    if s in DATA_POS:
        return 1, d ^ (1 << DATA_POS.index(s))
    return 2, d


def repair_word(d, c):
    """what a repair leaves stored of one (data, check) pair -> (status, data, check)"""
    st, out = decode(d, c)
    return (1, out, encode(out)) if st == 1 else (st, d & M64, c & 0xFF)


# ---- the layout ------------------------------------------------------------------------------------------------------------

def coded(network, weight_code, layer):
    """every layer but CNV layer 0"""
    return weight_code == 1 and not (network.startswith("cnv") and layer == 0)


def words_per_pe(network, weight_code, layer):
    if not coded(network, weight_code, layer):
        return 0
    F = params_io.layout(network)[layer]
    eb = hr.ebits(network, layer, 0)
    assert 64 % eb == 0 and (F["wmem"] * eb) % 64 == 0
    return F["wmem"] * eb // 64


def check_events(network, burst, seed, epoch, layer, rate):
    """the weight check memory's records: element q = PE * (code words per PE) + code word, width 8, module 1 of target 0
    in the counter word"""
    F = params_io.layout(network)[layer]
    cwpp = words_per_pe(network, 1, layer)
    per = -(-8 // burst)
    n = F["pe"] * cwpp * per
    word = 0 | 1 << 1 | (burst - 1) << 8
    u = ref.philox4x32_10((layer, word, np.arange((n + 3) // 4), 1 + (epoch << 8)), (seed & 0xFFFFFFFF, seed >> 32)).reshape(-1)[:n]
    e = np.nonzero(u.astype(np.uint64) < np.uint64(rate))[0]
    el, g = e // per, e % per
    rec = np.zeros((len(e), 9), np.int32)
    rec[:, 0], rec[:, 1], rec[:, 2], rec[:, 7], rec[:, 8] = epoch, 0, layer, burst, 1
    rec[:, 4], rec[:, 3], rec[:, 6] = el % cwpp, el // cwpp, g * burst
    return rec


def memories(network, scheme, code, weight_code, only=None):
    """(layer, target, module) in the in-epoch order: layer-major, weights then thresholds, module-major (data, check)"""
    out = []
    for l, t, m in er.memories(network, scheme, code):
        if only is None or only(l, t):
            out.append((l, t, m))
        if t == 0 and coded(network, weight_code, l) and m == er.org(network, scheme, code, l)[0] - 1:
            assert m == 0  # (no scheme gives the weights of these layers a second module)
            if only is None or only(l, t):
                out.append((l, 0, 1))
    return out


def events(network, scheme, code, weight_code, burst, seed, epoch, layer, target, module, rate):
    if target == 0 and module == 1 and coded(network, weight_code, layer):
        return check_events(network, burst, seed, epoch, layer, rate)
    return er.events(network, scheme, code, burst, seed, epoch, layer, target, module, rate)


def epoch_events(network, scheme, code, weight_code, burst, seed, epoch, rw, rt, only=None):
    return {(l, t, m): events(network, scheme, code, weight_code, burst, seed, epoch, l, t, m, (rw, rt)[t][l])
            for l, t, m in memories(network, scheme, code, weight_code, only)}


def flat(epoch):
    return xr.flat(epoch)


# ---- the library ------------------------------------------------------------------------------------------------------------

def lib_encode(L, d):
    return L.bnn_mi355x_wecc_encode(d)


def lib_decode(L, d, c):
    out = C.c_ulonglong(0)
    st = L.bnn_mi355x_wecc_decode(d, c, C.byref(out))
    return st, out.value


def lib_repair(L, d, c):
    od, oc = C.c_ulonglong(0), C.c_uint(0)
    st = L.bnn_mi355x_wecc_repair(d, c, C.byref(od), C.byref(oc))
    return st, od.value, oc.value


def lib_mask(L, scheme, code, weight_code, burst, seed, epoch, layer, target, module, rate, first=0, cap=None):
    total = L.bnn_mi355x_wecc_exposure_mask(scheme, code, weight_code, burst, seed, epoch, layer, target, module, rate, 0, None, 0)
    assert total >= 0, L.bnn_mi355x_last_error()
    cap = max(total - first, 0) if cap is None else cap
    rec = np.zeros((max(cap, 1), 9), np.int32)
    assert L.bnn_mi355x_wecc_exposure_mask(scheme, code, weight_code, burst, seed, epoch, layer, target, module, rate, first, rec.ctypes.data_as(ip),
                                           cap) == total
    return rec[:max(min(cap, total - first), 0)]


def lib_epoch_events(L, network, scheme, code, weight_code, burst, seed, epoch, rw, rt):
    return {(l, t, m): lib_mask(L, scheme, code, weight_code, burst, seed, epoch, l, t, m, (rw, rt)[t][l])
            for l, t, m in memories(network, scheme, code, weight_code)}


def lib_pack(L, pdir, scheme, code, weight_code, recs, expect_error=None):
    flat = np.ascontiguousarray(np.asarray(recs, np.int32).reshape(-1))
    fp = flat.ctypes.data_as(ip)
    n = len(flat) // 9
    size = L.bnn_mi355x_pack_params_wecc(pdir.encode(), scheme, code, weight_code, fp, n, None, 0)
    if expect_error is not None:
        assert size == 0 and expect_error in L.bnn_mi355x_last_error(), L.bnn_mi355x_last_error()
        return None
    assert size > 0, L.bnn_mi355x_last_error()
    blob = np.zeros(size, np.uint8)
    assert L.bnn_mi355x_pack_params_wecc(pdir.encode(), scheme, code, weight_code, fp, n, blob.ctypes.data, size) == size
    return blob


# ---- the independent route -----------------------------------------------------------------------------------------------
# (numpy over all code words of a layer; the masks and the syndrome table come from DATA_POS above, entry by entry)

MASK = [U(sum(1 << k for k in range(64) if DATA_POS[k] >> j & 1)) for j in range(7)]
SYNDROME = [(1, -1) if s == 0 or s in CHECK_POS else (1, DATA_POS.index(s)) if s in DATA_POS else (2, -1) for s in range(128)]
SYN_STATUS = np.array([x[0] for x in SYNDROME], np.int64)
SYN_FLIP = np.array([0 if x[1] < 0 else 1 << x[1] for x in SYNDROME], np.uint64)


def par_all(v):
    v = v.astype(np.uint64).copy()
    for s in (32, 16, 8, 4, 2, 1):
        v ^= v >> U(s)
    return (v & U(1)).astype(np.int64)


def popcount_all(v):
    return int(np.unpackbits(np.ascontiguousarray(v.astype("<u8")).view(np.uint8)).sum())


def encode_all(d):
    c = np.zeros(d.shape, np.int64)
    for j in range(7):
        c |= par_all(d & MASK[j]) << j
    return c | (par_all(d) ^ par_all(c.astype(np.uint64))) << 7


def decode_all(d, c):
    """decode over arrays (d uint64, c int64) -> (status, data)"""
    s = (encode_all(d) ^ c) & 127
    odd = (par_all(d) ^ par_all(c.astype(np.uint64))) == 1
    status = np.where(odd, SYN_STATUS[s], np.where(s == 0, 0, 2))
    return status, np.where(odd, d ^ SYN_FLIP[s], d)


class WCoded:
    """a coded weight memory: data[q] the 64 sites of code word q (bit j: site 64 q + j), check[q] its 8 check bits, q in
    PE-major order"""

    def __init__(self, network, layer, words):
        F = params_io.layout(network)[layer]
        self.network, self.layer, self.F = network, layer, F
        self.eb = hr.ebits(network, layer, 0)
        self.cwpp = words_per_pe(network, 1, layer)
        el = (np.array(words, np.uint64) & U((1 << self.eb) - 1 if self.eb < 64 else M64)).reshape(F["pe"], self.cwpp, 64 // self.eb)
        self.files = np.zeros((F["pe"], self.cwpp), np.uint64)
        for i in range(64 // self.eb):
            self.files |= el[:, :, i] << U(i * self.eb)
        self.files = self.files.reshape(-1)
        self.files_check = encode_all(self.files)
        self.flags = dict(w_status1=False, w_status2=False, w_accepted_triple=False, w_locked=False, w_cleared=False)
        self.rewrite()

    def rewrite(self):
        self.data, self.check = self.files.copy(), self.files_check.copy()

    def apply(self, recs):
        """-> the physical bits flipped (data and check, bursts clipped to the element)"""
        r = np.asarray(recs, np.int64).reshape(-1, 9)
        assert (r[:, 1] == 0).all() and (r[:, 2] == self.layer).all() and np.isin(r[:, 8], (0, 1)).all()
        ids = xr.bit_ids(self.network, r[r[:, 8] == 0], self.layer, 0)
        if len(ids):
            np.bitwise_xor.at(self.data, ids // 64, U(1) << (ids % 64).astype(np.uint64))
        c = r[r[:, 8] == 1]
        at = c[:, 6] // c[:, 7] * c[:, 7]
        flip = (((1 << c[:, 7]) - 1) << at) & 0xFF
        np.bitwise_xor.at(self.check, c[:, 3] * self.cwpp + c[:, 4], flip)
        return len(ids) + int(np.minimum(c[:, 7], 8 - at).sum())

    def repair(self):
        """-> (code words rewritten, code words whose stored state still differs from the loaded one)"""
        status, out = decode_all(self.data, self.check)
        one = status == 1
        self.data = np.where(one, out, self.data)
        self.check = np.where(one, encode_all(out), self.check)
        wrong = (self.data != self.files) | (self.check != self.files_check)
        self.flags["w_locked"] = self.flags["w_locked"] or bool((one & wrong).any())
        self.flags["w_cleared"] = self.flags["w_cleared"] or bool((one & ~wrong).any())
        return int(one.sum()), int(wrong.sum())

    def logical(self):
        """-> (words[pe], delivered data bits that differ, status-1 code words, status-2 code words)"""
        status, out = decode_all(self.data, self.check)
        res = out ^ self.files
        self.flags["w_status1"] = self.flags["w_status1"] or bool((status == 1).any())
        self.flags["w_status2"] = self.flags["w_status2"] or bool((status == 2).any())
        self.flags["w_accepted_triple"] = self.flags["w_accepted_triple"] or bool(((status == 1) & (res != 0)).any())
        o = out.reshape(self.F["pe"], self.cwpp)
        emask = U((1 << self.eb) - 1 if self.eb < 64 else M64)
        el = np.stack([(o >> U(i * self.eb)) & emask for i in range(64 // self.eb)], axis=2).reshape(self.F["pe"], -1)
        return [pe.tolist() for pe in el], popcount_all(res), int((status == 1).sum()), int((status == 2).sum())


def coded_layers(network, weight_code):
    return [l for l in range(len(params_io.layout(network))) if coded(network, weight_code, l)]


def mine(network, weight_code, recs):
    """which records hit a coded weight memory (data or check)"""
    recs = np.asarray(recs).reshape(-1, 9)
    return (recs[:, 1] == 0) & np.isin(recs[:, 2], coded_layers(network, weight_code))


def after(network, scheme, code, weight_code, pdir, recs):
    """-> (w, t) the words the network computes with after a marker-and-record stream"""
    recs = np.asarray(recs, np.int32).reshape(-1, 9)
    m = mine(network, weight_code, recs)
    w, t = rr.after(network, scheme, code, pdir, recs[~m])
    w0, _ = er.file_words(pdir, network)
    for l in coded_layers(network, weight_code):
        mem = WCoded(network, l, w0[l])
        start = 0
        for i in list(np.nonzero(recs[:, 2] < 0)[0]) + [len(recs)]:
            chunk = recs[start:i]
            mem.apply(chunk[(chunk[:, 2] == l) & (chunk[:, 1] == 0)])
            if i < len(recs):
                (mem.repair if recs[i, 2] == rr.REPAIR else mem.rewrite)()
            start = i + 1
        w[l] = mem.logical()[0]
    return w, t


def pack(network, scheme, code, weight_code, pdir, recs, out_dir):
    w, t = after(network, scheme, code, weight_code, pdir, recs)
    hr.write_words(out_dir, network, w, t)
    return gl.pack_params(network, out_dir)


def campaign_counts(network, scheme, code, weight_code, pdir, per_epoch, scrub_every, repair_every):
    """-> ([epoch][layer][12], flags): repair_ref's eight, with the weights' two of a coded layer restated from the stepped
    code words (physical: data plus check bits; logical: the delivered data bits that differ), then the code words at
    status 1 and 2 after the epoch, those the epoch's repair rewrote and those still unlike the loaded ones after it"""
    eight, flags = rr.campaign_counts(network, scheme, code, pdir, per_epoch, scrub_every, repair_every)
    out = np.zeros(eight.shape[:2] + (12,), np.int64)
    out[:, :, :8] = eight
    w0, _ = er.file_words(pdir, network)
    for l in coded_layers(network, weight_code):
        mem = WCoded(network, l, w0[l])
        for t, epoch in enumerate(per_epoch):
            if rr.rewrites(t, scrub_every):
                mem.rewrite()
            elif rr.repairs(t, scrub_every, repair_every):
                out[t, l, 10:12] = mem.repair()
            out[t, l, 0] = mem.apply(np.concatenate([epoch[(l, 0, 0)], epoch[(l, 0, 1)]]))
            _, out[t, l, 1], out[t, l, 8], out[t, l, 9] = mem.logical()
        for k, v in mem.flags.items():
            flags[k + "_%d" % l] = v
    return out, flags


# ---- the GPU test's plan (tests/test_gpu_wecc_exposure.py), here so that the CPU tests can assert what it covers -----------

GPU_RUNS, GPU_IMAGES, GPU_EPOCH_IMAGES, GPU_EPOCHS, GPU_SEED, GPU_RATE = 3, 24, 6, 4, 20261121, 2.0 ** -7
GPU_DATASET = {"cnvW1A1": "cifar10", "cnvW2A2": "cifar10", "lfcW1A1": "mnist", "lfcW1A2": "mnist"}
# (scrub_every, repair_every): never; a repair every epoch; a repair every epoch with a rewrite before epoch 2 in its place;
# a rewrite every epoch
GPU_SCHEDULES = [(0, 0), (0, 1), (2, 1), (1, 0)]
# network -> [(scheme, code, burst)]; CNV layer 0's rates are 0 in the coded-threshold cases
GPU_CASES = {"cnvW1A1": [(0, 0, 1), (1, 0, 2), (0, 1, 1), (2, 1, 2)],
             "cnvW2A2": [(0, 0, 2), (1, 0, 1), (0, 1, 1)],
             "lfcW1A1": [(0, 0, 1), (0, 1, 2)],
             "lfcW1A2": [(0, 0, 2), (0, 1, 1)]}


def gpu_rates(network, code):
    lay = params_io.layout(network)
    q = hr.q32(GPU_RATE)
    rw, rt = [q] * len(lay), [q if F["nthr"] else 0 for F in lay]
    if code == 1 and network.startswith("cnv"):
        rw[0] = rt[0] = 0
    return rw, rt
