"""Plain-Python restatement of the COLUMN-INTERLEAVED coded weight memories of the exposure campaigns (csrc/mem_org.h,
"column-interleaved code words"), on top of tests/wecc_ref.py.  Written from the model's text, not from the C++:
  depth     D = gcd(16, code words per PE) per coded layer (an odd count: 1); weight_interleave 0: 1
  group G   D consecutive code words' worth of storage in the site order: data sites [64 D G, 64 D (G + 1)), check elements
            [D G, D (G + 1)), 8 bits each
  data      the site at offset p of the group is data bit p // D of code word p % D of the group
  check     the bit at offset r = 8 * element + bit of the group's check elements is check bit r // D of code word r % D
The physical memories are kept as they are stored (64 sites to a word, 8 check bits to an element), take wecc_ref's events
unchanged, and are gathered into code words (numpy reshapes of the bit arrays, nothing cleverer) for wecc_ref's decode_all /
encode_all; corrections and repairs are scattered back.  Shared by tests/test_iwecc_*.py and tests/test_gpu_iwecc_exposure.py."""
import ctypes as C
from math import gcd

import numpy as np

import ecc_ref as er
import exposure_ref as xr
import gpu_lib as gl
import hardened_ref as hr
import repair_ref as rr
import wecc_ref as wr

from bnn import params_io

ip = C.POINTER(C.c_int)
U = np.uint64
MAX_BURST = 16


def depth(network, weight_code, weight_interleave, layer):
    """0 not coded, 1 coded and not interleaved"""
    cwpp = wr.words_per_pe(network, weight_code, layer)
    if not cwpp:
        return 0
    return gcd(MAX_BURST, cwpp) if weight_interleave == 1 and cwpp % 2 == 0 else 1


def member(D, offset):
    """offset p (data) or r (check) of a group -> (code word of the group, bit of the code word)"""
    return offset % D, offset // D


def site_of(network, weight_interleave, layer, module, index):
    """a data site (module 0) or a check bit 8 * element + bit (module 1) -> (code word of the layer, bit)"""
    D = depth(network, 1, weight_interleave, layer)
    per = (64, 8)[module] * D
    w, b = member(D, index % per)
    return index // per * D + w, b


def bits_of(words, width):
    """[n] words -> [n, width] bits, bit 0 first"""
    w = np.ascontiguousarray(np.asarray(words).astype("<u8" if width == 64 else np.uint8))
    return np.unpackbits(w.view(np.uint8), bitorder="little").reshape(-1, width)


def words_of(bits):
    """[n, width] bits -> [n] uint64"""
    packed = np.packbits(np.ascontiguousarray(bits), axis=1, bitorder="little")
    return (packed.view("<u8") if bits.shape[1] == 64 else packed).reshape(-1).astype(np.uint64)


def gather(phys, width, D):
    """physical words ([n] of `width` bits: 64-site words, or 8-bit check elements) -> the code words' bits, [n] words"""
    # a group's offsets p = bit * D + word: [group, bit, word] -> [group, word, bit]
    b = bits_of(phys, width).reshape(-1, width, D)
    return words_of(b.transpose(0, 2, 1).reshape(-1, width))


def scatter(code, width, D):
    b = bits_of(code, width).reshape(-1, D, width)
    return words_of(b.transpose(0, 2, 1).reshape(-1, width))


class IWCoded(wr.WCoded):
    """a coded weight memory at interleave depth D: data[q] the 64 physical sites [64 q, 64 q + 64), check[q] the 8 bits of
    check element q -- wecc_ref's storage and events (apply) as they are; the code words are gathered from them"""

    def __init__(self, network, layer, words, weight_interleave=1, track=False):
        """track: also keep the flags that need the epoch's single events (w_burst_in_words, w_elsewhere)"""
        super().__init__(network, layer, words)
        self.track = track
        self.D = depth(network, 1, weight_interleave, layer)
        assert self.cwpp % self.D == 0  # no group straddles PEs
        self.files_check = scatter(wr.encode_all(gather(self.files, 64, self.D)), 8, self.D).astype(np.int64)
        self.flags.update(w_burst_in_words=False, w_elsewhere=False)
        self.touched = np.zeros(len(self.files), bool)
        self.bursts = []
        self.rewrite()

    def apply(self, recs):
        """wecc_ref's; remembers the epoch's data events for the flags"""
        if self.track:
            r = np.asarray(recs, np.int64).reshape(-1, 9)
            d = r[r[:, 8] == 0]
            self.touched[:] = False
            self.touched[xr.bit_ids(self.network, d, self.layer, 0) // 64] = True
            self.bursts = [xr.bit_ids(self.network, d[i:i + 1], self.layer, 0) for i in range(len(d)) if d[i, 7] > 1]
        return super().apply(recs)

    def words(self):
        """-> (data, check) of every code word"""
        return gather(self.data, 64, self.D), gather(self.check, 8, self.D).astype(np.int64)

    def repair(self):
        d, c = self.words()
        fd, fc = gather(self.files, 64, self.D), gather(self.files_check, 8, self.D).astype(np.int64)
        status, out = wr.decode_all(d, c)
        one = status == 1
        d, c = np.where(one, out, d), np.where(one, wr.encode_all(out), c)
        wrong = (d != fd) | (c != fc)
        self.data, self.check = scatter(d, 64, self.D), scatter(c, 8, self.D).astype(np.int64)
        self.flags["w_locked"] = self.flags["w_locked"] or bool((one & wrong).any())
        self.flags["w_cleared"] = self.flags["w_cleared"] or bool((one & ~wrong).any())
        return int(one.sum()), int(wrong.sum())

    def logical(self):
        """-> (words[pe], delivered data bits that differ, status-1 code words, status-2 code words): per code word"""
        d, c = self.words()
        status, out = wr.decode_all(d, c)
        delivered = scatter(out, 64, self.D)
        res = delivered ^ self.files
        fixed = scatter(out ^ d, 64, self.D) if self.track else None  # the corrected bits, at their sites
        self.flags["w_status1"] = self.flags["w_status1"] or bool((status == 1).any())
        self.flags["w_status2"] = self.flags["w_status2"] or bool((status == 2).any())
        self.flags["w_accepted_triple"] = self.flags["w_accepted_triple"] or bool(((status == 1) & ((out ^ gather(self.files, 64, self.D)) != 0)).any())
        if self.track:
            self.flags["w_elsewhere"] = self.flags["w_elsewhere"] or bool(((fixed != 0) & ~self.touched).any())
        for ids in self.bursts if self.track else ():  # a burst whose bits were corrected in two or more different code words
            hit = [s for s in ids if (int(fixed[s // 64]) >> int(s % 64)) & 1]
            if len({site_of(self.network, 1, self.layer, 0, int(s))[0] for s in hit}) >= 2 and self.D > 1:
                self.flags["w_burst_in_words"] = True
        o = delivered.reshape(self.F["pe"], self.cwpp)
        emask = U((1 << self.eb) - 1 if self.eb < 64 else wr.M64)
        el = np.stack([(o >> U(i * self.eb)) & emask for i in range(64 // self.eb)], axis=2).reshape(self.F["pe"], -1)
        return [pe.tolist() for pe in el], wr.popcount_all(res), int((status == 1).sum()), int((status == 2).sum())


def after(network, scheme, code, weight_code, weight_interleave, pdir, recs):
    """-> (w, t) the words the network computes with after a marker-and-record stream (wecc_ref.after with IWCoded)"""
    recs = np.asarray(recs, np.int32).reshape(-1, 9)
    m = wr.mine(network, weight_code, recs)
    w, t = rr.after(network, scheme, code, pdir, recs[~m])
    w0, _ = er.file_words(pdir, network)
    for l in wr.coded_layers(network, weight_code):
        mem = IWCoded(network, l, w0[l], weight_interleave)
        start = 0
        for i in list(np.nonzero(recs[:, 2] < 0)[0]) + [len(recs)]:
            chunk = recs[start:i]
            mem.apply(chunk[(chunk[:, 2] == l) & (chunk[:, 1] == 0)])
            if i < len(recs):
                (mem.repair if recs[i, 2] == rr.REPAIR else mem.rewrite)()
            start = i + 1
        w[l] = mem.logical()[0]
    return w, t


def pack(network, scheme, code, weight_code, weight_interleave, pdir, recs, out_dir):
    w, t = after(network, scheme, code, weight_code, weight_interleave, pdir, recs)
    hr.write_words(out_dir, network, w, t)
    return gl.pack_params(network, out_dir)


def campaign_counts(network, scheme, code, weight_code, weight_interleave, pdir, per_epoch, scrub_every, repair_every):
    """-> ([epoch][layer][12], flags): wecc_ref.campaign_counts with the coded layers stepped as IWCoded"""
    eight, flags = rr.campaign_counts(network, scheme, code, pdir, per_epoch, scrub_every, repair_every)
    out = np.zeros(eight.shape[:2] + (12,), np.int64)
    out[:, :, :8] = eight
    w0, _ = er.file_words(pdir, network)
    for l in wr.coded_layers(network, weight_code):
        mem = IWCoded(network, l, w0[l], weight_interleave)
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


# ---- the library ------------------------------------------------------------------------------------------------------------

def lib_layout(L, weight_code, weight_interleave, layer):
    out = (C.c_int * 4)()
    assert L.bnn_mi355x_iwecc_layout(weight_code, weight_interleave, layer, out) == 0, L.bnn_mi355x_last_error()
    return list(out)


def lib_site(L, weight_code, weight_interleave, layer, module, index):
    out = (C.c_long * 2)()
    assert L.bnn_mi355x_iwecc_site(weight_code, weight_interleave, layer, module, index, out) == 0, L.bnn_mi355x_last_error()
    return out[0], out[1]


def lib_pack(L, pdir, scheme, code, weight_code, weight_interleave, recs, expect_error=None):
    flat = np.ascontiguousarray(np.asarray(recs, np.int32).reshape(-1))
    fp = flat.ctypes.data_as(ip)
    n = len(flat) // 9
    size = L.bnn_mi355x_pack_params_iwecc(pdir.encode(), scheme, code, weight_code, weight_interleave, fp, n, None, 0)
    if expect_error is not None:
        assert size == 0 and expect_error in L.bnn_mi355x_last_error(), L.bnn_mi355x_last_error()
        return None
    assert size > 0, L.bnn_mi355x_last_error()
    blob = np.zeros(size, np.uint8)
    assert L.bnn_mi355x_pack_params_iwecc(pdir.encode(), scheme, code, weight_code, weight_interleave, fp, n, blob.ctypes.data, size) == size
    return blob


# ---- the GPU test's plan (tests/test_gpu_iwecc_exposure.py): wecc_ref's shape, the issue's cases ------------------------------
# network -> [(scheme, code, burst)]; CNV layer 0's rates are 0 in the coded-threshold cases (wecc_ref.gpu_rates)
GPU_CASES = {"cnvW1A1": [(1, 0, 1), (1, 0, 2), (1, 0, 4), (2, 1, 1), (2, 1, 2), (2, 1, 4)],
             "cnvW2A2": [(0, 1, 2), (0, 1, 4)],
             "lfcW1A1": [(0, 1, 2)],
             "lfcW1A2": [(0, 0, 4)]}
