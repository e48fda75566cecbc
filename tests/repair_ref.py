"""Plain-Python restatement of the repair scrubs of the exposure campaigns (csrc/mem_org.h, "repair scrubs"; csrc/ecc.h),
on top of tests/hardened_ref.py, exposure_ref.py and ecc_ref.py.  A route of its own from the files' words: the PHYSICAL
state of every memory that has redundancy (three modules; data and check words, interleaved under scheme 2) is kept
word by word and stepped through events, repair markers (vote / de-interleave, decode, write back, re-interleave) and
rewrite markers; the memories without redundancy -- which a repair never touches -- go through hardened_ref's route
with the records since the last rewrite.  From it: the blob after any marker-and-record stream, and the eight counts of
(run, epoch, layer).  Shared by tests/test_repair_pack.py and tests/test_gpu_repair_exposure.py."""
import ctypes as C

import numpy as np

import ecc_ref as er
import exposure_ref as xr
import gpu_lib as gl
import hardened_ref as hr

from bnn import params_io

ip = C.POINTER(C.c_int)
REPAIR, REWRITE = -1, -2
# (network, scheme, code) with a defined layout: every scheme of hardened_ref without a code, ecc_ref's pairs with code 1
SUPPORTED = [(n, s, 0) for n in ("cnvW1A1", "cnvW1A2", "cnvW2A2", "lfcW1A1", "lfcW1A2") for s in (0,) + tuple(hr.SUPPORTED.get(n, ()))] + \
            [(n, s, 1) for n, ss in sorted(er.SUPPORTED.items()) for s in ss]


def marker(kind):
    rec = np.zeros((1, 9), np.int32)
    rec[0, 2] = kind
    return rec


def rewrites(t, scrub_every):
    return t > 0 and scrub_every > 0 and t % scrub_every == 0


def repairs(t, scrub_every, repair_every):
    return t > 0 and repair_every > 0 and t % repair_every == 0 and not rewrites(t, scrub_every)


def stream(per_epoch, t, scrub_every, repair_every):
    """the records the blob of epoch t is pack_params_repair of: over epochs 0 ... t, [the epoch's marker, if one is due]
    + the epoch's records in the in-epoch order"""
    out = [np.zeros((0, 9), np.int32)]
    for k in range(t + 1):
        if rewrites(k, scrub_every):
            out.append(marker(REWRITE))
        elif repairs(k, scrub_every, repair_every):
            out.append(marker(REPAIR))
        out.append(xr.flat(per_epoch[k]))
    return np.concatenate(out)


def lib_repair(L, d, c):
    od, oc = C.c_uint(0), C.c_uint(0)
    st = L.bnn_mi355x_ecc_repair(d, c, C.byref(od), C.byref(oc))
    return st, od.value, oc.value


def lib_pack(L, pdir, scheme, code, recs, expect_error=None):
    flat = np.ascontiguousarray(np.asarray(recs, np.int32).reshape(-1))
    fp = flat.ctypes.data_as(ip)
    n = len(flat) // 9
    size = L.bnn_mi355x_pack_params_repair(pdir.encode(), scheme, code, fp, n, None, 0)
    if expect_error is not None:
        assert size == 0 and expect_error in L.bnn_mi355x_last_error(), L.bnn_mi355x_last_error()
        return None
    assert size > 0, L.bnn_mi355x_last_error()
    blob = np.zeros(size, np.uint8)
    assert L.bnn_mi355x_pack_params_repair(pdir.encode(), scheme, code, fp, n, blob.ctypes.data, size) == size
    return blob


def repair_word(d, c):
    """what a repair leaves stored of one (data, check) pair -> (status, data, check)"""
    st, out = er.decode(d & 0xFFFF, c & 0x3F)
    return (1, out, er.encode(out)) if st == 1 else (st, d & 0xFFFF, c & 0x3F)


def sext(x, bits):
    x = x & ((1 << bits) - 1)
    return (x ^ (1 << (bits - 1))) - (1 << (bits - 1))


def maj(a, b, c):
    return (a & b) | (a & c) | (b & c)


class Voted:
    """a memory with three modules: words[m][pe][k] (int64; the 24-bit thresholds of CNV layer 0 keep their whole word,
    which an event rewrites as the integer part), k = ind for weights, ind * nthr + thresh for thresholds"""

    def __init__(self, words, ebits, nthr, quirk):
        self.loaded = np.stack([np.array(words, np.uint64).view(np.int64)] * 3)
        if not quirk:
            self.loaded &= (1 << ebits) - 1
        self.ebits, self.nthr, self.quirk, self.emask = ebits, max(nthr, 1), quirk, (1 << ebits) - 1
        self.rewrite()

    def rewrite(self):
        self.x = self.loaded.copy()

    def apply(self, recs):
        r = np.asarray(recs, np.int64).reshape(-1, 9)
        flip = ((1 << r[:, 7]) - 1) << (r[:, 6] // r[:, 7] * r[:, 7])
        k = r[:, 4] * self.nthr + r[:, 5]
        if not self.quirk:
            np.bitwise_xor.at(self.x, (r[:, 8], r[:, 3], k), flip & self.emask)
            return
        for m, pe, kk, f in zip(r[:, 8].tolist(), r[:, 3].tolist(), k.tolist(), flip.tolist()):  # (read back as the integer part, in order)
            self.x[m, pe, kk] = (sext(int(self.x[m, pe, kk]), 24) >> 8) ^ f

    def vote(self):
        return maj(self.x[0], self.x[1], self.x[2]) & self.emask

    def repair(self):
        """-> (words rewritten, words whose vote differs from the loaded word, flags)"""
        v = self.vote()
        differs = ((self.x & self.emask) != v[None]).any(axis=0)
        wrong = v != (self.loaded[0] & self.emask)
        self.x = (self.x & ~self.emask) | v[None]
        return int(differs.sum()), int(wrong.sum()), dict(tmr_cleared=bool((differs & ~wrong).any()), tmr_locked=bool((differs & wrong).any()))

    def logical(self):
        """-> (words[pe], logical bits that differ)"""
        v = self.vote()
        d = v ^ (self.loaded[0] & self.emask)
        return [pe.tolist() for pe in v], int(sum(bin(x).count("1") for x in d.reshape(-1).tolist() if x))


class Coded:
    """a coded 16-bit threshold memory: the data memory and the check memory as stored ([pe][line][threshold]; under
    scheme 2 both interleaved, at widths 16 and 6)"""

    def __init__(self, words, F, il):
        assert il in (0, 2)
        self.il = il
        self.files = (np.array(words, np.uint64) & np.uint64(0xFFFF)).astype(np.int64).reshape(F["pe"], F["tmem"], F["nthr"])
        self.loaded = self.store(self.files, er.ENC[self.files])
        self.left2 = np.zeros(self.files.shape, bool)
        self.flags = dict(status2_hit_again=False)
        self.rewrite()

    def store(self, d, c):
        return (er.interleave2(d, 16, True), er.interleave2(c, 6, True)) if self.il else (d.copy(), c.copy())

    def read(self):
        return (er.interleave2(self.data, 16, False), er.interleave2(self.check, 6, False)) if self.il else (self.data, self.check)

    def rewrite(self):
        self.data, self.check = self.loaded[0].copy(), self.loaded[1].copy()
        self.left2[:] = False

    def apply(self, recs):
        r = np.asarray(recs, np.int64).reshape(-1, 9)
        before = self.read()
        before = (before[0].copy(), before[1].copy())
        width = np.where(r[:, 8] == 1, 6, 16)
        flip = (((1 << r[:, 7]) - 1) << (r[:, 6] // r[:, 7] * r[:, 7])) & ((1 << width) - 1)
        for m, mem in ((0, self.data), (1, self.check)):
            k = r[:, 8] == m
            np.bitwise_xor.at(mem, (r[k, 3], r[k, 4], r[k, 5]), flip[k])
        d, c = self.read()
        if (self.left2 & ((d != before[0]) | (c != before[1]))).any():
            self.flags["status2_hit_again"] = True

    def repair(self):
        """-> (status-1 words, words whose stored state still differs from the loaded one, flags)"""
        d, c = self.read()
        status, out = er.decode_all(d, c)
        nd, nc = np.where(status == 1, out, d), np.where(status == 1, er.ENC[out], c)
        self.data, self.check = self.store(nd, nc)
        wrong = (nd != self.files) | (nc != er.ENC[self.files])
        self.left2 = status == 2
        return int((status == 1).sum()), int(wrong.sum()), dict(coded_cleared=bool(((status == 1) & ~wrong).any()),
                                                                 coded_locked=bool(((status == 1) & wrong).any()))

    def logical(self):
        """-> (words[pe], logical data bits that differ, status-1 words, status-2 words)"""
        status, out = er.decode_all(*self.read())
        res = out ^ self.files
        return [pe.reshape(-1).tolist() for pe in out], int(sum(bin(x).count("1") for x in res.reshape(-1).tolist() if x)), \
            int((status == 1).sum()), int((status == 2).sum())


class Redundant:
    """the memories of one run a repair visits: {(layer, target): Voted | Coded}"""

    def __init__(self, network, scheme, code, pdir):
        lay = params_io.layout(network)
        w0, t0 = er.file_words(pdir, network)
        self.layers = len(lay)
        self.mem = {}
        self.flags = {}
        for l, F in enumerate(lay):
            wm, tm, il, cb = er.org(network, scheme, code, l)
            if wm == 3:
                self.mem[(l, 0)] = Voted(w0[l], hr.ebits(network, l, 0), 0, False)
            if cb:
                self.mem[(l, 1)] = Coded(t0[l], F, il)
            elif tm == 3:
                T = hr.ebits(network, l, 1)
                self.mem[(l, 1)] = Voted(t0[l], T, F["nthr"], T == 24)

    def mine(self, recs):
        """which of the records hit one of these memories"""
        recs = np.asarray(recs).reshape(-1, 9)
        return np.isin(recs[:, 2].astype(np.int64) * 2 + recs[:, 1], [l * 2 + target for l, target in self.mem])

    def rewrite(self):
        for m in self.mem.values():
            m.rewrite()

    def apply(self, recs):
        recs = np.asarray(recs, np.int64).reshape(-1, 9)
        for (l, target), m in self.mem.items():  # (the memories are independent; inside one the order is kept)
            m.apply(recs[(recs[:, 2] == l) & (recs[:, 1] == target)])

    def repair(self):
        """-> [layer][2]: the words rewritten, the words still unlike the loaded ones (weights and thresholds together)"""
        out = np.zeros((self.layers, 2), np.int64)
        for (l, _), m in self.mem.items():
            a, b, flags = m.repair()
            out[l] += (a, b)
            for k, v in flags.items():
                self.flags[k] = self.flags.get(k, False) or v
        return out

    def all_flags(self):
        out = dict(self.flags)
        for m in self.mem.values():
            for k, v in getattr(m, "flags", {}).items():
                out[k] = out.get(k, False) or v
        return out


def after(network, scheme, code, pdir, recs):
    """-> (w, t) the words the network computes with after a marker-and-record stream"""
    recs = np.asarray(recs, np.int32).reshape(-1, 9)
    assert ((recs[:, 2] >= 0) | np.isin(recs[:, 2], (REPAIR, REWRITE))).all()
    red = Redundant(network, scheme, code, pdir)
    last = max([i for i in range(len(recs)) if recs[i, 2] == REWRITE], default=-1)
    rest = recs[last + 1:]
    rest = rest[rest[:, 2] >= 0]
    w, t, _, _ = hr.logical_after(network, scheme, pdir, rest[~red.mine(rest)] if len(rest) else rest)  # (a repair never touches these)
    start = 0
    for i in list(np.nonzero(recs[:, 2] < 0)[0]) + [len(recs)]:
        chunk = recs[start:i]
        red.apply(chunk[red.mine(chunk)] if len(chunk) else chunk)
        if i < len(recs):
            (red.repair if recs[i, 2] == REPAIR else red.rewrite)()
        start = i + 1
    for (l, target), m in red.mem.items():
        (t if target else w)[l] = m.logical()[0]
    return w, t


def pack(network, scheme, code, pdir, recs, out_dir):
    w, t = after(network, scheme, code, pdir, recs)
    hr.write_words(out_dir, network, w, t)
    return gl.pack_params(network, out_dir)


def base_counts(network, scheme, code, pdir, per_epoch, scrub_every):
    """-> [epoch][layer][6]: ecc_ref.implied_counts of every epoch -- what the masks imply with rewrites alone.  The large
    memories (the weights of every layer but CNV layer 0: one module, a pure XOR, never repaired) are stepped here, one
    parity bit per physical bit, where implied_counts would count every epoch since the last rewrite again"""
    lay = params_io.layout(network)
    big = [l for l in range(len(lay)) if not (l == 0 and network.startswith("cnv"))]
    none = np.zeros((0, 9), np.int32)
    small = [{k: (none if k[1] == 0 and k[0] in big else v) for k, v in e.items()} for e in per_epoch]
    out = np.zeros((len(per_epoch), len(lay), 6), np.int64)
    parity = {l: np.zeros(xr.memory_bits(network, l, 0), bool) for l in big}
    for t, e in enumerate(per_epoch):
        out[t] = er.implied_counts(network, scheme, code, pdir, small, t, scrub_every)
        for l in big:
            if rewrites(t, scrub_every):
                parity[l][:] = False
            ids = xr.bit_ids(network, e[(l, 0, 0)], l, 0)
            np.logical_xor.at(parity[l], ids, True)
            out[t, l, 0], out[t, l, 1] = len(ids), parity[l].sum()
    return out


def campaign_counts(network, scheme, code, pdir, per_epoch, scrub_every, repair_every, base=None):
    """-> ([epoch][layer][8], flags): the six counts of the coded route -- those of the memories a repair visits restated
    from the stepped physical state -- then the words the epoch's repair rewrote and the words still unlike the loaded ones
    after it.  base: base_counts for this scrub_every, where the caller has it already.  flags: what the stream held (a TMR word cleared by a repair, one locked in, a coded word corrected and
    cleared, one left at status 2 and hit again later, an accepted triple locked in)"""
    red = Redundant(network, scheme, code, pdir)
    base = base_counts(network, scheme, code, pdir, per_epoch, scrub_every) if base is None else base
    out = np.zeros((len(per_epoch), red.layers, 8), np.int64)
    for t, epoch in enumerate(per_epoch):
        if rewrites(t, scrub_every):
            red.rewrite()
        elif repairs(t, scrub_every, repair_every):
            out[t, :, 6:] = red.repair()
        recs = xr.flat(epoch)
        red.apply(recs[red.mine(recs)] if len(recs) else recs)
        # (physical: the epoch's own events; the memories without redundancy: since the last rewrite)
        out[t, :, :6] = base[t]
        for (l, target), m in red.mem.items():
            res = m.logical()
            out[t, l, 1 + 2 * target] = res[1]
            if len(res) == 4:
                out[t, l, 4:6] = res[2:]
    return out, red.all_flags()
