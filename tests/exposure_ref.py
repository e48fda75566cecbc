"""Plain-Python restatement of the exposure campaigns' model (csrc/mem_org.h, "exposure campaigns"), on top of
tests/hardened_ref.py: the hardened draw with the epoch in the fourth Philox counter word, the masks of an epoch in the
in-epoch order, their concatenation since the last scrub, and -- from the records alone -- the physical bits a module's
events flip, their accumulation (XOR: a bit hit an even number of times is back) and the counts they imply.  Shared by
tests/test_exposure_mask.py and tests/test_gpu_exposure.py."""
import ctypes as C

import numpy as np

import act_noise_ref as ref
import hardened_ref as hr

from bnn import params_io

ip = C.POINTER(C.c_int)
MAX_EPOCHS = 1 << 16


def first_epoch(t, scrub_every):
    """the last epoch <= t whose upsets met freshly written memories"""
    return t - t % scrub_every if scrub_every > 0 else 0


def events(network, burst, seed, epoch, layer, target, module, rate):
    """hardened_ref.events with the epoch: counter {L, target | m << 1 | (b - 1) << 8, e >> 2, 1 + (t << 8)}; the record's
    image field holds the epoch"""
    F = params_io.layout(network)[layer]
    eb = hr.ebits(network, layer, target)
    if eb == 0:
        return np.zeros((0, 9), np.int32)
    per = -(-eb // burst)
    inds, thr = (F["wmem"], 1) if target == 0 else (F["tmem"], F["nthr"])
    n = F["pe"] * inds * thr * per
    word = target | module << 1 | (burst - 1) << 8
    u = ref.philox4x32_10((layer, word, np.arange((n + 3) // 4), 1 + (epoch << 8)), (seed & 0xFFFFFFFF, seed >> 32)).reshape(-1)[:n]
    e = np.nonzero(u.astype(np.uint64) < np.uint64(rate))[0]
    el, g = e // per, e % per
    rec = np.zeros((len(e), 9), np.int32)
    rec[:, 0], rec[:, 1], rec[:, 2], rec[:, 7], rec[:, 8] = epoch, target, layer, burst, module
    rec[:, 5], rec[:, 4], rec[:, 3], rec[:, 6] = el % thr, (el // thr) % inds, el // thr // inds, g * burst
    return rec


def memories(network, scheme, only=None):
    """(layer, target, module) in the in-epoch order: layer-major, weights then thresholds, module-major.  only: a
    predicate on (layer, target)"""
    nl = len(params_io.layout(network))
    return [(l, t, m) for l in range(nl) for t in (0, 1) for m in range(hr.org(network, scheme, l)[t]) if only is None or only(l, t)]


def small(layer, target):
    """the memories a scheme replicates or interleaves, and layer 0: every threshold memory, layer 0's weights"""
    return target == 1 or layer == 0


def epoch_events(network, scheme, burst, seed, epoch, rw, rt, only=None):
    """-> {(layer, target, module): records}, in the in-epoch order"""
    return {(l, t, m): events(network, burst, seed, epoch, l, t, m, (rw, rt)[t][l]) for l, t, m in memories(network, scheme, only)}


def lib_mask(L, scheme, burst, seed, epoch, layer, target, module, rate, first=0, cap=None):
    total = L.bnn_mi355x_exposure_mask(scheme, burst, seed, epoch, layer, target, module, rate, 0, None, 0)
    assert total >= 0, L.bnn_mi355x_last_error()
    cap = max(total - first, 0) if cap is None else cap
    rec = np.zeros((max(cap, 1), 9), np.int32)
    assert L.bnn_mi355x_exposure_mask(scheme, burst, seed, epoch, layer, target, module, rate, first, rec.ctypes.data_as(ip), cap) == total
    return rec[:max(min(cap, total - first), 0)]


def lib_epoch_events(L, network, scheme, burst, seed, epoch, rw, rt):
    return {(l, t, m): lib_mask(L, scheme, burst, seed, epoch, l, t, m, (rw, rt)[t][l]) for l, t, m in memories(network, scheme)}


def flat(epoch):
    return np.concatenate([np.zeros((0, 9), np.int32)] + list(epoch.values()))


def since_scrub(per_epoch, t, scrub_every):
    """the records the blob of epoch t is pack_params_hardened of: epochs (last scrub epoch <= t) ... t, epoch-major"""
    return np.concatenate([flat(e) for e in per_epoch[first_epoch(t, scrub_every): t + 1]])


# ---- from the records alone: which physical bits, how often ------------------------------------------------------------

def memory_bits(network, layer, target):
    F = params_io.layout(network)[layer]
    return F["pe"] * (F["wmem"] if target == 0 else F["tmem"] * F["nthr"]) * hr.ebits(network, layer, target)


def bit_ids(network, recs, layer, target):
    """the physical bits (one integer per (mem, ind, thresh, bit)) the records of ONE module of one memory flip, with
    repetitions (one entry per flip; a burst clipped to its element)"""
    F = params_io.layout(network)[layer]
    eb = hr.ebits(network, layer, target)
    inds, thr = (F["wmem"], 1) if target == 0 else (F["tmem"], F["nthr"])
    r = recs.astype(np.int64)
    if len(r) == 0:
        return np.zeros(0, np.int64)
    base = ((r[:, 3] * inds + r[:, 4]) * thr + r[:, 5]) * eb + r[:, 6]
    width = np.minimum(r[:, 7], eb - r[:, 6])
    return np.concatenate([base[width > j] + j for j in range(int(r[:, 7].max()))])


def hit_counts(network, epochs, layer, target, module):
    """how often each physical bit of one module is flipped by the given epochs' records"""
    size = memory_bits(network, layer, target)
    out = np.zeros(size, np.int64)
    for e in epochs:
        out += np.bincount(bit_ids(network, e[(layer, target, module)], layer, target), minlength=size)
    return out


def state(network, epochs, layer, target, modules):
    """what the XOR leaves: per module, the bits flipped an odd number of times; three modules: then the majority"""
    s = [hit_counts(network, epochs, layer, target, m) & 1 for m in range(modules)]
    return (s[0] + s[1] + s[2] >= 2).astype(np.int64) if modules == 3 else s[0]


def implied_counts(network, scheme, pdir, per_epoch, t, scrub_every):
    """[layer][target][physical bits flipped IN epoch t, logical bits that differ AFTER it] from the masks: physical, the
    bits of the epoch's events; logical, with S the epochs since the last scrub: one module (interleaved or not: a
    permutation), the bits S flips an odd number of times; three modules, the bits that is true of in two or more.
    Layer 0 of a CNV net (24-bit thresholds read back as their integer part) through hardened_ref's own route."""
    lay = params_io.layout(network)
    since = per_epoch[first_epoch(t, scrub_every): t + 1]
    out = np.zeros((len(lay), 2, 2), np.int64)
    cnv = network.startswith("cnv")
    for layer in range(1 if cnv else 0, len(lay)):
        for target in (0, 1):
            mods = hr.org(network, scheme, layer)[target]
            if hr.ebits(network, layer, target) == 0:
                continue
            out[layer, target, 0] = sum(len(bit_ids(network, per_epoch[t][(layer, target, m)], layer, target)) for m in range(mods))
            out[layer, target, 1] = state(network, since, layer, target, mods).sum()
    if cnv:
        zero = lambda e: np.concatenate([np.zeros((0, 9), np.int32)] + [v for k, v in e.items() if k[0] == 0])
        _, _, physical, _ = hr.logical_after(network, scheme, pdir, zero(per_epoch[t]), only=(0,))
        _, _, _, logical = hr.logical_after(network, scheme, pdir, np.concatenate([zero(e) for e in since]), only=(0,))
        out[0, :, 0], out[0, :, 1] = physical[0], logical[0]
    return out
