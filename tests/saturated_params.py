"""Constant networks with closed-form activations: parameter sets whose accumulators sit at the ENDS of their range.

random_params.py and the shipped sets keep every accumulator behind layer 0 within a few standard deviations of its
centre.  The sets made here put rows at matches in {0, 1, 2, mw/2, mw-2, mw-1, mw} (1-bit nets) and d = +-sum|a|, +-mw,
+-2 mw (2-bit nets, the last with weights of -2), with thresholds exactly at and one below the row's accumulator, at the
neighbours of the clamps the kernels' tables apply, and at the int16 extremes.

CNV: layer 0's thresholds are the lowest / highest a 24-bit field holds, so its map is one channel pattern on every
pixel whatever the image; a 3x3 convolution and a 2x2 max-pool of a constant map are constant, so every later map is one
channel vector too and the whole network's output does not depend on the image.  LFC: layer 0 reads the image, so the
set comes with four images (all 0, all 255, a fixed pattern P and its complement) and layer-0 rows written against each
of them (the 48 padding columns of the input are bits of 0, value -1, as in the reference).

Each crafted layer's rows cycle a catalogue of (weight case, threshold case); the designed output of layer l is the
input pattern layer l + 1 is crafted against.  Configurations:
  mixed        layer 0 mixes -1 / (0) / +1; every later layer is crafted
  sat_even+/-  layers 0, 2, 4, 6 never / always fire (thresholds beyond the reachable range, clamp neighbours among
               them): the crafted layers 1, 3, 5, 7 read an all +1 / all -1 map and reach the absolute bounds
  sat_odd+/-   the same with layers 1, 3, 5, 7 saturated: layers 2, 4, 6, 8 reach the bounds
(the last thresholded layer of an LFC net is always crafted).  Written with bnn/params_io.py, as random_params.py is."""
import numpy as np

from bnn import params_io

CONFIGS = ("mixed", "sat_even+", "sat_even-", "sat_odd+", "sat_odd-")
CNV_SHAPE = [(900, 64), (196, 64), (144, 128), (25, 128), (9, 256), (1, 256), (1, 512), (1, 512)]  # pixels, channels
L0_LO, L0_HI = -(1 << 23), (1 << 23) - 1      # CNV layer 0: 24-bit thresholds, |2 * dot| <= 4 * 27 * 128
I16_LO, I16_HI = -32768, 32767
PRIMARY = 2                                    # LFC: layers 1.. are crafted against image P


def variants(network):
    """every (config, neg2) of `network`; neg2 (cnvW2A2): rows with weights of -2, which select the -2-aware kernels"""
    return [(c, n) for n in ((False, True) if network == "cnvW2A2" else (False,)) for c in CONFIGS]


def kind(network, l):
    """what a layer accumulates: 'int8' (CNV layer 0), 'xnor' = number of matches, 'signed' = sum of w * a"""
    if network.startswith("cnv") and l == 0:
        return "int8"
    return "signed" if network.endswith("A2") else "xnor"


def lfc_images():
    """all 0, all 255, the fixed pattern P, its complement: uint8 [4, 784]"""
    p = np.random.default_rng(784).integers(0, 256, 784, dtype=np.uint8)
    return np.stack([np.zeros(784, np.uint8), np.full(784, 255, np.uint8), p, 255 - p])


def lfc_inputs(imgs):
    """binarizeAndPack in the value domain: [n, 832], +1 where the pixel is >= 128, the 48 padding columns -1"""
    x = np.full((len(imgs), 832), -1, np.int64)
    x[:, :784] = np.where(imgs >= 128, 1, -1)
    return x


# ---------------------------------------------------------------------------------------------------------------------
# the restated arithmetic: one accumulator per row, strict compares
# ---------------------------------------------------------------------------------------------------------------------
def accumulate(knd, W, a):
    d = W.astype(np.int64) @ a.astype(np.int64)
    return (W.shape[1] + d) // 2 if knd == "xnor" else d      # matches = (mw + dot) / 2 on +-1 operands


def decide(acc, T, nthr):
    """ThresholdsActivation: fire_i <=> t_i < acc (strict); one threshold: +-1, two: -1 + fire_0 + fire_1"""
    T = np.asarray(T, np.int64).reshape(len(acc), -1)
    if nthr == 1:
        return np.where(T[:, 0] < acc, 1, -1)
    return -1 + (T[:, 0] < acc).astype(np.int64) + (T[:, 1] < acc)


# ---------------------------------------------------------------------------------------------------------------------
# the catalogue
# ---------------------------------------------------------------------------------------------------------------------
def weight_cases(wbits, neg2):
    c = ["k0", "k1", "k2", "kmid", "kmw-2", "kmw-1", "kmw"]
    if wbits == 2:
        c += ["zero"] + (["all-2", "one-2"] if neg2 else [])
    return c


def corner_columns(mw):
    return [0, 63, 64, mw - 64, mw - 1]


def weight_row(case, a, v):
    """the row of `case` against the input pattern a; v: which variant (the place of the differing columns)"""
    mw = len(a)
    s = np.where(a != 0, a, 1).astype(np.int64)      # the input's sign pattern (a zero activation counts as +1)
    pos = corner_columns(mw)
    one, two = [pos[v % 5]], [pos[v % 5], pos[(v + 1) % 5]]
    flip = np.zeros(mw, bool)
    if case == "zero":
        return np.zeros(mw, np.int64)
    if case == "all-2":
        return np.full(mw, -2, np.int64)
    if case == "one-2":
        w = s.copy()
        w[one] = -2
        return w
    if case == "k1":
        flip[one] = True
    elif case == "k2":
        flip[two] = True
    elif case == "kmid":
        flip[(np.arange(mw) + v) % 2 == 0] = True    # mw / 2 columns, 32 in every 64-column k step
    elif case == "kmw-2":
        flip[:] = True
        flip[two] = False
    elif case == "kmw-1":
        flip[:] = True
        flip[one] = False
    elif case == "kmw":
        flip[:] = True
    else:
        assert case == "k0", case
    return np.where(flip, -s, s)


def absolute_thresholds(knd, mw):
    """the neighbours of the table clamps (file units) and of the reachable range, and the int16 extremes"""
    if knd == "xnor":
        return [-1, 0, 1, mw, mw + 1, mw + 2, mw + 3, I16_LO, I16_HI]
    lim = 2 * mw
    return [-lim - 2, -lim - 1, -lim, lim - 1, lim, lim + 1, -mw - 1, -mw, mw - 1, mw, I16_LO, I16_HI]


def threshold_cases(knd, mw, nthr):
    """(relative, absolute) cases: (name, function of the row's accumulator -> thresholds, at the low end of the range)"""
    low = (lambda t: t <= 1) if knd == "xnor" else (lambda t: t < 0)
    at = absolute_thresholds(knd, mw)
    if nthr == 1:
        rel = [("d-1", lambda d: (d - 1,), None), ("d", lambda d: (d,), None)]
        ab = [("abs %d" % t, lambda d, t=t: (t,), low(t)) for t in at]
    else:
        rel = [("eq d-1", lambda d: (d - 1, d - 1), None), ("eq d", lambda d: (d, d), None), ("pair", lambda d: (d - 1, d), None),
               ("pair unordered", lambda d: (d, d - 1), None)]
        ab = [("abs %d" % t, lambda d, t=t: (t, t), low(t)) for t in at]
        ab += [("abs %d %d" % (x, y), lambda d, x=x, y=y: (x, y), i == 0) for i, (x, y) in enumerate(((at[1], at[4]), (at[4], at[1])))]
    return rel, ab


def saturating_thresholds(knd, mw, fire):
    """thresholds no accumulator of the layer reaches: every row fires (fire) or none does"""
    if knd == "xnor":
        return [I16_LO, -1, -2] if fire else [I16_HI, mw, mw + 1, mw + 2, mw + 3]
    lim = 2 * mw
    return [I16_LO, -lim - 1, -lim - 2] if fire else [I16_HI, lim, lim + 1]


def craft(knd, wbits, nthr, mh, a, neg2, saturate=None, slots=None):
    """one layer against the input pattern a -> (W [mh, mw], T [mh, max(nthr, 1)], designed output [mh] (the
    accumulators where nthr == 0), design record).  saturate: None, +1 or -1.  slots[n]: the catalogue slot of row n
    (default n)."""
    mw = len(a)
    wc = weight_cases(wbits, neg2)
    base = {c: int(accumulate(knd, weight_row(c, a, 0)[None], a)[0]) for c in wc}
    lowest, highest = min(wc, key=lambda c: base[c]), max(wc, key=lambda c: base[c])
    W = np.zeros((mh, mw), np.int64)
    T = np.zeros((mh, max(nthr, 1)), np.int64)
    names_w, names_t = [], []
    if nthr and saturate is None:
        rel, ab = threshold_cases(knd, mw, nthr)
        plan = [(c, t) for c in wc for t in rel]
        # an absolute threshold at the low end meets the row with the lowest accumulator, one at the high end the highest
        plan += [(lowest if t[2] else highest, t) for t in ab]
        allt = rel + ab
    seen = {}
    for n in range(mh):
        q = n if slots is None else int(slots[n])
        if nthr == 0 or saturate is not None:
            case, tc = wc[q % len(wc)], None
        elif q < len(plan):
            case, tc = plan[q]
        else:
            r = q - len(plan)
            case, tc = wc[(r + r // len(allt)) % len(wc)], allt[r % len(allt)]
        v = seen.get((case, q), None)
        if v is None:
            v = seen[(case, q)] = sum(1 for k in seen if k[0] == case)
        W[n] = weight_row(case, a, v)
        names_w.append(case)
        names_t.append(tc)
    acc = accumulate(knd, W, a)
    if nthr == 0:
        return W, T, acc, dict(weights=names_w, thresholds=[None] * mh, acc=acc, crafted=True)
    if saturate is not None:
        st = saturating_thresholds(knd, mw, saturate > 0)
        for i in range(T.shape[1]):
            T[:, i] = [st[(n + 2 * i) % len(st)] for n in range(mh)]
        names = ["sat %s" % (tuple(t),) for t in T.tolist()]
    else:
        for n in range(mh):
            T[n] = names_t[n][1](int(acc[n]))
        names = [t[0] for t in names_t]
    T = np.clip(T, I16_LO, I16_HI)
    return W, T, decide(acc, T, nthr), dict(weights=names_w, thresholds=names, acc=acc, crafted=saturate is None)


def _saturate(config, l, last):
    """+1 / -1 where layer l of `config` is a saturated one"""
    if config == "mixed" or l >= last:
        return None
    if (l % 2 == 0) == config.startswith("sat_even"):
        return 1 if config.endswith("+") else -1
    return None


def make(directory, network, config="mixed", neg2=False):
    """-> (weights, thresholds, expected).  expected: 'layers' = the value-domain map after every thresholded layer in
    the layout of Oracle.layer_ref (LFC: [4, 1024] per layer, one row per image of lfc_images()), 'scores' (CNV, int16
    [64]) or 'words' (LFC, one int per image), 'design' = per layer the catalogue case and accumulator of every row."""
    assert config in CONFIGS and (not neg2 or network == "cnvW2A2")
    lay = params_io.layout(network)
    cnv = network.startswith("cnv")
    a2 = network.endswith("A2")
    nl = len(lay)
    last = nl - 1                                   # CNV: the score layer; LFC: the output word's layer (always crafted)
    weights, thresholds, layers, design = [], [], [], []
    if cnv:
        rng = np.random.default_rng(27)
        L = lay[0]
        vals, p = ([-1, 1], None) if L["wbits"] == 1 else ([-1, 0, 1, -2], [0.35, 0.3, 0.35, 0.0] if not neg2 else [0.3, 0.3, 0.3, 0.1])
        W = rng.choice(np.array(vals, np.int64), size=(L["mh"], L["mw"]), p=p)
        sat = _saturate(config, 0, last)
        ch = np.arange(64)
        if sat is not None:
            out = np.full(64, sat, np.int64)
        elif a2:
            out = np.array([1, -1, 0], np.int64)[ch % 3]
        else:
            out = np.where(ch % 2 == 0, 1, -1)
        if a2:   # +1: both lowest, -1: both highest, 0: one of each, every other such pair unordered
            T = np.stack([np.where(out > 0, L0_LO, np.where(out < 0, L0_HI, np.where(ch % 2 == 0, L0_LO, L0_HI))),
                          np.where(out > 0, L0_LO, np.where(out < 0, L0_HI, np.where(ch % 2 == 0, L0_HI, L0_LO)))], axis=1)
        else:
            T = np.where(out > 0, L0_LO, L0_HI)[:, None]
        weights.append(W)
        thresholds.append(T)
        layers.append(np.tile(out, CNV_SHAPE[0][0]).astype(np.int8))
        design.append(dict(weights=None, thresholds=None, acc=None, crafted=False))
        pattern = out
        first = 1
    else:
        imgs = lfc_images()
        x = lfc_inputs(imgs)                        # [4, 832]: every image's own pattern
        pattern, first = x[PRIMARY], 0
    for l in range(first, nl):
        L = lay[l]
        conv = cnv and l < 6
        a = np.tile(pattern, 9) if conv else pattern
        assert len(a) == L["mw"], (l, len(a), L["mw"])
        knd = kind(network, l)
        sat = _saturate(config, l, last)
        if not cnv and l == 0:
            # every catalogue slot once per image: row n is written against image n % 4
            parts = [craft(knd, L["wbits"], L["nthr"], L["mh"] // 4, x[i], False, sat) for i in range(4)]
            W = np.zeros((L["mh"], L["mw"]), np.int64)
            T = np.zeros((L["mh"], L["nthr"]), np.int64)
            for i, p in enumerate(parts):
                W[i::4], T[i::4] = p[0], p[1]
            d = dict(weights=[parts[n % 4][3]["weights"][n // 4] for n in range(L["mh"])],
                     thresholds=[parts[n % 4][3]["thresholds"][n // 4] for n in range(L["mh"])],
                     acc=np.stack([accumulate(knd, W, x[i]) for i in range(4)]), crafted=sat is None, image=np.arange(L["mh"]) % 4)
            out = np.stack([decide(d["acc"][i], T, L["nthr"]) for i in range(4)])
            for i, p in enumerate(parts):              # the design holds on the image each row was written for
                assert (out[i, i::4] == p[2]).all()
        else:
            W, T, out, d = craft(knd, L["wbits"], L["nthr"], L["mh"], a, neg2, sat)
            if not cnv:                                # the other three images: the restated arithmetic
                acc = np.stack([accumulate(knd, W, x[i]) for i in range(4)])
                full = np.stack([decide(acc[i], T, L["nthr"]) for i in range(4)])
                assert (full[PRIMARY] == out).all() and (acc[PRIMARY] == d["acc"]).all()
                out, d["acc"] = full, acc
        weights.append(W)
        thresholds.append(T)
        design.append(d)
        if cnv:
            if L["nthr"]:
                layers.append(np.tile(out, CNV_SHAPE[l][0]).astype(np.int8))
                pattern = out
            else:
                scores = (out & 0xFFFF).astype(np.uint16).view(np.int16)
        else:
            layers.append(out.astype(np.int8))
            x = out
            pattern = out[PRIMARY]
    params_io.write_params(directory, network, weights, thresholds, classes=[str(i) for i in range(10)])
    expected = dict(layers=layers, design=design)
    if cnv:
        expected["scores"] = scores
    else:
        expected["words"] = [int(sum(1 << n for n in range(64) if layers[-1][i][n] > 0)) for i in range(4)]
        expected["images"] = imgs
    return weights, thresholds, expected


# ---------------------------------------------------------------------------------------------------------------------
# the matched-filter variant: the pooled layers (CNV 1 and 3), where a constant map makes the 2x2 pool trivial
# ---------------------------------------------------------------------------------------------------------------------
MATCHED_ROWS = range(24, 40)       # 16 rows across the boundary of two 32-neuron tiles
MATCHED_CELL = {1: (3, 5, 30, 64), 3: (2, 1, 12, 128)}   # layer -> pool cell (y, x), input width, input channels


def make_matched(directory, network, seed, layer, image):
    """a random_params set whose layer `layer` (1 or 3) holds, for the window at each of the four positions of one pool
    cell of `image`'s layer - 1 map (from the oracle), four rows: the window's sign, its negation, and each with one
    column flipped; thresholds one and two below the full match and the mirrored pair.  The truth is the oracle on the
    written set.  -> (weights, thresholds)"""
    import oracle_lib as ol
    import random_params
    W, T = random_params.make(directory, network, seed)
    o = ol.Oracle(network, directory)
    py, px, width, ch = MATCHED_CELL[layer]
    prev = o.layer_ref(image, layer - 1).astype(np.int64).reshape(width, width, ch)
    o.close()
    knd = kind(network, layer)
    L = params_io.layout(network)[layer]
    mw = L["mw"]
    rows = list(MATCHED_ROWS)
    for k, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        oy, ox = 2 * py + dy, 2 * px + dx
        a = prev[oy:oy + 3, ox:ox + 3, :].reshape(-1)              # (ky, kx, c): the reference's column order
        assert len(a) == mw
        s = a.copy() if L["wbits"] == 2 else np.where(a != 0, a, 1)
        col = corner_columns(mw)[k]
        while a[col] == 0:                                          # (a column that counts: a zero activation does not)
            col = (col + 1) % mw
        one = s.copy()
        one[col] = -one[col]
        for j, w in enumerate((s, -s, one, -one)):
            n = rows[4 * k + j]
            d = int(accumulate(knd, w[None], a)[0])
            W[layer][n] = w
            # the window's own rows fire on (nearly) the window alone, the negated ones everywhere but there; a 2-bit pair
            # lies just below (window) or straddles (one column off) the accumulator, unordered on the negated rows
            if L["nthr"] == 1:
                T[layer][n] = d - 1 if j % 2 == 0 else d
            else:
                T[layer][n] = ((d - 1, d - 2), (d, d + 1), (d - 1, d), (d + 1, d))[j]
    params_io.write_params(directory, network, W, T, classes=[str(i) for i in range(10)])
    return W, T
