"""An independent numpy restatement of the datapath upset draw (bnn_mi355x_act_noise_campaigns / _act_noise_mask), for
the tests: Philox4x32-10 written from the constants of the paper (Salmon, Moraes, Dror, Shaw: "Parallel random numbers:
as easy as 1, 2, 3", SC'11), and the upset sites of one (run seed, image, layer) as activation-sweep records."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57  # round multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85  # key increments (golden ratio, sqrt(3) - 1)
# (h, w, c) of every non-last layer's output as the next layer reads it (CNV layers 1 and 3 after the max-pool)
CNV_MAPS = [(30, 30, 64), (14, 14, 64), (12, 12, 128), (5, 5, 128), (3, 3, 256), (1, 1, 256), (1, 1, 512), (1, 1, 512)]
LFC_MAPS = [(1, 1, 1024)] * 3


def maps(network):
    return CNV_MAPS if network.startswith("cnv") else LFC_MAPS


def levels(network):
    return 3 if network.endswith("A2") else 2


def philox4x32_10(ctr, key):
    """ctr: four broadcastable arrays of 32-bit words, key: two ints -> uint32 [..., 4]"""
    u64, lo32 = np.uint64, np.uint64(0xFFFFFFFF)
    c = [np.asarray(x).astype(u64) & lo32 for x in np.broadcast_arrays(*ctr)]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = u64(M0) * c[0], u64(M1) * c[2]  # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> u64(32)) ^ c[1] ^ u64(k0), p1 & lo32, (p0 >> u64(32)) ^ c[3] ^ u64(k1), p0 & lo32]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return np.stack(c, axis=-1).astype(np.uint32)


def draw(network, run_seed, image, layer):
    """u of every site of the layer's map, in site order (y, x, channel)"""
    h, w, c = maps(network)[layer]
    sites = h * w * c
    blocks = np.arange((sites + 3) // 4)
    u = philox4x32_10((image, layer, blocks, 0), (run_seed & 0xFFFFFFFF, run_seed >> 32))
    return u.reshape(-1)[:sites]


def mask(network, run_seed, image, layer, rate_q32):
    """-> int32 [k, 5] records {layer, y, x, channel, shift} of the upset sites, in site order"""
    h, w, c = maps(network)[layer]
    u = draw(network, run_seed, image, layer)
    s = np.nonzero(u.astype(np.uint64) < np.uint64(rate_q32))[0]
    shift = 1 + (u[s] & 1).astype(np.int64) if levels(network) == 3 else np.ones(len(s), np.int64)
    return np.stack([np.full(len(s), layer), s // (w * c), (s // c) % w, s % c, shift], axis=1).astype(np.int32)


def apply(network, x, recs):
    """value-domain activations x [elements] int8 (HWC) with the records' sites moved on -> a changed copy"""
    lv = levels(network)
    x = x.copy()
    if len(recs) == 0:
        return x
    h, w, c = maps(network)[int(recs[0, 0])]
    e = (recs[:, 1].astype(np.int64) * w + recs[:, 2]) * c + recs[:, 3]
    i = (x[e].astype(np.int64) + 1) // (2 if lv == 2 else 1)
    i = (i + recs[:, 4]) % lv
    x[e] = (2 * i - 1) if lv == 2 else (i - 1)
    return x
