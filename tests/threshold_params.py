"""cnvW1A1 parameter sets with chosen thresholds in layers 1-3 (random_params.py draws thresholds, it cannot set them):
random weights and the other layers' thresholds from random_params.make, then the threshold files of layers 1-3
rewritten in place -- one neuron of every 32-neuron tile always firing and the others never (one_hot), or a mix of
rows that meet their threshold exactly and rows that saturate (boundary).  Written with bnn/params_io.py's file layout."""
import os

import numpy as np

from bnn import params_io

NETWORK = "cnvW1A1"
ALWAYS, NEVER = -32768, 32767  # "mismatches < t" with t clamped by the table: fires for every input / for none


def make_base(directory, seed):
    import random_params
    random_params.make(directory, NETWORK, seed)


def _write_thresholds(directory, layer, T):
    L = params_io.layout(NETWORK)[layer]
    T = np.asarray(T, np.int64).reshape(L["mh"], 1)
    for p in range(L["pe"]):
        T[p::L["pe"]].astype("<i8").tofile(os.path.join(directory, "%d-%d-thres.bin" % (layer, p)))


def one_hot(directory, j):
    """neuron 32 * tile + j of every tile of layers 1-3 always fires, every other neuron never does"""
    for layer in (1, 2, 3):
        mh = params_io.layout(NETWORK)[layer]["mh"]
        _write_thresholds(directory, layer, np.where(np.arange(mh) % 32 == j, ALWAYS, NEVER))


def boundary(directory, seed):
    """layers 1-3: of every four consecutive neurons one always fires, one never does, and two have their threshold within 3
    of the mean of the match count (mw / 2), so that accumulators of -1 (count == threshold) and +1 sit next to
    saturating ones in every tile"""
    rng = np.random.default_rng(seed)
    for layer in (1, 2, 3):
        L = params_io.layout(NETWORK)[layer]
        n = np.arange(L["mh"])
        near = L["mw"] // 2 + rng.integers(-3, 4, L["mh"])
        kind = (n + rng.integers(0, 4)) % 4
        _write_thresholds(directory, layer, np.where(kind == 0, ALWAYS, np.where(kind == 1, NEVER, near)))
