"""The Python layer of the parameter-memory upset campaigns, without a library: the seven PynqBNN.inference_multiple_*
families against a stub in place of PynqBNN.interface (symbol, argument order as include/bnn_mi355x.h declares it, the
shape of the counts, seeds, timing, error text, dispatch), and NetworkTest.hardening_curve / scrubbing_curve against a
fake FaultTest whose counts have a distinct value in every column.  The two fixtures under tests/golden/ are what the
curves wrote from this file's fake before the seven call bodies and the curves' index arithmetic were folded together."""
import ctypes
import json
import os

import numpy as np
import pytest

import gpu_lib as gl
import oracle_lib as ol

import sys
sys.path.insert(0, os.path.join(gl.ROOT, "bnn-pynq_amd"))

LAYERS, N, EPOCH_IMAGES, RUNS, SEED = 9, 5, 2, 3, 1000
EPOCHS = -(-N // EPOCH_IMAGES)  # 3: two whole epochs and a short last one
SCHEME, CODE, WEIGHT_CODE, WEIGHT_INTERLEAVE, BURST, SCRUB, REPAIR = 2, 7, 11, 13, 3, 4, 6  # (the stub refuses nothing)
USEC = 1.5


class StubLibrary:
    """what PynqBNN.interface has to be for a campaign call: every bnn_mi355x_<family>_campaigns records its arguments,
    fills image_number and usecPerImage and returns classes it owns; the getters hand out synthetic counts and seeds"""

    def __init__(self, fail=False):
        self.fail = fail
        self.calls = []
        self.freed = 0
        self.classes = (ctypes.c_int * (RUNS * N))(*[(7 * i + 3) % 10 for i in range(RUNS * N)])
        self.count_total = 0

    def bnn_mi355x_network(self):
        return b"cnvW1A1"

    def bnn_mi355x_last_error(self):
        return b"the stub says no"

    def free_results(self, ptr):
        self.freed += 1

    @staticmethod
    def _plain(a):
        if isinstance(a, ctypes.POINTER(ctypes.c_uint)):
            return [int(a[i]) for i in range(LAYERS)]
        if hasattr(a, "_obj"):  # ctypes.byref(x)
            return type(a._obj).__name__
        return a

    def _campaigns(self, symbol, per_run):
        def call(*args):
            self.calls.append((symbol, [self._plain(a) for a in args]))
            if self.fail:
                return ctypes.POINTER(ctypes.c_int)()
            args[-2]._obj.value, args[-1]._obj.value = N, USEC
            self.count_total = RUNS * per_run
            return ctypes.cast(self.classes, ctypes.POINTER(ctypes.c_int))
        return call

    def _counts(self, out, cap):
        for i in range(min(cap, self.count_total)):
            out[i] = 5 * i + 2
        return self.count_total

    def _seeds(self, out, cap):
        for r in range(cap):
            out[r] = SEED + r
        return cap

    def __getattr__(self, name):
        if name.endswith("_campaigns"):
            family = name[len("bnn_mi355x_"):-len("_campaigns")]
            return self._campaigns(name, FAMILIES[family]["per_run"])
        if name.startswith("bnn_mi355x_last_") and name.endswith("_counts"):
            self.calls.append((name, None))
            return self._counts
        if name.startswith("bnn_mi355x_last_") and name.endswith("_seeds"):
            self.calls.append((name, None))
            return self._seeds
        raise AttributeError(name)


PATH = "/nowhere/set.bin"
# per family: the method, its call with every organisation argument distinct, the ints the header puts before num_runs and
# after n_rates, the shape of the counts, the words of its error
FAMILIES = {
    "mem_noise": dict(call=lambda b: b.inference_multiple_mem_noise(PATH, RUNS, 0.25, 0.5, SEED),
                      lead=[], tail=[], shape=(RUNS, LAYERS, 2), words="memory noise"),
    "hardened_mem_noise": dict(call=lambda b: b.inference_multiple_hardened_mem_noise(PATH, RUNS, 0.25, 0.5, SCHEME, BURST, SEED),
                               lead=[SCHEME, BURST], tail=[], shape=(RUNS, LAYERS, 2, 2), words="hardened memory noise"),
    "exposure": dict(call=lambda b: b.inference_multiple_exposure(PATH, RUNS, 0.25, 0.5, EPOCH_IMAGES, SCRUB, SCHEME, BURST, SEED),
                     lead=[SCHEME, BURST], tail=[EPOCH_IMAGES, SCRUB], shape=(RUNS, EPOCHS, LAYERS, 2, 2), words="exposure"),
    "ecc_exposure": dict(call=lambda b: b.inference_multiple_ecc_exposure(PATH, RUNS, 0.25, 0.5, EPOCH_IMAGES, SCRUB, SCHEME, CODE, BURST, SEED),
                         lead=[SCHEME, CODE, BURST], tail=[EPOCH_IMAGES, SCRUB], shape=(RUNS, EPOCHS, LAYERS, 6), words="ecc exposure"),
    "repair_exposure": dict(call=lambda b: b.inference_multiple_repair_exposure(PATH, RUNS, 0.25, 0.5, EPOCH_IMAGES, SCRUB, REPAIR, SCHEME, CODE,
                                                                                BURST, SEED),
                            lead=[SCHEME, CODE, BURST], tail=[EPOCH_IMAGES, SCRUB, REPAIR], shape=(RUNS, EPOCHS, LAYERS, 8),
                            words="repair exposure"),
    "wecc_exposure": dict(call=lambda b: b.inference_multiple_wecc_exposure(PATH, RUNS, 0.25, 0.5, EPOCH_IMAGES, SCRUB, REPAIR, SCHEME, CODE,
                                                                            WEIGHT_CODE, BURST, SEED),
                          lead=[SCHEME, CODE, WEIGHT_CODE, BURST], tail=[EPOCH_IMAGES, SCRUB, REPAIR], shape=(RUNS, EPOCHS, LAYERS, 12),
                          words="wecc exposure"),
    "iwecc_exposure": dict(call=lambda b: b.inference_multiple_iwecc_exposure(PATH, RUNS, 0.25, 0.5, EPOCH_IMAGES, SCRUB, REPAIR, SCHEME, CODE,
                                                                              WEIGHT_CODE, WEIGHT_INTERLEAVE, BURST, SEED),
                           lead=[SCHEME, CODE, WEIGHT_CODE, WEIGHT_INTERLEAVE, BURST], tail=[EPOCH_IMAGES, SCRUB, REPAIR],
                           shape=(RUNS, EPOCHS, LAYERS, 12), words="iwecc exposure"),
}
for _f in FAMILIES.values():
    _f["per_run"] = int(np.prod(_f["shape"][1:]))

RATES_W = [1 << 30] * LAYERS                 # 0.25 of 2^32 in every layer
RATES_T = [1 << 31] * (LAYERS - 1) + [0]     # 0.5, and none in CNV layer 8: it has no threshold memory


def _bnn(fail=False):
    from bnn import bnn as mod
    b = mod.PynqBNN.__new__(mod.PynqBNN)
    b.interface = StubLibrary(fail)
    b.classes = ["class %d" % i for i in range(10)]
    b.usecPerImage = 0.0
    return b


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_family_call_and_result(family):
    f = FAMILIES[family]
    b = _bnn()
    result, counts = f["call"](b)
    lib = b.interface
    symbol, args = lib.calls[0]
    assert symbol == "bnn_mi355x_%s_campaigns" % family
    assert args == [PATH.encode(), 10] + f["lead"] + [RUNS, SEED, RATES_W, RATES_T, LAYERS] + f["tail"] + ["c_int", "c_float"]
    assert {c[0] for c in lib.calls[1:]} == {"bnn_mi355x_last_%s_counts" % family, "bnn_mi355x_last_%s_seeds" % family}
    assert result.dtype == np.int32 and result.shape == (RUNS, N) and result.ravel().tolist() == list(lib.classes)
    assert lib.freed == 1
    assert counts.dtype == np.int64 and counts.shape == f["shape"]
    assert counts.ravel().tolist() == [5 * i + 2 for i in range(RUNS * f["per_run"])]
    assert b.mem_noise_seeds == [SEED + r for r in range(RUNS)]
    assert b.usecPerImage == USEC


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_family_error_text(family):
    f = FAMILIES[family]
    b = _bnn(fail=True)
    with pytest.raises(RuntimeError) as e:
        f["call"](b)
    assert str(e.value) == f["words"] + " campaigns failed: the stub says no"
    assert len(b.interface.calls) == 1 and b.interface.freed == 0


def _reached(call):
    b = _bnn()
    _, counts = call(b)
    symbol, args = b.interface.calls[0]
    return symbol[len("bnn_mi355x_"):-len("_campaigns")], args, counts.shape


def test_exposure_dispatch():
    """the five branches of inference_multiple_exposure: which family runs, what it is handed, the shape that comes back"""
    base = (PATH, RUNS, 0.25, 0.5, EPOCH_IMAGES, SCRUB, SCHEME, BURST, SEED)
    head, rates = [PATH.encode(), 10], [RUNS, SEED, RATES_W, RATES_T, LAYERS]
    end = ["c_int", "c_float"]
    assert _reached(lambda b: b.inference_multiple_exposure(*base)) == \
        ("exposure", head + [SCHEME, BURST] + rates + [EPOCH_IMAGES, SCRUB] + end, (RUNS, EPOCHS, LAYERS, 2, 2))
    assert _reached(lambda b: b.inference_multiple_exposure(*base, code=0, repair_every=0, weight_code=0, weight_interleave=0))[0] == "exposure"
    assert _reached(lambda b: b.inference_multiple_exposure(*base, CODE)) == \
        ("ecc_exposure", head + [SCHEME, CODE, BURST] + rates + [EPOCH_IMAGES, SCRUB] + end, (RUNS, EPOCHS, LAYERS, 6))
    assert _reached(lambda b: b.inference_multiple_exposure(*base, 0, REPAIR)) == \
        ("repair_exposure", head + [SCHEME, 0, BURST] + rates + [EPOCH_IMAGES, SCRUB, REPAIR] + end, (RUNS, EPOCHS, LAYERS, 8))
    assert _reached(lambda b: b.inference_multiple_exposure(*base, code=CODE, repair_every=REPAIR)) == \
        ("repair_exposure", head + [SCHEME, CODE, BURST] + rates + [EPOCH_IMAGES, SCRUB, REPAIR] + end, (RUNS, EPOCHS, LAYERS, 8))
    assert _reached(lambda b: b.inference_multiple_exposure(*base, CODE, 0, WEIGHT_CODE)) == \
        ("wecc_exposure", head + [SCHEME, CODE, WEIGHT_CODE, BURST] + rates + [EPOCH_IMAGES, SCRUB, 0] + end, (RUNS, EPOCHS, LAYERS, 12))
    assert _reached(lambda b: b.inference_multiple_exposure(*base, CODE, REPAIR, WEIGHT_CODE, WEIGHT_INTERLEAVE)) == \
        ("iwecc_exposure", head + [SCHEME, CODE, WEIGHT_CODE, WEIGHT_INTERLEAVE, BURST] + rates + [EPOCH_IMAGES, SCRUB, REPAIR] + end,
         (RUNS, EPOCHS, LAYERS, 12))
    # the defaults: no scrub, scheme 0, burst 1, seed 0
    assert _reached(lambda b: b.inference_multiple_exposure(PATH, RUNS, 0.25, 0.5, EPOCH_IMAGES))[1] == \
        head + [0, 1] + [RUNS, 0, RATES_W, RATES_T, LAYERS] + [EPOCH_IMAGES, 0] + end


def test_mem_noise_dispatch():
    """the two branches of inference_multiple_mem_noise: a scheme (0 included) or a burst > 1 is the hardened family"""
    head, rates, end = [PATH.encode(), 10], [RUNS, SEED, RATES_W, RATES_T, LAYERS], ["c_int", "c_float"]
    assert _reached(lambda b: b.inference_multiple_mem_noise(PATH, RUNS, 0.25, 0.5, SEED)) == \
        ("mem_noise", head + rates + end, (RUNS, LAYERS, 2))
    assert _reached(lambda b: b.inference_multiple_mem_noise(PATH, RUNS, 0.25, 0.5, SEED, None, 1))[0] == "mem_noise"
    assert _reached(lambda b: b.inference_multiple_mem_noise(PATH, RUNS, 0.25, 0.5, SEED, 0)) == \
        ("hardened_mem_noise", head + [0, 1] + rates + end, (RUNS, LAYERS, 2, 2))
    assert _reached(lambda b: b.inference_multiple_mem_noise(PATH, RUNS, 0.25, 0.5, SEED, SCHEME, BURST)) == \
        ("hardened_mem_noise", head + [SCHEME, BURST] + rates + end, (RUNS, LAYERS, 2, 2))
    assert _reached(lambda b: b.inference_multiple_mem_noise(PATH, RUNS, 0.25, 0.5, SEED, burst=BURST)) == \
        ("hardened_mem_noise", head + [0, BURST] + rates + end, (RUNS, LAYERS, 2, 2))


# ---- the curves ----
PRIMES = (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37)  # one per column of the widest counts: a swapped index changes a sum


def _synthetic_counts(shape, width, salt):
    """int64 counts of `shape` + the last axes of `width` (4: (2, 2)); column c holds PRIMES[c] times a number that
    differs per run, epoch and layer and with `salt`"""
    cell = np.arange(1, int(np.prod(shape)) + 1, dtype=np.int64).reshape(shape) + salt
    counts = cell[..., None] * np.array(PRIMES[:width], np.int64)
    return counts.reshape(shape + (2, 2)) if width == 4 else counts


class FakeFaultTest:
    """FaultTest as the curves see it: fixed accuracies and counts of the width the organisation asked for"""
    network, dataset = "cnvW1A1", "cifar10"
    labels = [3, 1, 4, 1, 5]
    runs, layers = 2, LAYERS

    def __init__(self):
        self.calls = []

    @staticmethod
    def _salt(scheme, burst, p):
        return 100 * int(scheme or 0) + 10 * int(burst) + int(round(float(p) * 1000))

    def run_memory_noise_test(self, num_runs, rates_w, rates_t, seed=0, scheme=None, burst=1, code=0, weight_code=0, weight_interleave=0):
        self.calls.append(("memory", scheme, burst, code, weight_code, weight_interleave))
        assert rates_w == rates_t
        salt = self._salt(scheme, burst, rates_w) + 7 * weight_interleave
        if weight_code:
            counts = _synthetic_counts((num_runs, self.layers), 12, salt)
        elif code:
            counts = _synthetic_counts((num_runs, self.layers), 6, salt)
        elif scheme is not None or burst != 1:
            counts = _synthetic_counts((num_runs, self.layers), 4, salt)
        else:
            counts = _synthetic_counts((num_runs, self.layers), 2, salt)
        return [80.0 - r - (salt % 17) for r in range(num_runs)], counts

    def run_exposure_test(self, num_runs, rates_w, rates_t, epoch_images, scrub_every=0, scheme=None, burst=1, seed=0, code=0, repair_every=0,
                          weight_code=0, weight_interleave=0):
        self.calls.append(("exposure", scheme, burst, code, weight_code, weight_interleave, scrub_every, repair_every))
        assert rates_w == rates_t
        salt = self._salt(scheme, burst, rates_w) + 7 * weight_interleave + 3 * scrub_every + repair_every
        epochs = -(-len(self.labels) // epoch_images)
        width = 12 if weight_code else 8 if repair_every else 6 if code else 4
        self.exposure_results = np.array([[(l + (1 if (i + r + salt) % 3 == 0 else 0)) % 10 for i, l in enumerate(self.labels)]
                                          for r in range(num_runs)], np.int32)
        per_epoch = [[90.0 - 5 * t - r - (salt % 11) for t in range(epochs)] for r in range(num_runs)]
        return per_epoch, _synthetic_counts((num_runs, epochs, self.layers), width, salt)


SCHEMES = [0, (2, 1), [1, 0, 1], (0, 1, 1, 1), (3, 0), (2, 1, 1)]  # plain scheme, pairs, triples and a 4-tuple
INTERVALS = [0, 2, (4, 1), (0, 2)]                              # numbers and (scrub_every, repair_every) pairs


def run_curves(folder):
    """both curves on the fake -> (hardening dict, scrubbing dict, the fake's calls)"""
    import bnn
    ft = FakeFaultTest()
    nt = bnn.faults.NetworkTest(ft)
    nt.hardening_curve(str(folder), FakeFaultTest.runs, [0.004], SCHEMES, bursts=(1, 2), seed=5)
    nt.scrubbing_curve(str(folder), FakeFaultTest.runs, [0.002], INTERVALS, SCHEMES, EPOCH_IMAGES, bursts=(2,), seed=5)
    base = os.path.join(str(folder), "cnvW1A1", "cifar10")
    with open(os.path.join(base, "hardening", "cnvW1A1_cifar10_hardening_stats.json")) as f:
        hardening = json.load(f)
    with open(os.path.join(base, "scrubbing", "cnvW1A1_cifar10_scrubbing_stats.json")) as f:
        scrubbing = json.load(f)
    return hardening, scrubbing, ft.calls


def test_curves_write_what_they_wrote(tmp_path):
    hardening, scrubbing, calls = run_curves(tmp_path)
    with open(os.path.join(ol.GOLDEN, "upset_hardening_stats.json")) as f:
        assert hardening == json.load(f)
    with open(os.path.join(ol.GOLDEN, "upset_scrubbing_stats.json")) as f:
        assert scrubbing == json.load(f)
    # the control run first (today's plain path), then every organisation reaches the fake with all four of its parts
    assert calls[0] == ("memory", None, 1, 0, 0, 0)
    want = [(0, 0, 0, 0), (2, 1, 0, 0), (1, 0, 1, 0), (0, 1, 1, 1), (3, 0, 0, 0), (2, 1, 1, 0)]
    assert [c[1:2] + c[3:6] for c in calls if c[0] == "memory"][1::2] == want
    assert [c[1:2] + c[3:6] for c in calls if c[0] == "exposure"][::4] == want
    assert [c[6:] for c in calls if c[0] == "exposure"][:4] == [(0, 0), (2, 0), (4, 1), (0, 2)]
