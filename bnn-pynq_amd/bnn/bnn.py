"""Python classifier API of the MI355X-native BNN-PYNQ runtime.

Mirrors the public surface of the reference's ``bnn/bnn.py`` (names, argument
meaning, printed messages, return types) so that code and notebooks written
against ``bnn.LfcClassifier`` / ``bnn.CnvClassifier`` run unchanged:

  reference                          here
  ---------------------------------  -------------------------------------------
  bnn.py:37-53   RUNTIME_*/NETWORK_*  same constants
  bnn.py:55-65   PLATFORM / *_DIR     PLATFORM = "mi355x" (no $BOARD needed)
  bnn.py:67-79   cffi cdef + dlopen   ctypes binding of the same six symbols (_CDEF)
  bnn.py:82-91   available_params     same
  bnn.py:94-207  PynqBNN              same methods; no bitstream download
  bnn.py:210-345 CnvClassifier        same 13 classify_* methods + image_to_cifar
  bnn.py:348-388 LfcClassifier        same

The shared object it loads, ``libraries/<PLATFORM>/<runtime>-<network>-
<PLATFORM>.so``, is the HIP runtime built from ``../csrc`` (C ABI:
``include/bnn_mi355x.h``).  There is no CPU implementation behind this module:
if the library is missing the constructor raises.

Additions (not in the reference): ``PynqBNN.inference_array`` /
``classify_array`` for images already in a numpy array, and ``bnn.multigpu``.
"""
import ctypes
import os
import tempfile

import numpy as np

from . import abi

try:  # the reference imports PIL unconditionally; keep the module importable without it
    from PIL import Image
except ImportError:  # pragma: no cover
    Image = None

RUNTIME_HW = "python_hw"
RUNTIME_SW = "python_sw"

NETWORK_CNVW1A1 = "cnvW1A1"
NETWORK_CNVW1A1_INTERLEAVED = "cnvW1A1-interleaved"
NETWORK_CNVW1A1_RESILIENT_INTERLEAVED = "cnvW1A1-resilient-interleaved"
NETWORK_CNVW1A1_TMR = "cnvW1A1-TMR"
NETWORK_CNVW1A2 = "cnvW1A2"
NETWORK_CNVW1A2_INTERLEAVED = "cnvW1A2-interleaved"
NETWORK_CNVW1A2_RESILIENT_INTERLEAVED = "cnvW1A2-resilient-interleaved"
NETWORK_CNVW2A2 = "cnvW2A2"
NETWORK_CNVW2A2_INTERLEAVED = "cnvW2A2-interleaved"
NETWORK_CNVW2A2_RESILIENT_INTERLEAVED = "cnvW2A2-resilient-interleaved"
NETWORK_CNVW2A2_TMR = "cnvW2A2-TMR"
NETWORK_LFCW1A1 = "lfcW1A1"
NETWORK_LFCW1A2 = "lfcW1A2"
NETWORK_LFCW1A2_INTERLEAVED = "lfcW1A2-interleaved"

# The reference derives PLATFORM from $BOARD (Ultra96 / Pynq-Z1 / Pynq-Z2); a GPU
# host has no such variable.  BNN_PLATFORM overrides the directory name.
PLATFORM = abi.PLATFORM

BNN_ROOT_DIR = os.path.dirname(os.path.realpath(__file__))
BNN_LIB_DIR = abi.LIB_DIR
BNN_BIT_DIR = os.path.join(BNN_ROOT_DIR, "bitstreams", PLATFORM)  # kept for name compatibility; unused
BNN_PARAM_DIR = os.path.join(BNN_ROOT_DIR, "params")

# the reference's cdef, verbatim signatures: the contract both sides bind to
_CDEF = """
void load_parameters(const char* path);
int inference(const char* path, int results[64], int number_class, float *usecPerImage);
int* inference_multiple(const char* path, int number_class, int *image_number, float *usecPerImage, int enable_detail);
int* inference_multiple_with_faults(const char* path, int number_class, int *image_number, float *usecPerImage, unsigned int flip_count, int word_size, int target, int* target_layers, unsigned int num_targets);
void free_results(int * result);
void deinit();
"""

_libraries = {}


def _open_library(dllname):
    """dlopen once per process and name, like the reference's _libraries cache"""
    if dllname not in _libraries:
        _libraries[dllname] = abi.load_path(os.path.join(BNN_LIB_DIR, dllname))
    return _libraries[dllname]


def _param_name(network, dataset_dir):
    """directory name holding `network`'s parameters: the hardened variants (-TMR, -interleaved,
    -resilient-interleaved) ship byte-identical copies of their base network's files in the
    reference; this package keeps one copy and resolves the variant to its base when absent"""
    names = os.listdir(dataset_dir)
    if network in names:
        return network
    base = network.split("-")[0]
    return base if base != network and base in names else None


def available_params(network):
    """datasets for which a parameter set of `network` is installed"""
    found = []
    for dataset in os.listdir(BNN_PARAM_DIR):
        dpath = os.path.join(BNN_PARAM_DIR, dataset)
        if os.path.isdir(dpath) and _param_name(network, dpath):
            found.append(dataset)
    return found


class PynqBNN:
    """Interface object onto the per-network shared library."""

    def __init__(self, runtime, network, load_overlay=True):
        # RUNTIME_HW meant "download the FPGA bitstream" in the reference; on
        # MI355X both runtime names resolve to the same HIP library.
        self.bitstream_name = None
        dllname = "{0}-{1}-{2}.so".format(runtime, network, PLATFORM)
        self.interface = _open_library(dllname)
        self.num_classes = 0
        self.classes = []
        self.usecPerImage = 0.0

    def __del__(self):
        try:
            self.interface.deinit()
        except Exception:
            pass

    def load_parameters(self, params):
        if not os.path.isabs(params):
            params = os.path.join(BNN_PARAM_DIR, params)
            if not os.path.isdir(params) and os.path.isdir(os.path.dirname(params)):
                name = _param_name(os.path.basename(params), os.path.dirname(params))
                if name:
                    params = os.path.join(os.path.dirname(params), name)
        if os.path.isdir(params):
            self.interface.load_parameters(params.encode())
            with open(os.path.join(params, "classes.txt")) as f:
                self.classes = [c.strip() for c in f.readlines()]
        else:
            print("\nERROR: No such parameter directory \"" + params + "\"")

    def _report_single(self, usec):
        print("Inference took %.2f microseconds" % usec)
        print("Classification rate: %.2f images per second" % (1000000.0 / usec))
        self.usecPerImage = usec

    def _report_multi(self, usec, count):
        print("Inference took %.2f microseconds, %.2f usec per image" % (usec * count, usec))
        print("Classification rate: %.2f images per second" % (1000000.0 / usec))
        self.usecPerImage = usec

    def inference(self, path):
        usec = ctypes.c_float(0)
        cls = self.interface.inference(path.encode(), None, len(self.classes), ctypes.byref(usec))
        if cls < 0:
            raise RuntimeError("inference failed: see stderr")
        self._report_single(usec.value)
        return cls

    def detailed_inference(self, path):
        n = len(self.classes)
        details = (ctypes.c_int * max(n, 64))()
        usec = ctypes.c_float(0)
        if self.interface.inference(path.encode(), details, n, ctypes.byref(usec)) < 0:
            raise RuntimeError("inference failed: see stderr")
        self._report_single(usec.value)
        return np.array(details[:n], dtype=np.int32)

    def _collect(self, ptr, count):
        if not ptr:
            raise RuntimeError("inference failed: see stderr")
        arr = np.ctypeslib.as_array(ptr, shape=(count,)).astype(np.int32, copy=True) if count else np.zeros(0, np.int32)
        self.interface.free_results(ptr)
        return arr

    def inference_multiple(self, path):
        size = ctypes.c_int(0)
        usec = ctypes.c_float(0)
        ptr = self.interface.inference_multiple(path.encode(), len(self.classes), ctypes.byref(size),
                                                ctypes.byref(usec), 0)
        result = self._collect(ptr, size.value)
        self._report_multi(usec.value, size.value)
        return result

    def inference_multiple_with_faults(self, path, num_faults, word_size, target_type, target_layers=[]):
        if len(target_layers) == 0:
            targets = None
        else:
            tl = np.array(target_layers, dtype=np.int32)
            targets = tl.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
        size = ctypes.c_int(0)
        usec = ctypes.c_float(0)
        ptr = self.interface.inference_multiple_with_faults(
            path.encode(), len(self.classes), ctypes.byref(size), ctypes.byref(usec), num_faults, word_size,
            target_type, targets, len(target_layers))
        result = self._collect(ptr, size.value)
        self._report_multi(usec.value, size.value)
        return result

    # extension: num_runs independent campaigns in one call, side by side on the GPU
    def inference_multiple_with_faults_runs(self, path, num_runs, num_faults, word_size, target_type, target_layers=[],
                                            seed=0):
        """-> int32 array (num_runs, n): row r is what load_parameters + set_fault_seed(seed + r) +
        inference_multiple_with_faults returns (seed 0: every run seeds from std::random_device).  The loaded
        parameters are not changed.  usecPerImage: device time of the call / (num_runs * n)."""
        tl = np.array(list(target_layers), dtype=np.int32)
        targets = tl.ctypes.data_as(ctypes.POINTER(ctypes.c_int)) if len(tl) else None
        size = ctypes.c_int(0)
        usec = ctypes.c_float(0)
        ptr = self.interface.bnn_mi355x_fault_campaigns(
            path.encode(), len(self.classes), num_runs, seed, num_faults, word_size, target_type, targets, len(tl),
            ctypes.byref(size), ctypes.byref(usec))
        if not ptr:
            raise RuntimeError("fault campaigns failed: " + self.interface.bnn_mi355x_last_error().decode())
        result = self._collect(ptr, num_runs * size.value).reshape(num_runs, size.value)
        self.usecPerImage = usec.value
        return result

    # extension: exhaustive single-fault sweeps (which bits matter)
    def enumerate_faults(self, layer, target, word_size=1):
        """-> int32 array (k, 8): every distinct fault of one layer's weight (target 0) or threshold (target 1)
        memory as records of bnn_mi355x_plan_faults (image 0), ordered by (mem, ind, thresh, bit)."""
        lib = self.interface
        k = lib.bnn_mi355x_enumerate_faults(layer, target, word_size, 0, None, 0)
        if k < 0:
            raise ValueError(lib.bnn_mi355x_last_error().decode())
        recs = np.zeros((k, 8), np.int32)
        for first in range(0, k, 1 << 20):  # (cap_records is an int)
            m = min(1 << 20, k - first)
            lib.bnn_mi355x_enumerate_faults(layer, target, word_size, first,
                                            recs[first:].ctypes.data_as(ctypes.POINTER(ctypes.c_int)), m)
        return recs

    def fault_sweep(self, path, records, max_diffs=None):
        """Every record (8 ints, the image field ignored) alone for every image of `path`: -> (changed, diffs) with
        changed[f] the images whose class differs from the fault-free one and diffs int32 (k, 3) rows {fault, image,
        class} of those images in (fault, image) order (the first max_diffs of them; None: all).  The loaded
        parameters are not changed.  usecPerImage: device time / (faults * images)."""
        lib = self.interface
        recs = np.ascontiguousarray(records, np.int32).reshape(-1, 8)
        nf = recs.shape[0]
        changed = np.zeros(max(nf, 1), np.int32)
        ip = ctypes.POINTER(ctypes.c_int)
        size, usec = ctypes.c_int(0), ctypes.c_float(0)
        cap = (1 << 22) if max_diffs is None else int(max_diffs)
        while True:
            diffs = np.zeros((max(cap, 1), 3), np.int32)
            total = lib.bnn_mi355x_fault_sweep(path.encode(), len(self.classes), recs.ctypes.data_as(ip), nf,
                                               changed.ctypes.data_as(ip), diffs.ctypes.data_as(ip), cap, ctypes.byref(size),
                                               ctypes.byref(usec))
            if total < 0:
                raise RuntimeError("fault sweep failed: " + lib.bnn_mi355x_last_error().decode())
            if max_diffs is not None or total <= cap:
                break
            cap = total  # (all of them asked for, more than guessed: once more with room for every one)
        self.usecPerImage = usec.value
        if nf and size.value:
            print("Fault sweep took %.2f microseconds for %d faults x %d images, %.4f usec per image" % (
                usec.value * nf * size.value, nf, size.value, usec.value))
        return changed[:nf], diffs[:min(cap, total)]

    # extension: activation-fault sweeps (which datapath bits matter)
    def enumerate_act_faults(self, layer):
        """-> int32 array (k, 5): every site x shift of layer `layer`'s output map (any layer but the last) as records
        {layer, y, x, channel, shift}, ordered by (y, x, channel, shift); HWC order of the oracle's layer outputs."""
        lib = self.interface
        k = lib.bnn_mi355x_enumerate_act_faults(layer, 0, None, 0)
        if k < 0:
            raise ValueError(lib.bnn_mi355x_last_error().decode())
        recs = np.zeros((k, 5), np.int32)
        for first in range(0, k, 1 << 20):  # (cap_records is an int)
            m = min(1 << 20, k - first)
            lib.bnn_mi355x_enumerate_act_faults(layer, first, recs[first:].ctypes.data_as(ctypes.POINTER(ctypes.c_int)), m)
        return recs

    def act_fault_sweep(self, path, records, max_diffs=None):
        """Every record {layer, y, x, channel, shift} alone for every image of `path`: that activation of the layer's
        output moved `shift` levels on (mod the levels) while the image is classified.  -> (changed, diffs) as
        fault_sweep returns them.  The loaded parameters are not changed.  usecPerImage: device time / (records *
        images)."""
        lib = self.interface
        recs = np.ascontiguousarray(records, np.int32).reshape(-1, 5)
        nf = recs.shape[0]
        changed = np.zeros(max(nf, 1), np.int32)
        ip = ctypes.POINTER(ctypes.c_int)
        size, usec = ctypes.c_int(0), ctypes.c_float(0)
        cap = (1 << 22) if max_diffs is None else int(max_diffs)
        while True:
            diffs = np.zeros((max(cap, 1), 3), np.int32)
            total = lib.bnn_mi355x_act_fault_sweep(path.encode(), len(self.classes), recs.ctypes.data_as(ip), nf,
                                                   changed.ctypes.data_as(ip), diffs.ctypes.data_as(ip), cap, ctypes.byref(size),
                                                   ctypes.byref(usec))
            if total < 0:
                raise RuntimeError("activation fault sweep failed: " + lib.bnn_mi355x_last_error().decode())
            if max_diffs is not None or total <= cap:
                break
            cap = total  # (all of them asked for, more than guessed: once more with room for every one)
        self.usecPerImage = usec.value
        if nf and size.value:
            print("Activation fault sweep took %.2f microseconds for %d sites x %d images, %.4f usec per image" % (
                usec.value * nf * size.value, nf, size.value, usec.value))
        return changed[:nf], diffs[:min(cap, total)]

    # extension: datapath upset-rate campaigns (every activation upset with probability p)
    def act_noise_rates(self, rates):
        """rates as probabilities in [0, 1) -- a scalar for every layer, or one per layer but the last -- -> uint32 array
        of floor(p * 2^32), the unit of bnn_mi355x_act_noise_campaigns"""
        layers = 8 if self.interface.bnn_mi355x_network().startswith(b"cnv") else 3  # (every layer but the last)
        p = np.full(layers, float(rates)) if np.isscalar(rates) else np.asarray(list(rates), np.float64)
        if p.shape != (layers,) or (p < 0).any() or (p >= 1).any():
            raise ValueError("rates: a probability in [0, 1) for each of the {} layers that have activations".format(layers))
        return np.floor(p * 4294967296.0).astype(np.uint64).astype(np.uint32)

    def inference_multiple_act_noise(self, path, num_runs, rates, seed=0):
        """num_runs independent runs over the images of `path`, every activation of layer L's output upset with
        probability rates[L] (act_noise_rates) before the next layer reads it; run r draws with seed + r (seed 0: every
        run's seed from std::random_device, then in self.act_noise_seeds).  -> (classes int32 (num_runs, n), counts int64
        (num_runs, layers - 1): the sites actually upset per run and layer, over all n images).  The loaded parameters
        are not changed.  usecPerImage: device time of the call / (num_runs * n)."""
        lib = self.interface
        q = np.ascontiguousarray(self.act_noise_rates(rates), np.uint32)
        size, usec = ctypes.c_int(0), ctypes.c_float(0)
        ptr = lib.bnn_mi355x_act_noise_campaigns(path.encode(), len(self.classes), num_runs, seed,
                                                 q.ctypes.data_as(ctypes.POINTER(ctypes.c_uint)), len(q), ctypes.byref(size),
                                                 ctypes.byref(usec))
        if not ptr:
            raise RuntimeError("activation noise campaigns failed: " + lib.bnn_mi355x_last_error().decode())
        result = self._collect(ptr, num_runs * size.value).reshape(num_runs, size.value)
        k = lib.bnn_mi355x_last_act_noise_counts(None, 0)
        counts = (ctypes.c_long * max(k, 1))()
        lib.bnn_mi355x_last_act_noise_counts(counts, k)
        seeds = (ctypes.c_ulonglong * num_runs)()
        lib.bnn_mi355x_last_act_noise_seeds(seeds, num_runs)
        self.act_noise_seeds = list(seeds)
        self.usecPerImage = usec.value
        return result, np.array(counts[:k], np.int64).reshape(num_runs, -1)

    # extension: memory upset-rate campaigns (every bit of the weight / threshold memories upset with probability p)
    def mem_noise_rates(self, rates, thresholds=False):
        """rates as probabilities in [0, 1) -- a scalar for every layer (thresholds: every layer that has threshold memory),
        or one per layer -- -> uint32 array of floor(p * 2^32), the unit of bnn_mi355x_mem_noise_campaigns"""
        cnv = self.interface.bnn_mi355x_network().startswith(b"cnv")
        layers = 9 if cnv else 4
        p = np.full(layers, float(rates)) if np.isscalar(rates) else np.asarray(list(rates), np.float64)
        if np.isscalar(rates) and thresholds and cnv:
            p[8] = 0.0  # (CNV layer 8 passes its accumulators through: no threshold memory)
        if p.shape != (layers,) or (p < 0).any() or (p >= 1).any():
            raise ValueError("rates: a probability in [0, 1) for each of the {} layers".format(layers))
        return np.floor(p * 4294967296.0).astype(np.uint64).astype(np.uint32)

    # the families of parameter-memory upset campaigns, by the stem of bnn_mi355x_<stem>_campaigns and
    # bnn_mi355x_last_<stem>_counts / _seeds: the words of the family's error, the last axes of its counts per layer
    _UPSET_FAMILIES = {"mem_noise": ("memory noise", (2,)), "hardened_mem_noise": ("hardened memory noise", (2, 2)),
                       "exposure": ("exposure", (2, 2)), "ecc_exposure": ("ecc exposure", (6,)), "repair_exposure": ("repair exposure", (8,)),
                       "wecc_exposure": ("wecc exposure", (12,)), "iwecc_exposure": ("iwecc exposure", (12,))}

    def _upset_campaign(self, family, path, num_runs, rates_w, rates_t, seed, lead_args=(), tail_args=()):
        """One call of bnn_mi355x_<family>_campaigns, whose arguments are (path, classes, *lead_args: the memory
        organisation, num_runs, seed, the two rate arrays, their length, *tail_args: epoch_images first where the family
        has epochs, image_number, usecPerImage).  -> (classes int32 (num_runs, n), counts int64 (num_runs, [epochs,]
        layers) + the family's last axes); the seeds go to self.mem_noise_seeds, the time to self.usecPerImage."""
        lib = self.interface
        words, counts_tail = self._UPSET_FAMILIES[family]
        qw = np.ascontiguousarray(self.mem_noise_rates(rates_w), np.uint32)
        qt = np.ascontiguousarray(self.mem_noise_rates(rates_t, thresholds=True), np.uint32)
        up = ctypes.POINTER(ctypes.c_uint)
        size, usec = ctypes.c_int(0), ctypes.c_float(0)
        ptr = getattr(lib, "bnn_mi355x_{}_campaigns".format(family))(
            path.encode(), len(self.classes), *lead_args, num_runs, seed, qw.ctypes.data_as(up), qt.ctypes.data_as(up), len(qw), *tail_args,
            ctypes.byref(size), ctypes.byref(usec))
        if not ptr:
            raise RuntimeError(words + " campaigns failed: " + lib.bnn_mi355x_last_error().decode())
        result = self._collect(ptr, num_runs * size.value).reshape(num_runs, size.value)
        last_counts = getattr(lib, "bnn_mi355x_last_{}_counts".format(family))
        k = last_counts(None, 0)
        counts = (ctypes.c_long * max(k, 1))()
        last_counts(counts, k)
        seeds = (ctypes.c_ulonglong * num_runs)()
        getattr(lib, "bnn_mi355x_last_{}_seeds".format(family))(seeds, num_runs)
        self.mem_noise_seeds = list(seeds)
        self.usecPerImage = usec.value
        epochs = (-(-size.value // tail_args[0]),) if tail_args else ()  # (the last epoch may be short)
        return result, np.array(counts[:k], np.int64).reshape((num_runs,) + epochs + (len(qw),) + counts_tail)

    def inference_multiple_mem_noise(self, path, num_runs, rates_w, rates_t, seed=0, scheme=None, burst=1):
        """scheme (0 none, 1 TMR, 2 interleaved, 3 resilient-interleaved) or burst > 1: the hardened form,
        inference_multiple_hardened_mem_noise.  Else num_runs independent runs over the images of `path`, every bit of layer L's weight memory flipped with
        probability rates_w[L] and every bit of its threshold memory with rates_t[L] (mem_noise_rates), in place from the
        first image on; run r draws with seed + r (seed 0: every run's seed from std::random_device, then in
        self.mem_noise_seeds).  -> (classes int32 (num_runs, n), counts int64 (num_runs, layers, 2): the flips actually
        applied per run, layer and memory kind (0 weights, 1 thresholds)).  The loaded parameters are not changed.
        usecPerImage: device time of the call / (num_runs * n)."""
        if scheme is not None or burst != 1:
            return self.inference_multiple_hardened_mem_noise(path, num_runs, rates_w, rates_t, scheme or 0, burst, seed)
        return self._upset_campaign("mem_noise", path, num_runs, rates_w, rates_t, seed)

    # extension: hardened memory schemes in the memory upset campaigns (TMR, interleaved thresholds; bursts)
    def hardening_layout(self, scheme):
        """-> int array (layers, 3): weight modules, threshold modules, threshold interleave (0 / 2 / 3) per layer of this
        network under `scheme`; RuntimeError with the reason for a (network, scheme) pair that is not modelled"""
        lib = self.interface
        out = (ctypes.c_int * 3)()
        rows = []
        for layer in range(len(self.mem_noise_rates(0.0))):
            if lib.bnn_mi355x_hardening_layout(scheme, layer, out) != 0:
                raise RuntimeError(lib.bnn_mi355x_last_error().decode())
            rows.append(list(out))
        return np.array(rows, np.int32)

    def inference_multiple_hardened_mem_noise(self, path, num_runs, rates_w, rates_t, scheme, burst=1, seed=0):
        """inference_multiple_mem_noise on the PHYSICAL memories of a hardened overlay: `scheme` 0 none, 1 TMR (three
        modules of layer 0's weights and of the thresholds of layers 0-4, bitwise majority), 2 / 3 (resilient-)interleaved
        threshold lines; an event flips `burst` (1 ... 16) adjacent physical bits of one memory word of one module, with
        probability rates_w[L] / rates_t[L] per aligned group.  -> (classes int32 (num_runs, n), counts int64 (num_runs,
        layers, 2: weights, thresholds, 2: physical bits flipped, logical bits that differ after voting and
        de-interleaving)).  The seeds are left in self.mem_noise_seeds."""
        return self._upset_campaign("hardened_mem_noise", path, num_runs, rates_w, rates_t, seed, (scheme, burst))

    # extension: exposure campaigns (upsets that accumulate over epochs of images, with scrubbing)
    def inference_multiple_exposure(self, path, num_runs, rates_w, rates_t, epoch_images, scrub_every=0, scheme=0, burst=1, seed=0, code=0,
                                    repair_every=0, weight_code=0, weight_interleave=0):
        """inference_multiple_hardened_mem_noise spread over time: the run is cut into epochs of `epoch_images` images, the
        rates are per epoch, an epoch's upsets XOR onto the physical state the earlier ones left, and before every epoch
        t > 0 with t % scrub_every == 0 (0: never) all memories are rewritten from the loaded parameters.  -> (classes
        int32 (num_runs, n), counts int64 (num_runs, epochs, layers, 2: weights, thresholds, 2: physical bits flipped in
        the epoch, logical bits that differ from the loaded parameters after it)).  The seeds are left in
        self.mem_noise_seeds.  code 1 (SEC-DED coded 16-bit threshold memories): inference_multiple_ecc_exposure;
        repair_every > 0 (repair scrubs): inference_multiple_repair_exposure; weight_code 1 (SEC-DED (72,64) coded weight
        memories): inference_multiple_wecc_exposure; weight_interleave 1 (their code words column-interleaved):
        inference_multiple_iwecc_exposure."""
        if weight_interleave:
            return self.inference_multiple_iwecc_exposure(path, num_runs, rates_w, rates_t, epoch_images, scrub_every, repair_every, scheme, code,
                                                          weight_code, weight_interleave, burst, seed)
        if weight_code:
            return self.inference_multiple_wecc_exposure(path, num_runs, rates_w, rates_t, epoch_images, scrub_every, repair_every, scheme, code,
                                                         weight_code, burst, seed)
        if repair_every:
            return self.inference_multiple_repair_exposure(path, num_runs, rates_w, rates_t, epoch_images, scrub_every, repair_every, scheme, code,
                                                           burst, seed)
        if code:
            return self.inference_multiple_ecc_exposure(path, num_runs, rates_w, rates_t, epoch_images, scrub_every, scheme, code, burst, seed)
        return self._upset_campaign("exposure", path, num_runs, rates_w, rates_t, seed, (scheme, burst), (epoch_images, scrub_every))

    # extension: SEC-DED coded threshold memories in the exposure campaigns
    def inference_multiple_ecc_exposure(self, path, num_runs, rates_w, rates_t, epoch_images, scrub_every=0, scheme=0, code=1, burst=1, seed=0):
        """inference_multiple_exposure with the 16-bit threshold memories protected by a SEC-DED code (`code` 1; 0: none):
        Hamming(21,16) plus an overall parity bit, the 6 check bits of an element in a check memory of their own that takes
        upsets at the threshold rate; `scheme` 0 or 2 (interleaved: a burst becomes single errors of two code words).
        Weights and the 24-bit thresholds of CNV layer 0 are not coded.  -> (classes int32 (num_runs, n), counts int64
        (num_runs, epochs, layers, 6: weights physical, logical; thresholds physical (data plus check), logical (after
        decoding); threshold words corrected; detected as uncorrectable)).  The seeds are left in self.mem_noise_seeds."""
        return self._upset_campaign("ecc_exposure", path, num_runs, rates_w, rates_t, seed, (scheme, code, burst), (epoch_images, scrub_every))

    # extension: repair scrubs in the exposure campaigns
    def inference_multiple_repair_exposure(self, path, num_runs, rates_w, rates_t, epoch_images, scrub_every=0, repair_every=1, scheme=0, code=0,
                                           burst=1, seed=0):
        """inference_multiple_ecc_exposure with the scrub a TMR or coded memory really has: before every epoch t > 0 with
        t % repair_every == 0 (0: never) that is no rewrite epoch (t % scrub_every == 0), every memory with redundancy is
        read, voted (TMR: the bitwise majority written to all three modules) or decoded (SEC-DED: a status-1 word written
        back with fresh check bits) and written back.  Memories without redundancy keep accumulating upsets, and what the
        redundancy gets wrong (a bit hit in two modules, an accepted triple error) is locked in.  -> (classes int32
        (num_runs, n), counts int64 (num_runs, epochs, layers, 8: the six of inference_multiple_ecc_exposure, the words
        the epoch's repair rewrote, the words of the repaired memories still unlike the loaded ones after it)).  The seeds
        are left in self.mem_noise_seeds."""
        return self._upset_campaign("repair_exposure", path, num_runs, rates_w, rates_t, seed, (scheme, code, burst),
                                    (epoch_images, scrub_every, repair_every))

    # extension: SEC-DED (72,64) coded weight memories in the exposure campaigns
    def inference_multiple_wecc_exposure(self, path, num_runs, rates_w, rates_t, epoch_images, scrub_every=0, repair_every=0, scheme=0, code=0,
                                         weight_code=1, burst=1, seed=0):
        """inference_multiple_repair_exposure with the weight memories of every layer but CNV layer 0 protected by a SEC-DED
        code (`weight_code` 1; 0: none): Hamming(71,64) plus an overall parity bit over every 64 sites of the memory, the 8
        check bits of a code word in a check memory of the layer's own that takes upsets at the weight rate.  A repair epoch
        also rewrites the status-1 code words.  Goes with every (scheme, code) the repair campaign accepts, TMR included.
        -> (classes int32 (num_runs, n), counts int64 (num_runs, epochs, layers, 12: the eight of
        inference_multiple_repair_exposure -- weights physical counts data plus check bits, weights logical the data bits
        that differ after decoding -- then the weight code words corrected, detected as uncorrectable, rewritten by the
        epoch's repair, still unlike the loaded ones after it)).  The seeds are left in self.mem_noise_seeds."""
        return self._upset_campaign("wecc_exposure", path, num_runs, rates_w, rates_t, seed, (scheme, code, weight_code, burst),
                                    (epoch_images, scrub_every, repair_every))

    # extension: column-interleaved code words over the coded weight memories
    def inference_multiple_iwecc_exposure(self, path, num_runs, rates_w, rates_t, epoch_images, scrub_every=0, repair_every=0, scheme=0, code=0,
                                          weight_code=1, weight_interleave=1, burst=1, seed=0):
        """inference_multiple_wecc_exposure with the (72,64) code words of a layer's weight memory COLUMN-INTERLEAVED
        (`weight_interleave` 1; 0: not, and then this is inference_multiple_wecc_exposure's result): at depth D = gcd(16,
        code words per PE) adjacent columns of a memory word lie in D different code words, so a burst of up to D bits
        is D single errors, each corrected -- where without it an aligned burst of 2 is a double error of one code word
        and nothing is corrected.  The weights stay where they were and the upsets are the same events; only which code
        word a bit belongs to changes.  Needs weight_code 1.  -> (classes int32 (num_runs, n), counts int64 (num_runs,
        epochs, layers, 12) as inference_multiple_wecc_exposure, the code words counted after gathering).  The seeds are
        left in self.mem_noise_seeds."""
        return self._upset_campaign("iwecc_exposure", path, num_runs, rates_w, rates_t, seed, (scheme, code, weight_code, weight_interleave, burst),
                                    (epoch_images, scrub_every, repair_every))

    # extension: input-buffer faults (which pixel bits matter; the accuracy at input-buffer upset rate p)
    def enumerate_input_faults(self):
        """-> int32 array (image_bytes * 8, 2): every bit of the input image as records {byte, bit} in site order (byte in
        the layout of inference_array: CNV planar CHW, LFC row-major; bit 0 the LSB)."""
        lib = self.interface
        k = lib.bnn_mi355x_enumerate_input_faults(0, None, 0)
        recs = np.zeros((k, 2), np.int32)
        lib.bnn_mi355x_enumerate_input_faults(0, recs.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), k)
        return recs

    def input_fault_sweep(self, path, records, max_diffs=None):
        """Every record {byte, bit} alone for every image of `path`: that bit of the image flipped while it is
        classified.  -> (changed, diffs) as fault_sweep returns them.  The loaded parameters are not changed.
        usecPerImage: device time / (records * images)."""
        lib = self.interface
        recs = np.ascontiguousarray(records, np.int32).reshape(-1, 2)
        nf = recs.shape[0]
        changed = np.zeros(max(nf, 1), np.int32)
        ip = ctypes.POINTER(ctypes.c_int)
        size, usec = ctypes.c_int(0), ctypes.c_float(0)
        cap = (1 << 22) if max_diffs is None else int(max_diffs)
        while True:
            diffs = np.zeros((max(cap, 1), 3), np.int32)
            total = lib.bnn_mi355x_input_fault_sweep(path.encode(), len(self.classes), recs.ctypes.data_as(ip), nf,
                                                     changed.ctypes.data_as(ip), diffs.ctypes.data_as(ip), cap, ctypes.byref(size),
                                                     ctypes.byref(usec))
            if total < 0:
                raise RuntimeError("input fault sweep failed: " + lib.bnn_mi355x_last_error().decode())
            if max_diffs is not None or total <= cap:
                break
            cap = total  # (all of them asked for, more than guessed: once more with room for every one)
        self.usecPerImage = usec.value
        if nf and size.value:
            print("Input fault sweep took %.2f microseconds for %d sites x %d images, %.4f usec per image" % (
                usec.value * nf * size.value, nf, size.value, usec.value))
        return changed[:nf], diffs[:min(cap, total)]

    def inference_multiple_input_noise(self, path, num_runs, rate, seed=0):
        """num_runs independent runs over the images of `path`, every bit of every image flipped with probability `rate`
        (in [0, 1); floor(rate * 2^32) is what the library takes) while that image is classified; run r draws with seed + r
        (seed 0: every run's seed from std::random_device, then in self.input_noise_seeds).  -> (classes int32 (num_runs,
        n), counts int64 (num_runs,): the bits actually flipped per run, over all n images).  The loaded parameters are not
        changed.  usecPerImage: device time of the call / (num_runs * n)."""
        lib = self.interface
        if not 0.0 <= float(rate) < 1.0:
            raise ValueError("rate: a probability in [0, 1)")
        q = int(np.floor(float(rate) * 4294967296.0))
        size, usec = ctypes.c_int(0), ctypes.c_float(0)
        ptr = lib.bnn_mi355x_input_noise_campaigns(path.encode(), len(self.classes), num_runs, seed, q, ctypes.byref(size),
                                                   ctypes.byref(usec))
        if not ptr:
            raise RuntimeError("input noise campaigns failed: " + lib.bnn_mi355x_last_error().decode())
        result = self._collect(ptr, num_runs * size.value).reshape(num_runs, size.value)
        counts = (ctypes.c_long * num_runs)()
        lib.bnn_mi355x_last_input_noise_counts(counts, num_runs)
        seeds = (ctypes.c_ulonglong * num_runs)()
        lib.bnn_mi355x_last_input_noise_seeds(seeds, num_runs)
        self.input_noise_seeds = list(seeds)
        self.usecPerImage = usec.value
        return result, np.array(counts[:num_runs], np.int64)

    # extension: propagation profiles of the single-fault sweeps (where a fault is masked)
    def sweep_profile(self, enable):
        """True: fault_sweep, act_fault_sweep and input_fault_sweep called from now on also record, per record and layer,
        the images and the activations that differ from the fault-free ones (last_sweep_profile).  -> the previous
        setting.  The setting belongs to the library, which outlives this object."""
        return bool(self.interface.bnn_mi355x_sweep_profile(1 if enable else 0))

    def last_sweep_profile(self):
        """The profile of the last sweep that ran with profiling on -> (alive, flipped), int64 arrays of shape
        (records, layers - 1) in the order of that call's records.  alive[f, l]: the images whose layer-l output (CNV layers
        1 and 3: after the max-pool) differs from the fault-free one; flipped[f, l]: the activations that differ, summed
        over those images.  Columns before the first layer the sweep evaluates for a record (a parameter fault's layer,
        the layer after an activation site, layer 0 for an input bit) are 0."""
        lib = self.interface
        cols = ctypes.c_int(0)
        rows = lib.bnn_mi355x_last_sweep_profile(0, None, None, 0, ctypes.byref(cols))
        if rows < 0:
            raise RuntimeError(lib.bnn_mi355x_last_error().decode())
        alive = np.zeros((rows, cols.value), np.int64)
        flipped = np.zeros((rows, cols.value), np.int64)
        lp = ctypes.POINTER(ctypes.c_long)
        lib.bnn_mi355x_last_sweep_profile(0, alive.ctypes.data_as(lp), flipped.ctypes.data_as(lp), rows, None)
        return alive, flipped

    def inference_multiple_detail(self, path):
        size = ctypes.c_int(0)
        usec = ctypes.c_float(0)
        ptr = self.interface.inference_multiple(path.encode(), len(self.classes), ctypes.byref(size),
                                                ctypes.byref(usec), 1)
        result = self._collect(ptr, size.value * len(self.classes))
        self._report_multi(usec.value, size.value)
        return result

    # -- extension: images already in memory ----------------------------------
    def inference_array(self, images, detail=False):
        """images: uint8 array, n x 3072 (planar CHW) for cnv*, n x 784 for lfc*"""
        if not self.interface.has_extensions:
            raise RuntimeError("this runtime library has no in-memory entry point")
        isz = self.interface.bnn_mi355x_image_bytes()
        a = np.ascontiguousarray(images, dtype=np.uint8).reshape(-1, isz)
        usec = ctypes.c_float(0)
        ptr = self.interface.bnn_mi355x_inference_buffer(a.ctypes.data, a.shape[0], len(self.classes),
                                                         ctypes.byref(usec), 1 if detail else 0)
        count = a.shape[0] * (len(self.classes) if detail else 1)
        result = self._collect(ptr, count)
        self.usecPerImage = usec.value
        return result

    def class_name(self, index):
        return self.classes[index]


class CnvClassifier:
    """CNV networks on CIFAR-10 formatted (32x32x3) images."""

    def __init__(self, network, params, runtime=RUNTIME_HW):
        if params in available_params(network):
            self.net = network
            self.params = params
            self.runtime = runtime
            self.usecPerImage = 0.0
            self.bnn = PynqBNN(runtime, network)
            self.bnn.load_parameters(os.path.join(params, network))
            self.classes = self.bnn.classes
        else:
            print("ERROR: parameters are not availlable for {0}".format(network))

    def image_to_cifar(self, img, fp):
        """append one CIFAR-10 record (label byte + R, G, B planes) for `img`.

        Same procedure as the reference (thumbnail to 32x32 with the ANTIALIAS
        = LANCZOS filter from the full-resolution image, centred on a
        transparent white canvas).  `reducing_gap=None` keeps modern Pillow
        from pre-shrinking JPEGs, which is what reproduces
        tests/Test_image/deer.bin."""
        img.thumbnail((32, 32), Image.LANCZOS, reducing_gap=None)
        canvas = Image.new("RGBA", (32, 32), (255, 255, 255, 0))
        canvas.paste(img, (int((32 - img.size[0]) / 2), int((32 - img.size[1]) / 2)))
        px = np.array(canvas)
        fp.write(np.identity(1, dtype=np.uint8).tobytes())
        for ch in range(3):
            fp.write(px[:, :, ch].flatten().tobytes())

    def images_to_cifar(self, imgs):
        """CIFAR-10 records (uint8 array [n, 3073]) of a list of PIL images (or decoded pictures as
        uint8 arrays [H, W, 3] / [H, W, 4] / [H, W], which skips the PIL -> numpy copy), the resampling done on
        the GPU (``bnn_mi355x_images_to_cifar``): same bytes as :meth:`image_to_cifar` writes, but
        the caller's images are left as they are (the reference's ``thumbnail`` shrinks them in
        place).  Modes other than RGB, RGBA and L (palette, LA, ...) take the PIL route on the host."""
        import io
        from concurrent.futures import ThreadPoolExecutor
        recs = np.empty((len(imgs), 3073), dtype=np.uint8)
        # a library with only the reference's six symbols (the reference's own .so) has no such entry point
        on_device = hasattr(self.bnn.interface, "bnn_mi355x_images_to_cifar")

        def decoded(img):
            """uint8 array for the device route, None for the PIL route"""
            if isinstance(img, np.ndarray):  # a decoded picture
                if img.dtype != np.uint8 or not (img.ndim == 2 or (img.ndim == 3 and img.shape[2] in (3, 4))):
                    raise ValueError("pictures given as arrays must be uint8 [H, W, 3] (RGB), [H, W, 4] (RGBA) or [H, W] (L)")
                return np.ascontiguousarray(img) if on_device else None
            if on_device and img.mode in ("RGB", "RGBA", "L"):
                return np.ascontiguousarray(np.asarray(img))  # (decodes lazily opened files: PIL releases the GIL there)
            return None

        # a bounded number of decoded pictures in memory at a time; decoding on a few threads
        CHUNK = 32
        with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
            for base in range(0, len(imgs), CHUNK):
                part = imgs[base:base + CHUNK]
                arrays = list(pool.map(decoded, part)) if len(part) > 1 else [decoded(part[0])]
                dev = [(base + i, a) for i, a in enumerate(arrays) if a is not None]
                for i, a in enumerate(arrays):
                    if a is None:  # the reference's own procedure, on the host
                        img = part[i]
                        buf = io.BytesIO()
                        self.image_to_cifar(Image.fromarray(img) if isinstance(img, np.ndarray) else img.copy(), buf)
                        recs[base + i] = np.frombuffer(buf.getvalue(), dtype=np.uint8)
                n = len(dev)
                if n:
                    arrs = [a for _, a in dev]
                    ptrs = (ctypes.c_void_p * n)(*[a.ctypes.data for a in arrs])
                    ws = (ctypes.c_int * n)(*[a.shape[1] for a in arrs])
                    hs = (ctypes.c_int * n)(*[a.shape[0] for a in arrs])
                    bs = (ctypes.c_int * n)(*[1 if a.ndim == 2 else a.shape[2] for a in arrs])
                    out = np.empty((n, 3073), dtype=np.uint8)
                    lib = self.bnn.interface
                    if lib.bnn_mi355x_images_to_cifar(ptrs, ws, hs, bs, None, n, out.ctypes.data) != 0:
                        raise RuntimeError(lib.bnn_mi355x_last_error().decode())
                    recs[[i for i, _ in dev]] = out
        return recs

    def _with_tmp(self, imgs, fn):
        with tempfile.NamedTemporaryFile() as tmp:
            tmp.write(self.images_to_cifar(list(imgs)).tobytes())
            tmp.flush()
            result = fn(tmp.name)
        self.usecPerImage = self.bnn.usecPerImage
        return result

    def classify_image(self, img):
        return self._with_tmp([img], self.bnn.inference)

    def classify_cifar(self, path):
        result = self.bnn.inference(path)
        self.usecPerImage = self.bnn.usecPerImage
        return result

    def classify_image_details(self, img):
        return self._with_tmp([img], self.bnn.detailed_inference)

    def classify_cifar_details(self, path):
        result = self.bnn.detailed_inference(path)
        self.usecPerImage = self.bnn.usecPerImage
        return result

    def classify_path(self, path):
        return self.classify_image(Image.open(path))

    def classify_images(self, imgs):
        return self._with_tmp(imgs, self.bnn.inference_multiple)

    def classify_images_with_faults(self, imgs, num_faults, word_size, target_type, target_layers=[]):
        return self._with_tmp(imgs, lambda p: self.bnn.inference_multiple_with_faults(
            p, num_faults, word_size, target_type, target_layers))

    def classify_images_with_faults_runs(self, imgs, num_runs, num_faults, word_size, target_type, target_layers=[], seed=0):
        return self._with_tmp(imgs, lambda p: self.bnn.inference_multiple_with_faults_runs(
            p, num_runs, num_faults, word_size, target_type, target_layers, seed))

    def classify_cifars(self, path):
        result = self.bnn.inference_multiple(path)
        self.usecPerImage = self.bnn.usecPerImage
        return result

    def classify_cifars_with_faults(self, path, num_faults, word_size, target_type, target_layers=[]):
        result = self.bnn.inference_multiple_with_faults(path, num_faults, word_size, target_type, target_layers)
        self.usecPerImage = self.bnn.usecPerImage
        return result

    def classify_cifars_with_faults_runs(self, path, num_runs, num_faults, word_size, target_type, target_layers=[], seed=0):
        result = self.bnn.inference_multiple_with_faults_runs(path, num_runs, num_faults, word_size, target_type,
                                                              target_layers, seed)
        self.usecPerImage = self.bnn.usecPerImage
        return result

    # extension: exhaustive single-fault sweeps (PynqBNN.fault_sweep)
    def classify_images_fault_sweep(self, imgs, records, max_diffs=None):
        return self._with_tmp(imgs, lambda p: self.bnn.fault_sweep(p, records, max_diffs))

    def classify_cifars_fault_sweep(self, path, records, max_diffs=None):
        result = self.bnn.fault_sweep(path, records, max_diffs)
        self.usecPerImage = self.bnn.usecPerImage
        return result

    def classify_images_act_fault_sweep(self, imgs, records, max_diffs=None):
        return self._with_tmp(imgs, lambda p: self.bnn.act_fault_sweep(p, records, max_diffs))

    def classify_cifars_act_fault_sweep(self, path, records, max_diffs=None):
        result = self.bnn.act_fault_sweep(path, records, max_diffs)
        self.usecPerImage = self.bnn.usecPerImage
        return result

    # extension: datapath upset-rate campaigns (PynqBNN.inference_multiple_act_noise)
    def classify_images_act_noise(self, imgs, num_runs, rates, seed=0):
        return self._with_tmp(imgs, lambda p: self.bnn.inference_multiple_act_noise(p, num_runs, rates, seed))

    def classify_cifars_act_noise(self, path, num_runs, rates, seed=0):
        result = self.bnn.inference_multiple_act_noise(path, num_runs, rates, seed)
        self.usecPerImage = self.bnn.usecPerImage
        return result

    # extension: memory upset-rate campaigns (PynqBNN.inference_multiple_mem_noise)
    def classify_images_mem_noise(self, imgs, num_runs, rates_w, rates_t, seed=0, scheme=None, burst=1):
        return self._with_tmp(imgs, lambda p: self.bnn.inference_multiple_mem_noise(p, num_runs, rates_w, rates_t, seed, scheme, burst))

    def classify_cifars_mem_noise(self, path, num_runs, rates_w, rates_t, seed=0, scheme=None, burst=1):
        result = self.bnn.inference_multiple_mem_noise(path, num_runs, rates_w, rates_t, seed, scheme, burst)
        self.usecPerImage = self.bnn.usecPerImage
        return result

    # extension: exposure campaigns (PynqBNN.inference_multiple_exposure)
    def classify_images_exposure(self, imgs, *args, **kwargs):
        return self._with_tmp(imgs, lambda p: self.bnn.inference_multiple_exposure(p, *args, **kwargs))

    def classify_cifars_exposure(self, path, *args, **kwargs):
        result = self.bnn.inference_multiple_exposure(path, *args, **kwargs)
        self.usecPerImage = self.bnn.usecPerImage
        return result

    # extension: input-buffer faults (PynqBNN.input_fault_sweep, PynqBNN.inference_multiple_input_noise)
    def classify_images_input_fault_sweep(self, imgs, records, max_diffs=None):
        return self._with_tmp(imgs, lambda p: self.bnn.input_fault_sweep(p, records, max_diffs))

    def classify_cifars_input_fault_sweep(self, path, records, max_diffs=None):
        result = self.bnn.input_fault_sweep(path, records, max_diffs)
        self.usecPerImage = self.bnn.usecPerImage
        return result

    def classify_images_input_noise(self, imgs, num_runs, rate, seed=0):
        return self._with_tmp(imgs, lambda p: self.bnn.inference_multiple_input_noise(p, num_runs, rate, seed))

    def classify_cifars_input_noise(self, path, num_runs, rate, seed=0):
        result = self.bnn.inference_multiple_input_noise(path, num_runs, rate, seed)
        self.usecPerImage = self.bnn.usecPerImage
        return result

    def classify_images_details(self, imgs):
        return self._with_tmp(imgs, self.bnn.inference_multiple_detail)

    def classify_cifars_details(self, path):
        result = self.bnn.inference_multiple_detail(path)
        self.usecPerImage = self.bnn.usecPerImage
        return result

    def classify_paths(self, paths):
        return self.classify_images([Image.open(p) for p in paths])

    # -- extension: every window of one scene in one call (CNV-BNN_Road-Signs.ipynb cells 13-16) ----------
    def tile_boxes(self, size, sizes=(64, 96)):
        """the notebook's tiling of a picture of ``size`` = (width, height): for each window size in ``sizes`` (size-major,
        like cell 13) windows every ``s // 4`` pixels, rows outer, columns inner, kept when ``right <= width and lower <
        height`` -> list of (left, upper, right, lower), what ``Image.crop`` takes"""
        width, height = size
        lib = self.bnn.interface
        bounds = []
        for s in sizes:
            if hasattr(lib, "bnn_mi355x_tile_boxes"):
                n = lib.bnn_mi355x_tile_boxes(width, height, s, None, 0)
                if n < 0:
                    raise ValueError(lib.bnn_mi355x_last_error().decode())
                out = np.zeros((n, 4), np.int32)
                lib.bnn_mi355x_tile_boxes(width, height, s, out.ctypes.data, n)
                bounds += [tuple(int(v) for v in b) for b in out]
            else:  # a library without the symbol: cell 13 as it stands
                stride = s // 4
                for j in range(height // stride):
                    for i in range(width // stride):
                        b = (stride * i, stride * j, stride * i + s, stride * j + s)
                        if b[2] <= width and b[3] < height:
                            bounds.append(b)
        return bounds

    def _scene(self, img):
        """(uint8 array for the device route or None for the PIL route, PIL image or None)"""
        if isinstance(img, np.ndarray):
            if img.dtype != np.uint8 or not (img.ndim == 2 or (img.ndim == 3 and img.shape[2] in (3, 4))):
                raise ValueError("pictures given as arrays must be uint8 [H, W, 3] (RGB), [H, W, 4] (RGBA) or [H, W] (L)")
            return np.ascontiguousarray(img), None
        if img.mode in ("RGB", "RGBA", "L"):
            return np.ascontiguousarray(np.asarray(img)), img
        return None, img

    @staticmethod
    def _boxes(boxes):
        b = np.ascontiguousarray(np.asarray(boxes, dtype=np.int32).reshape(-1, 4))
        return b

    def windows_to_cifar(self, img, boxes):
        """CIFAR-10 records (uint8 array [n, 3073]) of the windows ``boxes`` (left, upper, right, lower) of ONE picture
        (a PIL image or a uint8 array, as in :meth:`images_to_cifar`): the same bytes as :meth:`image_to_cifar` writes
        for ``img.crop(box)``, made on the GPU from one upload of the picture (``bnn_mi355x_windows_to_cifar``).  Modes
        other than RGB, RGBA and L, and a library without the entry point, take :meth:`images_to_cifar` on the crops.
        The caller's image is left as it is."""
        lib = self.bnn.interface
        a, pil = self._scene(img)
        b = self._boxes(boxes)
        if a is None or not hasattr(lib, "bnn_mi355x_windows_to_cifar"):
            pil = pil if pil is not None else Image.fromarray(a)
            return self.images_to_cifar([pil.crop(tuple(int(v) for v in box)) for box in b])
        recs = np.empty((len(b), 3073), dtype=np.uint8)
        bands = 1 if a.ndim == 2 else a.shape[2]
        if lib.bnn_mi355x_windows_to_cifar(a.ctypes.data, a.shape[1], a.shape[0], bands, 0, b.ctypes.data, len(b), recs.ctypes.data) != 0:
            raise RuntimeError(lib.bnn_mi355x_last_error().decode())
        return recs

    def _classify_windows(self, img, boxes, detail):
        lib = self.bnn.interface
        a, pil = self._scene(img)
        b = self._boxes(boxes)
        if a is None or not hasattr(lib, "bnn_mi355x_classify_windows"):
            pil = pil if pil is not None else Image.fromarray(a)
            crops = [pil.crop(tuple(int(v) for v in box)) for box in b]
            return self.classify_images_details(crops) if detail else self.classify_images(crops)
        bands = 1 if a.ndim == 2 else a.shape[2]
        usec, pre = ctypes.c_float(0), ctypes.c_float(0)
        ptr = lib.bnn_mi355x_classify_windows(a.ctypes.data, a.shape[1], a.shape[0], bands, 0, b.ctypes.data, len(b), len(self.classes),
                                              ctypes.byref(usec), ctypes.byref(pre), 1 if detail else 0)
        if not ptr:
            raise RuntimeError(lib.bnn_mi355x_last_error().decode())
        result = self.bnn._collect(ptr, len(b) * (len(self.classes) if detail else 1))
        self.usecPerImage = self.bnn.usecPerImage = usec.value
        self.usecPreprocess = pre.value
        return result

    def classify_windows(self, img, boxes):
        """what :meth:`classify_images` returns for ``[img.crop(b) for b in boxes]``; the picture goes to the GPU once
        and the records never leave it (``bnn_mi355x_classify_windows``)"""
        return self._classify_windows(img, boxes, False)

    def classify_windows_details(self, img, boxes):
        """what :meth:`classify_images_details` returns for the crops: ``len(classes)`` scores per window"""
        return self._classify_windows(img, boxes, True)

    # -- extension: the dense scan -- every 32 x 32 window at stride 4 from one pass over the picture ----------
    def _scan_lib(self):
        """the library when it scans on the device (cnvW1A1 with the ``bnn_mi355x_scan_*`` symbols), else None"""
        lib = self.bnn.interface
        if hasattr(lib, "bnn_mi355x_scan_scene") and lib.bnn_mi355x_network().decode().split("-")[0] == NETWORK_CNVW1A1:
            return lib
        return None

    @staticmethod
    def _as_pil(img):
        return Image.fromarray(img) if isinstance(img, np.ndarray) else img

    @staticmethod
    def _planes(pil):
        """planar uint8 [3, H, W] as a window's record holds the picture (L: the grey plane three times)"""
        if pil.mode == "L":
            return np.ascontiguousarray(np.broadcast_to(np.asarray(pil)[None], (3,) + pil.size[::-1]))
        a = np.asarray(pil if pil.mode == "RGB" else pil.convert("RGBA"))[:, :, :3]
        return np.ascontiguousarray(a.transpose(2, 0, 1))

    def _scan_planes(self, planes, details):
        """[ny, nx] classes or [ny, nx, len(classes)] scores of a planar picture"""
        _, h, w = planes.shape
        if w < 32 or h < 32:
            raise ValueError("scan: need a picture of 32 x 32 pixels or more")
        nx, ny = (w - 32) // 4 + 1, (h - 32) // 4 + 1
        ncls = len(self.classes)
        lib = self._scan_lib()
        if lib is None:  # the same records through the per-window pass: the same answers by construction
            recs = np.stack([planes[:, 4 * j:4 * j + 32, 4 * i:4 * i + 32].reshape(3072) for j in range(ny) for i in range(nx)])
            res = np.asarray(self.classify_array(recs, detail=details))
        else:
            gx, gy, usec = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_float(0)
            ptr = lib.bnn_mi355x_scan_planes(planes.ctypes.data, w, h, ncls, ctypes.byref(gx), ctypes.byref(gy), ctypes.byref(usec),
                                             1 if details else 0)
            if not ptr:
                raise RuntimeError(lib.bnn_mi355x_last_error().decode())
            res = self.bnn._collect(ptr, nx * ny * (ncls if details else 1))
            self.usecPerImage = self.bnn.usecPerImage = usec.value
        return res.reshape((ny, nx, ncls) if details else (ny, nx))

    def scan(self, img, details=False):
        """the class (or, with ``details``, the ``len(classes)`` scores) of EVERY 32 x 32 window of ``img`` at stride 4:
        entry [j, i] is what :meth:`classify_array` returns for the record cut at columns 4i .. 4i + 31, rows 4j .. 4j + 31,
        computed from one pass over the whole picture (``bnn_mi355x_scan_planes``; cnvW1A1).  Other networks and libraries
        without the entry point classify the cut records one by one."""
        return self._scan_planes(self._planes(self._as_pil(img)), details)

    @staticmethod
    def scan_boxes(size, window):
        """the level and the boxes of ONE window size ``window`` (8 or more, a multiple of 8) of a picture of ``size`` =
        (width, height): ((level_w, level_h), int32 array [n, 4]) -- the picture is resized to the level, ``width * 32 //
        window`` x ``height * 32 // window``, and cell (i, j) of the level's scan is the window (i w/8, j w/8, i w/8 + w, j w/8 + w)"""
        width, height = size
        if window < 8 or window % 8:
            raise ValueError("scan_boxes: the window size must be a multiple of 8 (8 or more)")
        lw, lh = width * 32 // window, height * 32 // window
        if lw < 32 or lh < 32:
            raise ValueError("scan_boxes: window size %d leaves a level below 32 x 32 pixels" % window)
        nx, ny, step = (lw - 32) // 4 + 1, (lh - 32) // 4 + 1, window // 8
        left, upper = np.meshgrid(np.arange(nx) * step, np.arange(ny) * step)
        b = np.stack([left, upper, left + window, upper + window], axis=-1).reshape(-1, 4).astype(np.int32)
        return (lw, lh), b

    def scan_scene(self, img, sizes=(64, 96), details=False):
        """a pyramid of dense scans: for each window size in ``sizes`` (size-major) the picture is resized like
        ``img.resize(level, Image.LANCZOS)`` and scanned (:meth:`scan`) -> (boxes int32 [n, 4] in the picture's coordinates,
        classes [n] or scores [n, len(classes)]).  On cnvW1A1 one upload and one stream (``bnn_mi355x_scan_scene``: RGB and L
        pictures); otherwise PIL resizes on the host."""
        pil = self._as_pil(img)
        ncls = len(self.classes)
        levels = [self.scan_boxes(pil.size, s) for s in sizes]
        boxes = np.concatenate([b for _, b in levels]) if levels else np.zeros((0, 4), np.int32)
        lib = self._scan_lib()
        if lib is None or pil.mode not in ("RGB", "L"):
            res = [self._scan_planes(self._planes(pil.resize(lv, Image.LANCZOS)), details).reshape((-1, ncls) if details else -1)
                   for lv, _ in levels]
            return boxes, (np.concatenate(res) if res else np.zeros((0, ncls) if details else 0, np.int32))
        a = np.ascontiguousarray(np.asarray(pil))
        sz = np.asarray(sizes, dtype=np.int32)
        out = np.zeros((len(boxes), 4), np.int32)
        usec, pre = ctypes.c_float(0), ctypes.c_float(0)
        ptr = lib.bnn_mi355x_scan_scene(a.ctypes.data, a.shape[1], a.shape[0], 1 if a.ndim == 2 else 3, 0, sz.ctypes.data, len(sz), ncls,
                                        out.ctypes.data, ctypes.byref(usec), ctypes.byref(pre), 1 if details else 0)
        if not ptr:
            raise RuntimeError(lib.bnn_mi355x_last_error().decode())
        res = self.bnn._collect(ptr, len(boxes) * (ncls if details else 1))
        self.usecPerImage = self.bnn.usecPerImage = usec.value
        self.usecPreprocess = pre.value
        return out, (res.reshape(-1, ncls) if details else res)

    def locate(self, img, class_index, sizes=(64, 96), min_score=None, dense=False):
        """cells 14 and 16: the windows of the notebook's tiling (:meth:`tile_boxes`) whose class is ``class_index`` -- or,
        with ``min_score``, those whose score for ``class_index`` exceeds it -> list of (left, upper, right, lower).
        ``dense``: the windows of :meth:`scan_scene` instead, a stride twice as fine in each direction (``size // 8``)."""
        if dense:
            boxes, res = self.scan_scene(img, sizes, details=min_score is not None)
            hit = (res == class_index) if min_score is None else (res[:, class_index] > min_score)
            return [tuple(int(v) for v in b) for b, h in zip(boxes, hit) if h]
        size = (img.shape[1], img.shape[0]) if isinstance(img, np.ndarray) else img.size
        bounds = self.tile_boxes(size, sizes)
        if not bounds:
            return []
        if min_score is None:
            hit = np.asarray(self.classify_windows(img, bounds)) == class_index
        else:
            scores = np.asarray(self.classify_windows_details(img, bounds)).reshape(len(bounds), len(self.classes))
            hit = scores[:, class_index] > min_score
        return [b for b, h in zip(bounds, hit) if h]

    # -- extension: the clip scan -- all frames and pyramid levels of a clip in one set of launches ----------
    @staticmethod
    def _clip_frames(frames):
        """(uint8 array [F, H, W] or [F, H, W, 3] for the device route, or None; the frames as a list)"""
        if isinstance(frames, np.ndarray):
            if frames.dtype != np.uint8 or frames.ndim not in (3, 4) or (frames.ndim == 4 and frames.shape[3] not in (3, 4)):
                raise ValueError("a clip given as one array must be uint8 [F, H, W] (L), [F, H, W, 3] (RGB) or [F, H, W, 4] (RGBA)")
            frames = list(frames)
        else:
            frames = list(frames)
        if not frames:
            raise ValueError("scan_clip: need one frame or more")
        arrays = [f if isinstance(f, np.ndarray) else (np.asarray(f) if f.mode in ("RGB", "RGBA", "L") else None) for f in frames]
        if any(a is None for a in arrays):
            if any(isinstance(f, np.ndarray) or f.size != frames[0].size or f.mode != frames[0].mode for f in frames):
                raise ValueError("scan_clip: the frames of a clip have one size and one mode")
            return None, frames
        if any(a.dtype != np.uint8 or a.shape != arrays[0].shape for a in arrays) or not (
                arrays[0].ndim == 2 or (arrays[0].ndim == 3 and arrays[0].shape[2] in (3, 4))):
            raise ValueError("scan_clip: the frames of a clip are uint8 pictures of one size and one mode")
        if arrays[0].ndim == 3 and arrays[0].shape[2] == 4:  # RGBA: the host route of scan_scene, frame by frame
            return None, frames
        return np.ascontiguousarray(np.stack(arrays)), frames

    # -- extension: camera frames -- NV12, I420, YUYV and BGR clips, from host memory or from a CUDA tensor ----------
    @staticmethod
    def _is_cuda_tensor(frames):
        return type(frames).__module__.split(".")[0] == "torch" and hasattr(frames, "data_ptr") and frames.is_cuda

    def _camera_clip(self, frames, pixel_format, video_range, what, always=False):
        """None for what the clip methods have always taken (``pixel_format="rgb"`` and no CUDA tensor; not with
        ``always``), else the clip as ``bnn_mi355x_frames`` states it: a dict with the uint8 array or CUDA tensor ``clip``
        (contiguous), ``format``, ``range``, ``width``, ``height`` and ``device``"""
        fmt = str(pixel_format).lower()
        if fmt not in abi.PIXEL_FORMATS:
            raise ValueError("%s: pixel_format must be one of %s" % (what, ", ".join(sorted(abi.PIXEL_FORMATS))))
        device = self._is_cuda_tensor(frames)
        if fmt == "rgb" and not device and not always:
            return None
        if device:
            import torch
            if frames.dtype != torch.uint8:
                raise ValueError("%s: a clip given as a tensor must be torch.uint8" % what)
            clip = frames.contiguous()
        else:
            clip = np.ascontiguousarray(frames)
            if clip.dtype != np.uint8:
                raise ValueError("%s: a %s clip must be one uint8 array" % (what, fmt))
        shape = tuple(clip.shape)
        if fmt in ("nv12", "i420"):
            ok, height = len(shape) == 3 and shape[1] % 3 == 0, shape[1] // 3 * 2 if len(shape) == 3 else 0
            want = "[F, h * 3 / 2, w]"
        elif fmt == "yuyv":
            ok, height, want = len(shape) == 4 and shape[3] == 2, shape[1] if len(shape) > 1 else 0, "[F, h, w, 2]"
        elif fmt == "l" or (fmt == "rgb" and len(shape) == 3):
            ok, height, want, fmt = len(shape) == 3, shape[1] if len(shape) > 1 else 0, "[F, h, w]", "l"
        else:
            ok, height, want = len(shape) == 4 and shape[3] == 3, shape[1] if len(shape) > 1 else 0, "[F, h, w, 3]"
        if not ok or shape[0] < 1:
            raise ValueError("%s: a %s clip must be uint8 %s with one frame or more" % (what, fmt, want))
        return dict(clip=clip, format=abi.PIXEL_FORMATS[fmt], range=1 if video_range else 0, width=shape[2], height=height, device=device)

    @staticmethod
    def _camera_piece(cam, first, step):
        """frames [first, first + step) of a camera clip -> (``bnn_mi355x_frames``, pointer, stream handle or None, the piece)"""
        part = cam["clip"][first:first + step]
        fr = abi.Frames(cam["format"], cam["range"], cam["width"], cam["height"], len(part), 0, 0)
        if cam["device"]:
            import torch
            return fr, part.data_ptr(), torch.cuda.current_stream(part.device).cuda_stream, part
        return fr, part.ctypes.data, None, part

    def unpack_frames(self, frames, pixel_format="nv12", video_range=False):
        """the packed RGB frames, uint8 ``[F, h, w, 3]``, of a camera clip: ``[F, h * 3 / 2, w]`` for ``nv12`` and ``i420``
        (a Y plane, then interleaved or planar chroma), ``[F, h, w, 2]`` for ``yuyv``, ``[F, h, w, 3]`` for ``bgr``.  Chroma is
        replicated; the colour is Pillow's ``convert("RGB")`` from YCbCr byte for byte, or with ``video_range`` BT.601 video
        range.  On the device where the library has ``bnn_mi355x_unpack_frames`` (CNV), else with the host model: the same
        bytes."""
        lib = self.bnn.interface
        if not hasattr(lib, "bnn_mi355x_unpack_frames_host"):
            raise RuntimeError("unpack_frames: the library has no bnn_mi355x_unpack_frames_host")
        if self._is_cuda_tensor(frames):
            frames = frames.cpu().numpy()
        cam = self._camera_clip(frames, pixel_format, video_range, "unpack_frames", always=True)
        fr, ptr, _, part = self._camera_piece(cam, 0, len(cam["clip"]))
        out = np.empty((len(part), cam["height"], cam["width"], 3), np.uint8)
        if lib.bnn_mi355x_network().decode().startswith("cnv"):
            rc = lib.bnn_mi355x_unpack_frames(ctypes.byref(fr), ptr, out.ctypes.data, None)
        else:
            rc = lib.bnn_mi355x_unpack_frames_host(ctypes.byref(fr), ptr, out.ctypes.data)
        if rc != 0:
            raise ValueError(lib.bnn_mi355x_last_error().decode())
        return out

    def _camera_lib(self):
        lib = self._scan_lib()
        return lib if lib is not None and hasattr(lib, "bnn_mi355x_detect_clip_frames") else None

    def _scan_camera_clip(self, cam, sizes, details, max_frames):
        """:meth:`scan_clip` of a camera clip through ``bnn_mi355x_scan_clip_frames`` / ``_device``"""
        lib, ncls = self._camera_lib(), len(self.classes)
        width, height, n_frames = cam["width"], cam["height"], len(cam["clip"])
        boxes = np.concatenate([self.scan_boxes((width, height), s)[1] for s in sizes]) if len(sizes) else np.zeros((0, 4), np.int32)
        sz = np.asarray(sizes, dtype=np.int32)
        step = lib.bnn_mi355x_scan_clip_capacity(width, height, sz.ctypes.data, len(sz))
        if step < 1:
            raise RuntimeError(lib.bnn_mi355x_last_error().decode())
        step = min(step, max_frames) if max_frames is not None else step
        out = np.zeros((len(boxes), 4), np.int32)
        parts, pre_us, pass_us = [], 0.0, 0.0
        for first in range(0, n_frames, step):
            fr, ptr, stream, part = self._camera_piece(cam, first, step)
            usec, pre = ctypes.c_float(0), ctypes.c_float(0)
            args = [ctypes.byref(fr), ptr, sz.ctypes.data, len(sz), ncls, out.ctypes.data, ctypes.byref(usec), ctypes.byref(pre), 1 if details else 0]
            res = lib.bnn_mi355x_scan_clip_device(*(args + [stream])) if cam["device"] else lib.bnn_mi355x_scan_clip_frames(*args)
            if not res:
                raise RuntimeError(lib.bnn_mi355x_last_error().decode())
            n = len(part) * len(boxes)
            parts.append(self.bnn._collect(res, n * (ncls if details else 1)).reshape((len(part), len(boxes), ncls) if details else (len(part), len(boxes))))
            pre_us += pre.value * n
            pass_us += usec.value * n
        total = n_frames * len(boxes)
        self.usecPerImage = self.bnn.usecPerImage = pass_us / total if total else 0.0
        self.usecPreprocess = pre_us / total if total else 0.0
        return out, np.concatenate(parts)

    def scan_clip(self, frames, sizes=(64, 96), details=False, max_frames=None, pixel_format="rgb", video_range=False):
        """:meth:`scan_scene` of every frame of a clip -- a sequence of PIL images or uint8 arrays of one size and mode, or
        one array ``[F, H, W(, 3)]`` -> (boxes int32 [n, 4], the same for every frame; classes [F, n] or scores
        [F, n, len(classes)]).  On cnvW1A1 the clip goes up once and every (frame, level) map runs through ONE launch per
        stage (``bnn_mi355x_scan_clip``: RGB and L frames); clips longer than one call accepts, or than ``max_frames``, go
        in several calls and are joined.  Other networks, libraries without the entry point and RGBA frames loop over
        :meth:`scan_scene`: the same answers by construction.

        ``pixel_format`` ``"nv12"``, ``"i420"``, ``"yuyv"`` or ``"bgr"`` takes camera frames as one array (the shapes of
        :meth:`unpack_frames`; ``video_range``: BT.601 video range instead of JFIF full range): they go up as they are and
        become RGB on the device (``bnn_mi355x_scan_clip_frames``).  A CUDA ``torch.uint8`` tensor of any format, ``"rgb"``
        and ``"l"`` included, is read where it lies, on the current stream (``bnn_mi355x_scan_clip_device``).  Libraries
        without those entry points convert with :meth:`unpack_frames` and go on as above."""
        cam = self._camera_clip(frames, pixel_format, video_range, "scan_clip")
        if cam is not None:
            if max_frames is not None and max_frames < 1:
                raise ValueError("scan_clip: max_frames must be 1 or more")
            if self._camera_lib() is None:
                return self.scan_clip(self.unpack_frames(frames, pixel_format, video_range), sizes, details, max_frames)
            return self._scan_camera_clip(cam, sizes, details, max_frames)
        clip, frames = self._clip_frames(frames)
        ncls = len(self.classes)
        if max_frames is not None and max_frames < 1:
            raise ValueError("scan_clip: max_frames must be 1 or more")
        lib = self._scan_lib()
        if lib is None or clip is None or not hasattr(lib, "bnn_mi355x_scan_clip"):
            res = [self.scan_scene(f, sizes, details) for f in frames]
            return res[0][0], np.stack([r for _, r in res])
        n_frames, height, width = clip.shape[:3]
        boxes = np.concatenate([self.scan_boxes((width, height), s)[1] for s in sizes]) if len(sizes) else np.zeros((0, 4), np.int32)
        sz = np.asarray(sizes, dtype=np.int32)
        step = lib.bnn_mi355x_scan_clip_capacity(width, height, sz.ctypes.data, len(sz))
        if step < 1:
            raise RuntimeError(lib.bnn_mi355x_last_error().decode())
        step = min(step, max_frames) if max_frames is not None else step
        out = np.zeros((len(boxes), 4), np.int32)
        parts, pre_us, pass_us = [], 0.0, 0.0
        for first in range(0, n_frames, step):
            part = clip[first:first + step]
            usec, pre = ctypes.c_float(0), ctypes.c_float(0)
            ptr = lib.bnn_mi355x_scan_clip(part.ctypes.data, len(part), 0, width, height, 1 if clip.ndim == 3 else 3, 0, sz.ctypes.data, len(sz), ncls,
                                           out.ctypes.data, ctypes.byref(usec), ctypes.byref(pre), 1 if details else 0)
            if not ptr:
                raise RuntimeError(lib.bnn_mi355x_last_error().decode())
            n = len(part) * len(boxes)
            parts.append(self.bnn._collect(ptr, n * (ncls if details else 1)).reshape((len(part), len(boxes), ncls) if details else (len(part), len(boxes))))
            pre_us += pre.value * n
            pass_us += usec.value * n
        total = n_frames * len(boxes)
        self.usecPerImage = self.bnn.usecPerImage = pass_us / total if total else 0.0
        self.usecPreprocess = pre_us / total if total else 0.0
        return out, np.concatenate(parts)

    def locate_clip(self, frames, class_index, sizes=(64, 96), min_score=None):
        """:meth:`locate` with ``dense=True`` for every frame of a clip (:meth:`scan_clip`) -> a list, per frame, of the
        windows (left, upper, right, lower) whose class is ``class_index`` -- or, with ``min_score``, whose score for it
        exceeds ``min_score``"""
        boxes, res = self.scan_clip(frames, sizes, details=min_score is not None)
        hits = (res == class_index) if min_score is None else (res[:, :, class_index] > min_score)
        return [[tuple(int(v) for v in b) for b, h in zip(boxes, hit) if h] for hit in hits]

    # -- extension: detections -- threshold, order and non-maximum suppression on the windows of a scan ----------
    def _detect_opts(self, classes, min_score, by_score, iou, max_det, max_candidates):
        """``bnn_mi355x_detect_opts`` of the Python arguments: ``classes`` None (all of ``self.classes``), an int or an
        iterable; ``iou`` a float, taken as ``round(iou * 65536) / 65536``, or an exact ``(num, den)`` pair"""
        if classes is None:
            wanted = range(len(self.classes))
        else:
            wanted = [classes] if isinstance(classes, (int, np.integer)) else list(classes)
        mask = 0
        for c in wanted:
            if not 0 <= int(c) < 64:
                raise ValueError("detect: class %r is outside 0..63" % (c,))
            mask |= 1 << int(c)
        num, den = (int(iou[0]), int(iou[1])) if isinstance(iou, (tuple, list)) else (int(round(float(iou) * 65536)), 65536)
        return abi.DetectOpts(mask, 1 if by_score else 0, -32769 if min_score is None else int(min_score), num, den, int(max_candidates),
                              int(max_det))

    @staticmethod
    def _detections(dets, counts):
        """per frame a list of ((left, upper, right, lower), class, score)"""
        return [[(tuple(int(v) for v in d[:4]), int(d[4]), int(d[5])) for d in frame[:k]] for frame, k in zip(dets, counts)]

    def suppress(self, boxes, scores, classes=None, min_score=None, by_score=False, iou=0.5, max_det=64, max_candidates=4096):
        """the detections among windows the caller has classified: ``boxes`` [n, 4] of ONE frame and ``scores`` [n, ncls]
        (or [F, n, ncls] for F frames that share the boxes), e.g. :meth:`tile_boxes` and :meth:`classify_windows_details`
        -> a list of ``((left, upper, right, lower), class, score)``, best first (for [F, n, ncls] one list per frame).  A
        window is a candidate when its class -- its argmax, or with ``by_score`` the ONE class of ``classes`` whatever its
        argmax -- is among ``classes`` and its score for that class exceeds ``min_score``; candidates are walked by score
        and kept unless an already kept one of the same class overlaps them with an IoU above ``iou``.  On the device where
        the library has ``bnn_mi355x_detect_windows``, else on the host: the same answers by construction.  After a call
        ``self.n_candidates`` holds, per frame, how many windows passed ``min_score`` (above ``max_candidates``: a cut)."""
        lib = self.bnn.interface
        b = self._boxes(boxes)
        s = np.ascontiguousarray(np.asarray(scores, dtype=np.int32))
        single = s.ndim == 2
        s = s[None] if single else s
        if s.ndim != 3 or s.shape[1] != len(b):
            raise ValueError("suppress: scores must be [n, ncls] or [F, n, ncls] for the n boxes given")
        if not hasattr(lib, "bnn_mi355x_detect_windows_host"):
            raise RuntimeError("suppress: the library has no bnn_mi355x_detect_windows_host")
        frames, n, ncls = s.shape
        o = self._detect_opts(classes if classes is not None else range(ncls), min_score, by_score, iou, max_det, max_candidates)
        dets = np.zeros((frames, max(o.max_det, 1), 8), np.int32)
        counts, ncand = np.zeros(frames, np.int32), np.zeros(frames, np.int32)
        args = [b.ctypes.data, n, s.ctypes.data, frames, ncls, ctypes.byref(o), dets.ctypes.data, counts.ctypes.data, ncand.ctypes.data]
        on_device = lib.bnn_mi355x_network().decode().startswith("cnv")
        rc = lib.bnn_mi355x_detect_windows(*(args + [None])) if on_device else lib.bnn_mi355x_detect_windows_host(*args)
        if rc != 0:
            raise ValueError(lib.bnn_mi355x_last_error().decode())
        self.n_candidates = ncand.tolist()
        found = self._detections(dets, counts)
        return found[0] if single else found

    def detect_clip(self, frames, classes=None, sizes=(64, 96), min_score=None, by_score=False, iou=0.5, max_det=64, max_candidates=4096,
                    max_frames=None, pixel_format="rgb", video_range=False):
        """where the objects are in every frame of a clip: :meth:`scan_clip` followed by :meth:`suppress` -> per frame a
        list of ``((left, upper, right, lower), class, score)``, best first.  On cnvW1A1 one call per piece of the clip
        (``bnn_mi355x_detect_clip``: RGB and L frames): the scan's launches, then the detection kernels on the scores where
        the scan left them, and only the lists come back; long clips are cut by the call's capacity and ``max_frames`` as
        in :meth:`scan_clip`.  Other networks, libraries without the entry point and RGBA frames take
        ``scan_clip(details=True)`` and :meth:`suppress`: the same answers by construction.

        ``pixel_format``, ``video_range`` and CUDA tensors: as :meth:`scan_clip` (``bnn_mi355x_detect_clip_frames``,
        ``bnn_mi355x_detect_clip_device``)."""
        if max_frames is not None and max_frames < 1:
            raise ValueError("detect_clip: max_frames must be 1 or more")
        ncls = len(self.classes)
        o = self._detect_opts(classes, min_score, by_score, iou, max_det, max_candidates)
        cam = self._camera_clip(frames, pixel_format, video_range, "detect_clip")
        if cam is not None and self._camera_lib() is None:
            frames, cam = self.unpack_frames(frames, pixel_format, video_range), None
        if cam is not None:
            return self._detect_camera_clip(cam, sizes, o, max_frames)
        lib = self._scan_lib()
        clip, listed = self._clip_frames(frames)
        if lib is None or clip is None or not hasattr(lib, "bnn_mi355x_detect_clip"):
            boxes, scores = self.scan_clip(listed, sizes, details=True, max_frames=max_frames)
            wanted = [k for k in range(64) if (o.class_mask >> k) & 1]
            return self.suppress(boxes, scores, wanted, o.min_score, by_score, (o.iou_num, o.iou_den), max_det, max_candidates)
        n_frames, height, width = clip.shape[:3]
        sz = np.asarray(sizes, dtype=np.int32)
        step = lib.bnn_mi355x_scan_clip_capacity(width, height, sz.ctypes.data, len(sz))
        if step < 1:
            raise RuntimeError(lib.bnn_mi355x_last_error().decode())
        step = min(step, max_frames) if max_frames is not None else step
        found, ncand, pre_us, pass_us, det_us, windows = [], [], 0.0, 0.0, 0.0, 0
        n = sum(len(self.scan_boxes((width, height), s)[1]) for s in sizes)
        for first in range(0, n_frames, step):
            part = clip[first:first + step]
            dets = np.zeros((len(part), max(o.max_det, 1), 8), np.int32)
            counts, nc = np.zeros(len(part), np.int32), np.zeros(len(part), np.int32)
            usec, pre, det = ctypes.c_float(0), ctypes.c_float(0), ctypes.c_float(0)
            rc = lib.bnn_mi355x_detect_clip(part.ctypes.data, len(part), 0, width, height, 1 if clip.ndim == 3 else 3, 0, sz.ctypes.data, len(sz),
                                            ncls, ctypes.byref(o), dets.ctypes.data, counts.ctypes.data, nc.ctypes.data, ctypes.byref(usec),
                                            ctypes.byref(pre), ctypes.byref(det))
            if rc != 0:
                raise RuntimeError(lib.bnn_mi355x_last_error().decode())
            found += self._detections(dets, counts)
            ncand += nc.tolist()
            pre_us += pre.value * n * len(part)
            pass_us += usec.value * n * len(part)
            det_us += det.value * len(part)
            windows += n * len(part)
        self.usecPerImage = self.bnn.usecPerImage = pass_us / windows if windows else 0.0
        self.usecPreprocess = pre_us / windows if windows else 0.0
        self.usecDetect = det_us / n_frames
        self.n_candidates = ncand
        return found

    def _detect_camera_clip(self, cam, sizes, o, max_frames):
        """:meth:`detect_clip` of a camera clip through ``bnn_mi355x_detect_clip_frames`` / ``_device``"""
        lib, ncls = self._camera_lib(), len(self.classes)
        width, height, n_frames = cam["width"], cam["height"], len(cam["clip"])
        sz = np.asarray(sizes, dtype=np.int32)
        step = lib.bnn_mi355x_scan_clip_capacity(width, height, sz.ctypes.data, len(sz))
        if step < 1:
            raise RuntimeError(lib.bnn_mi355x_last_error().decode())
        step = min(step, max_frames) if max_frames is not None else step
        found, ncand, pre_us, pass_us, det_us, windows = [], [], 0.0, 0.0, 0.0, 0
        n = sum(len(self.scan_boxes((width, height), s)[1]) for s in sizes)
        for first in range(0, n_frames, step):
            fr, ptr, stream, part = self._camera_piece(cam, first, step)
            dets = np.zeros((len(part), max(o.max_det, 1), 8), np.int32)
            counts, nc = np.zeros(len(part), np.int32), np.zeros(len(part), np.int32)
            usec, pre, det = ctypes.c_float(0), ctypes.c_float(0), ctypes.c_float(0)
            args = [ctypes.byref(fr), ptr, sz.ctypes.data, len(sz), ncls, ctypes.byref(o), dets.ctypes.data, counts.ctypes.data, nc.ctypes.data,
                    ctypes.byref(usec), ctypes.byref(pre), ctypes.byref(det)]
            rc = lib.bnn_mi355x_detect_clip_device(*(args + [stream])) if cam["device"] else lib.bnn_mi355x_detect_clip_frames(*args)
            if rc != 0:
                raise RuntimeError(lib.bnn_mi355x_last_error().decode())
            found += self._detections(dets, counts)
            ncand += nc.tolist()
            pre_us += pre.value * n * len(part)
            pass_us += usec.value * n * len(part)
            det_us += det.value * len(part)
            windows += n * len(part)
        self.usecPerImage = self.bnn.usecPerImage = pass_us / windows if windows else 0.0
        self.usecPreprocess = pre_us / windows if windows else 0.0
        self.usecDetect = det_us / n_frames
        self.n_candidates = ncand
        return found

    def detect(self, img, classes=None, sizes=(64, 96), **kwargs):
        """:meth:`detect_clip` on one picture -> a list of ``((left, upper, right, lower), class, score)``; with
        ``pixel_format`` one camera frame (``[h * 3 / 2, w]``, ``[h, w, 2]`` or ``[h, w, 3]``), as an array or a CUDA tensor"""
        one = img[None] if self._is_cuda_tensor(img) or str(kwargs.get("pixel_format", "rgb")).lower() != "rgb" else [img]
        return self.detect_clip(one, classes, sizes, **kwargs)[0]

    # extension
    def classify_array(self, images, detail=False):
        result = self.bnn.inference_array(images, detail)
        self.usecPerImage = self.bnn.usecPerImage
        return result

    def class_name(self, index):
        return self.bnn.classes[index]


class LfcClassifier:
    """LFC networks on MNIST formatted (28x28) images."""

    def __init__(self, network, params, runtime=RUNTIME_HW):
        if params in available_params(network):
            self.net = network
            self.params = params
            self.runtime = runtime
            self.usecPerImage = 0.0
            self.bnn = PynqBNN(runtime, network)
            self.bnn.load_parameters(os.path.join(params, network))
            self.classes = self.bnn.classes
        else:
            print("ERROR: parameters are not availlable for {0}".format(network))

    def classify_mnist(self, mnist_format_file):
        result = self.bnn.inference(mnist_format_file)
        self.usecPerImage = self.bnn.usecPerImage
        return result

    def classify_mnists(self, mnist_format_file):
        result = self.bnn.inference_multiple(mnist_format_file)
        self.usecPerImage = self.bnn.usecPerImage
        return result

    def classify_mnists_with_faults(self, mnist_format_file, num_faults, flip_word, target_type, target_layers=[]):
        result = self.bnn.inference_multiple_with_faults(mnist_format_file, num_faults, flip_word, target_type,
                                                         target_layers)
        self.usecPerImage = self.bnn.usecPerImage
        return result

    # extension
    def classify_mnists_with_faults_runs(self, mnist_format_file, num_runs, num_faults, flip_word, target_type,
                                         target_layers=[], seed=0):
        result = self.bnn.inference_multiple_with_faults_runs(mnist_format_file, num_runs, num_faults, flip_word,
                                                              target_type, target_layers, seed)
        self.usecPerImage = self.bnn.usecPerImage
        return result

    def classify_mnists_fault_sweep(self, mnist_format_file, records, max_diffs=None):
        result = self.bnn.fault_sweep(mnist_format_file, records, max_diffs)
        self.usecPerImage = self.bnn.usecPerImage
        return result

    def classify_mnists_act_fault_sweep(self, mnist_format_file, records, max_diffs=None):
        result = self.bnn.act_fault_sweep(mnist_format_file, records, max_diffs)
        self.usecPerImage = self.bnn.usecPerImage
        return result

    def classify_mnists_act_noise(self, mnist_format_file, num_runs, rates, seed=0):
        result = self.bnn.inference_multiple_act_noise(mnist_format_file, num_runs, rates, seed)
        self.usecPerImage = self.bnn.usecPerImage
        return result

    def classify_mnists_mem_noise(self, mnist_format_file, num_runs, rates_w, rates_t, seed=0, scheme=None, burst=1):
        result = self.bnn.inference_multiple_mem_noise(mnist_format_file, num_runs, rates_w, rates_t, seed, scheme, burst)
        self.usecPerImage = self.bnn.usecPerImage
        return result

    def classify_mnists_exposure(self, mnist_format_file, *args, **kwargs):
        result = self.bnn.inference_multiple_exposure(mnist_format_file, *args, **kwargs)
        self.usecPerImage = self.bnn.usecPerImage
        return result

    def classify_mnists_input_fault_sweep(self, mnist_format_file, records, max_diffs=None):
        result = self.bnn.input_fault_sweep(mnist_format_file, records, max_diffs)
        self.usecPerImage = self.bnn.usecPerImage
        return result

    def classify_mnists_input_noise(self, mnist_format_file, num_runs, rate, seed=0):
        result = self.bnn.inference_multiple_input_noise(mnist_format_file, num_runs, rate, seed)
        self.usecPerImage = self.bnn.usecPerImage
        return result

    def classify_array(self, images):
        result = self.bnn.inference_array(images)
        self.usecPerImage = self.bnn.usecPerImage
        return result

    # -- extension: from a picture to MNIST-format records and classes (LFC-BNN_MNIST_Webcam.ipynb and
    #    LFC-BNN_Chars_Webcam.ipynb, cells 9-13) ------------------------------------------------------------
    GLYPH_PRESETS = {"mnist": (3, 4.0, None), "chars": (5, 2.0, 180)}  # contrast, brightness, threshold of the two notebooks

    @classmethod
    def _glyph_opts(cls, preset="mnist", contrast=None, brightness=None, threshold=None, filter=3, square_blank=False):
        """the notebooks' knobs -> ``bnn_mi355x_glyph_opts``.  ``preset``: "mnist" (contrast 3, brightness 4.0, no
        threshold) or "chars" (5, 2.0, 180); each knob given by name overrides it.  ``filter``: 3 (BICUBIC, what
        ``Image.resize`` takes by default) or 0 (NEAREST, the default of the notebooks' 2018 Pillow).  ``square_blank``:
        reproduce the notebooks' blank record for a square ink box (they forget the paste)."""
        if preset not in cls.GLYPH_PRESETS:
            raise ValueError("preset must be one of %s" % sorted(cls.GLYPH_PRESETS))
        c, b, t = cls.GLYPH_PRESETS[preset]
        c = c if contrast is None else contrast
        b = b if brightness is None else brightness
        t = t if threshold is None else threshold
        return abi.GlyphOpts(float(c), float(b), -1 if t is None else int(t), int(filter), 1 if square_blank else 0)

    @staticmethod
    def _picture(img):
        """(uint8 array [H, W] / [H, W, 3] / [H, W, 4], bands); other PIL modes are made "L" as the notebooks do"""
        if isinstance(img, np.ndarray):
            if img.dtype != np.uint8 or not (img.ndim == 2 or (img.ndim == 3 and img.shape[2] in (3, 4))):
                raise ValueError("pictures given as arrays must be uint8 [H, W, 3] (RGB), [H, W, 4] (RGBA) or [H, W] (L)")
            a = np.ascontiguousarray(img)
        else:
            a = np.ascontiguousarray(np.asarray(img if img.mode in ("RGB", "RGBA", "L") else img.convert("L")))
        return a, (1 if a.ndim == 2 else a.shape[2])

    @staticmethod
    def _glyph_boxes(boxes):
        if boxes is None:
            return None, 0
        b = np.ascontiguousarray(np.asarray(boxes, dtype=np.int32).reshape(-1, 4))
        if len(b) == 0:
            raise ValueError("no boxes (boxes=None takes the whole picture)")
        return b, len(b)

    def _on_device(self):
        # a library with only the reference's six symbols (the reference's own .so) has no such entry points
        return hasattr(self.bnn.interface, "bnn_mi355x_classify_glyphs")

    @staticmethod
    def _enhance_host(a, o):
        """cells 9 of the notebooks in PIL: the enhanced "L" picture"""
        from PIL import ImageEnhance
        img = Image.fromarray(a).convert("L")
        img = ImageEnhance.Contrast(img).enhance(o.contrast)
        img = ImageEnhance.Brightness(img).enhance(o.brightness)
        if o.threshold >= 0:
            img = img.point(lambda p: 255 if p > o.threshold else 0)
        return img

    def _glyphs_host(self, a, b, o):
        """cells 9-13 in PIL, per box: (records, ink boxes, status)"""
        from PIL import ImageOps
        plane = self._enhance_host(a, o)
        boxes = [(0, 0) + plane.size] if b is None else [tuple(int(v) for v in box) for box in b]
        recs = np.zeros((len(boxes), 784), np.uint8)
        ink = np.zeros((len(boxes), 4), np.int32)
        status = np.zeros(len(boxes), np.int32)
        for i, box in enumerate(boxes):
            crop = plane.crop(box)
            found = ImageOps.invert(crop).getbbox()
            if found is None:
                found, status[i] = (0, 0) + crop.size, 1
            glyph = crop.crop(found)
            ink[i] = (box[0] + found[0], box[1] + found[1], box[0] + found[2], box[1] + found[3])
            width, height = glyph.size
            ratio = min((28. / height), (28. / width))
            size = (28, 28) if height == width else (int(width * ratio), 28) if height > width else (28, int(height * ratio))
            if 0 in size:
                status[i] = 2
                continue
            background = Image.new("L", (28, 28), 255)
            if not (o.square_blank and height == width):
                glyph = glyph.resize(size, o.filter)
                background.paste(glyph, (int((28 - glyph.size[0]) / 2), int((28 - glyph.size[1]) / 2)))
            recs[i] = np.where(np.asarray(background).reshape(-1) == 0, 255, 1)
        return recs, ink, status

    def enhance(self, img, **opts):
        """the picture after greyscale, contrast, brightness and threshold (see :meth:`_glyph_opts` for the knobs) as a
        PIL "L" image: what the notebooks display before they crop.  Made on the GPU (``bnn_mi355x_enhance_picture``)."""
        o = self._glyph_opts(**opts)
        a, bands = self._picture(img)
        if not self._on_device():
            return self._enhance_host(a, o)
        lib = self.bnn.interface
        out = np.empty(a.shape[:2], np.uint8)
        if lib.bnn_mi355x_enhance_picture(a.ctypes.data, a.shape[1], a.shape[0], bands, 0, ctypes.byref(o), out.ctypes.data, None) != 0:
            raise RuntimeError(lib.bnn_mi355x_last_error().decode())
        return Image.fromarray(out)

    def glyphs_to_mnist(self, img, boxes=None, details=False, **opts):
        """MNIST-format records (uint8 array [n, 784]) of the glyphs in the ``boxes`` (left, upper, right, lower) of ONE
        picture -- ``boxes=None``: the whole picture holds one glyph.  Per box what the notebooks do to a camera frame:
        enhance, bounding box of the ink, resize into 28 x 28 keeping the aspect ratio, paste centred on white, 255 / 1
        per pixel; on the GPU from one upload of the picture (``bnn_mi355x_glyphs_to_mnist``).  ``details=True``:
        (records, ink boxes [n, 4] in picture coordinates, status [n]: 0 fine, 1 no ink in the box, 2 ink more than 28
        times as long as wide, where Pillow raises -- that record is all zero).  The caller's image is left as it is."""
        o = self._glyph_opts(**opts)
        a, bands = self._picture(img)
        b, n = self._glyph_boxes(boxes)
        if not self._on_device():
            recs, ink, status = self._glyphs_host(a, b, o)
        else:
            lib = self.bnn.interface
            m = max(n, 1)
            recs, ink, status = np.zeros((m, 784), np.uint8), np.zeros((m, 4), np.int32), np.zeros(m, np.int32)
            if lib.bnn_mi355x_glyphs_to_mnist(a.ctypes.data, a.shape[1], a.shape[0], bands, 0, None if b is None else b.ctypes.data, n,
                                              ctypes.byref(o), recs.ctypes.data, ink.ctypes.data, status.ctypes.data) != 0:
                raise RuntimeError(lib.bnn_mi355x_last_error().decode())
        return (recs, ink, status) if details else recs

    def image_to_mnist(self, img, fp, **opts):
        """write the idx3 header for one image and the record of the one glyph in ``img`` (cell 13's file, what
        :meth:`classify_mnist` takes).  Raises ``ValueError`` where Pillow does: ink more than 28 times as long as wide."""
        recs, _, status = self.glyphs_to_mnist(img, None, details=True, **opts)
        if status[0] == 2:
            raise ValueError("height and width must be > 0")
        fp.write(bytes([0, 0, 8, 3, 0, 0, 0, 1, 0, 0, 0, 28, 0, 0, 0, 28]))
        fp.write(recs[0].tobytes())

    def classify_glyphs(self, img, boxes=None, **opts):
        """the classes of the glyphs in ``boxes`` (see :meth:`glyphs_to_mnist`): what :meth:`classify_mnists` returns for
        an idx file of their records, -1 for a glyph of status 2.  The picture goes to the GPU once and the records never
        leave it (``bnn_mi355x_classify_glyphs``).  ``self.glyph_status`` holds the status per glyph."""
        o = self._glyph_opts(**opts)
        a, bands = self._picture(img)
        b, n = self._glyph_boxes(boxes)
        if not self._on_device():
            recs, _, status = self._glyphs_host(a, b, o)
            with tempfile.NamedTemporaryFile() as tmp:
                tmp.write(bytes([0, 0, 8, 3]) + len(recs).to_bytes(4, "big") + bytes([0, 0, 0, 28, 0, 0, 0, 28]) + recs.tobytes())
                tmp.flush()
                result = self.classify_mnists(tmp.name)
            result[status == 2] = -1
            self.glyph_status = status
            return result
        lib = self.bnn.interface
        m = max(n, 1)
        status = np.zeros(m, np.int32)
        usec, pre = ctypes.c_float(0), ctypes.c_float(0)
        ptr = lib.bnn_mi355x_classify_glyphs(a.ctypes.data, a.shape[1], a.shape[0], bands, 0, None if b is None else b.ctypes.data, n,
                                             ctypes.byref(o), len(self.classes), ctypes.byref(usec), ctypes.byref(pre), status.ctypes.data)
        if not ptr:
            raise RuntimeError(lib.bnn_mi355x_last_error().decode())
        result = self.bnn._collect(ptr, m)
        self.usecPerImage = self.bnn.usecPerImage = usec.value
        self.usecPreprocess = pre.value
        self.glyph_status = status
        return result

    # -- extension: find the glyphs of a picture (connected components of its ink, on the GPU) and read them ----------
    FIND_ORDERS = {"raster": 0, "left": 1}

    def _find_entry(self, symbol):
        lib = self.bnn.interface
        if not hasattr(lib, symbol):  # no second implementation in Python
            raise RuntimeError("the runtime library has no %s: rebuild it with `make -C bnn-pynq_amd`" % symbol)
        return lib

    @classmethod
    def _find_opts(cls, reach, min_pixels, ink_level, order, max_glyphs):
        if order not in cls.FIND_ORDERS:
            raise ValueError("order must be one of %s" % sorted(cls.FIND_ORDERS))
        rx, ry = reach
        return abi.FindOpts(int(ink_level), int(rx), int(ry), int(min_pixels), cls.FIND_ORDERS[order]), int(max_glyphs)

    def find_glyphs(self, img, reach=(1, 1), min_pixels=1, ink_level=255, order="left", max_glyphs=4096, details=False, **opts):
        """the boxes (int32 array [n, 4]: left, upper, right, lower, as :meth:`classify_glyphs` takes them) of the glyphs of
        ONE picture: the connected components of its ink, labelled on the GPU on the enhanced plane
        (``bnn_mi355x_find_glyphs``; ``**opts``: the knobs of :meth:`_glyph_opts`).  A pixel is ink below ``ink_level``;
        two ink pixels are adjacent within ``reach`` = (x, y) pixels -- (1, 1) is 8-connectivity, a larger y joins the dot
        of an "i" to its stem; components of fewer than ``min_pixels`` pixels are dropped.  ``order``: "left" (by left
        edge: the reading order of one line) or "raster" (by first pixel).  At most ``max_glyphs`` are returned.
        ``details=True``: (boxes, pixel counts, total found, labels int32 [height, width]: the index of each pixel's glyph,
        -1 for background, dropped glyphs and glyphs beyond ``max_glyphs``)."""
        o = self._glyph_opts(**opts)
        f, cap = self._find_opts(reach, min_pixels, ink_level, order, max_glyphs)
        a, bands = self._picture(img)
        lib = self._find_entry("bnn_mi355x_find_glyphs")
        n = max(1, min(cap, ((a.shape[1] + 1) // 2) * ((a.shape[0] + 1) // 2)))  # never more glyphs than 2 x 2 cells
        boxes, counts = np.zeros((n, 4), np.int32), np.zeros(n, np.int32)
        labels = np.empty(a.shape[:2], np.int32) if details else None
        total = lib.bnn_mi355x_find_glyphs(a.ctypes.data, a.shape[1], a.shape[0], bands, 0, ctypes.byref(o), ctypes.byref(f), boxes.ctypes.data,
                                           counts.ctypes.data, None if labels is None else labels.ctypes.data, cap)
        if total < 0:
            raise RuntimeError(lib.bnn_mi355x_last_error().decode())
        self.glyphs_found = total
        k = min(total, cap)
        return (boxes[:k], counts[:k], total, labels) if details else boxes[:k]

    def read_glyphs(self, img, reach=(1, 1), min_pixels=1, ink_level=255, order="left", max_glyphs=4096, **opts):
        """(classes, boxes) of the glyphs of ONE picture, found as :meth:`find_glyphs` finds them and classified as
        :meth:`classify_glyphs` classifies those boxes, in one call (``bnn_mi355x_read_glyphs``): the picture goes to the
        GPU once, neither the plane nor the records come back.  ``self.glyph_status`` holds the status per glyph,
        ``self.glyphs_found`` how many there were (it may exceed ``max_glyphs``)."""
        o = self._glyph_opts(**opts)
        f, cap = self._find_opts(reach, min_pixels, ink_level, order, max_glyphs)
        a, bands = self._picture(img)
        lib = self._find_entry("bnn_mi355x_read_glyphs")
        n = max(1, min(cap, ((a.shape[1] + 1) // 2) * ((a.shape[0] + 1) // 2)))
        boxes, status = np.zeros((n, 4), np.int32), np.zeros(n, np.int32)
        usec, pre, found = ctypes.c_float(0), ctypes.c_float(0), ctypes.c_int(0)
        ptr = lib.bnn_mi355x_read_glyphs(a.ctypes.data, a.shape[1], a.shape[0], bands, 0, ctypes.byref(o), ctypes.byref(f), len(self.classes), cap,
                                         ctypes.byref(found), boxes.ctypes.data, ctypes.byref(usec), ctypes.byref(pre), status.ctypes.data)
        if not ptr:
            raise RuntimeError(lib.bnn_mi355x_last_error().decode())
        k = min(found.value, cap)
        result = np.ctypeslib.as_array(ptr, shape=(max(k, 1),))[:k].astype(np.int32, copy=True)
        lib.free_results(ptr)
        self.usecPerImage = self.bnn.usecPerImage = usec.value
        self.usecPreprocess = pre.value
        self.glyph_status = status[:k]
        self.glyphs_found = found.value
        return result, boxes[:k]

    # -- extension: read a page -- lines of text, every glyph masked to its own ink (csrc/page.h) -----------------------
    def _page_call(self, symbol, img, mask, lines, word_gap, reach, min_pixels, ink_level, order, max_glyphs, opts):
        o = self._glyph_opts(**opts)
        f, cap = self._find_opts(reach, min_pixels, ink_level, order, max_glyphs)
        g = abi.PageOpts(1 if mask else 0, 1 if lines else 0, int(word_gap))
        a, bands = self._picture(img)
        lib = self._find_entry(symbol)
        n = max(1, min(cap, ((a.shape[1] + 1) // 2) * ((a.shape[0] + 1) // 2)))
        return lib, a, bands, o, f, g, cap, n

    def page_to_mnist(self, img, mask=True, lines=True, word_gap=0, reach=(1, 1), min_pixels=1, ink_level=255, order="left", max_glyphs=4096,
                      **opts):
        """the records form of :meth:`read_page` (``bnn_mi355x_page_to_mnist``): (records uint8 [n, 784] with zeros for a
        glyph of status 2, boxes [n, 4], status [n], lines [n], gaps [n]).  Sets ``self.glyphs_found``."""
        lib, a, bands, o, f, g, cap, n = self._page_call("bnn_mi355x_page_to_mnist", img, mask, lines, word_gap, reach, min_pixels, ink_level,
                                                         order, max_glyphs, opts)
        recs, boxes = np.zeros((n, 784), np.uint8), np.zeros((n, 4), np.int32)
        status, line, gap = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
        found = ctypes.c_int(0)
        if lib.bnn_mi355x_page_to_mnist(a.ctypes.data, a.shape[1], a.shape[0], bands, 0, ctypes.byref(o), ctypes.byref(f), ctypes.byref(g), cap,
                                        ctypes.byref(found), boxes.ctypes.data, recs.ctypes.data, status.ctypes.data, line.ctypes.data,
                                        gap.ctypes.data) != 0:
            raise RuntimeError(lib.bnn_mi355x_last_error().decode())
        k = min(found.value, cap)
        self.glyphs_found = found.value
        return recs[:k], boxes[:k], status[:k], line[:k], gap[:k]

    def read_page(self, img, mask=True, lines=True, word_gap=0, reach=(1, 1), min_pixels=1, ink_level=255, order="left", max_glyphs=4096,
                  **opts):
        """(classes, boxes, lines, gaps) of the glyphs of ONE picture that may hold several lines of glyphs whose boxes
        overlap (``bnn_mi355x_read_page``).  ``mask``: a glyph's record holds its own ink alone -- whatever else lies
        inside its box is white -- so a neighbour's stroke, a dot inside a "0" or a speck dropped by ``min_pixels`` does
        not move its scale and class; False is :meth:`read_glyphs`' crop of the box.  ``lines``: the glyphs come line by
        line, top to bottom, each line left to right (``lines[i]``: the line of glyph i; a glyph joins the line whose band
        it overlaps by half its own or the band's height); False keeps ``order``.  ``word_gap`` > 0: ``gaps[i]`` is 1
        where glyph i starts ``word_gap`` pixels or more to the right of everything before it in its line.  The other
        knobs are :meth:`find_glyphs`' and :meth:`_glyph_opts`'.  ``self.glyph_status`` holds the status per glyph,
        ``self.glyphs_found`` how many there were."""
        lib, a, bands, o, f, g, cap, n = self._page_call("bnn_mi355x_read_page", img, mask, lines, word_gap, reach, min_pixels, ink_level, order,
                                                         max_glyphs, opts)
        boxes, status, line, gap = np.zeros((n, 4), np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
        usec, pre, found = ctypes.c_float(0), ctypes.c_float(0), ctypes.c_int(0)
        ptr = lib.bnn_mi355x_read_page(a.ctypes.data, a.shape[1], a.shape[0], bands, 0, ctypes.byref(o), ctypes.byref(f), ctypes.byref(g),
                                       len(self.classes), cap, ctypes.byref(found), boxes.ctypes.data, line.ctypes.data, gap.ctypes.data,
                                       ctypes.byref(usec), ctypes.byref(pre), status.ctypes.data)
        if not ptr:
            raise RuntimeError(lib.bnn_mi355x_last_error().decode())
        k = min(found.value, cap)
        result = np.ctypeslib.as_array(ptr, shape=(max(k, 1),))[:k].astype(np.int32, copy=True)
        lib.free_results(ptr)
        self.usecPerImage = self.bnn.usecPerImage = usec.value
        self.usecPreprocess = pre.value
        self.glyph_status = status[:k]
        self.glyphs_found = found.value
        return result, boxes[:k], line[:k], gap[:k]

    def read_text(self, img, **kwargs):
        """what the picture says: the class names of :meth:`read_glyphs`' glyphs in order, "?" for a glyph of status 2.
        Given ``mask=``, ``lines=`` or ``word_gap=`` it reads through :meth:`read_page`: the lines joined with "\\n", a
        " " in front of a glyph whose gap is set."""
        if not any(k in kwargs for k in ("mask", "lines", "word_gap")):
            classes, _ = self.read_glyphs(img, **kwargs)
            return "".join(self.class_name(c) if c >= 0 else "?" for c in classes)
        classes, _, lines, gaps = self.read_page(img, **kwargs)
        text = []
        for i, c in enumerate(classes):
            if i and lines[i] != lines[i - 1]:
                text.append("\n")
            elif gaps[i]:
                text.append(" ")
            text.append(self.class_name(c) if c >= 0 else "?")
        return "".join(text)

    def classify_image(self, img, **opts):
        """the class of the one glyph in ``img`` (a PIL image or a uint8 array): the notebooks, from the camera frame to
        the class, in one call.  Raises ``ValueError`` where Pillow does (see :meth:`image_to_mnist`)."""
        result = self.classify_glyphs(img, None, **opts)
        if self.glyph_status[0] == 2:
            raise ValueError("height and width must be > 0")
        return int(result[0])

    def classify_path(self, path, **opts):
        return self.classify_image(Image.open(path), **opts)

    def class_name(self, index):
        return self.bnn.classes[index]
