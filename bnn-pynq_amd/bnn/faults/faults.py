"""Campaign drivers over ``classify_*_with_faults`` -- same classes, methods, arguments and result
files as the reference's ``bnn/faults/faults.py``, written for this package.

``FaultTest.run_test`` builds a fresh classifier for every run (``load_parameters`` again: the
faults of the previous run are gone), injects ``num_flips`` upsets of ``word_size`` adjacent bits
while the input set is classified, and reports the accuracy of each run.  ``NetworkTest`` sweeps
fault counts x {any, weight, threshold} x {bit, word}, writes the raw accuracies and the statistics
(min / max / average, "effective" runs = runs whose accuracy differs from the control) as JSON.

On the MI355X runtime a run of 10 000 CIFAR-10 images with 100 upsets takes about 5 ms plus the
3 ms parameter reload (tools/fault_campaign_rate.py).  ``batched=True`` runs all of a test's runs in ONE
call instead (``classify_*_with_faults_runs``: the runs side by side on the GPU, tools/fault_campaigns_rate.py);
with the same ``seed`` (run i seeded with seed + i) both paths return identical results.

``FaultTest.sensitivity`` / ``NetworkTest.sensitivity_map`` answer the question random campaigns can only
sample: which bits matter.  Every distinct single fault of the chosen layers is evaluated alone on the whole input
set (``PynqBNN.fault_sweep``: the fault-free pass once, each fault from its own layer on, (fault, image) pairs
dropped as soon as their activations equal the fault-free ones).

``FaultTest.activation_sensitivity`` / ``NetworkTest.activation_sensitivity_map`` ask the same of the datapath: every
single activation of a layer's output, moved to another level while one image passes (``PynqBNN.act_fault_sweep``).

``FaultTest.run_noise_test`` / ``NetworkTest.upset_rate_curve`` give the datapath's accuracy-versus-upset-rate curve:
every activation of the chosen layers' outputs upset with probability p, independently per run, image and site
(``PynqBNN.inference_multiple_act_noise``), with the spread over the runs and the rate the runs actually saw.

``FaultTest.run_memory_noise_test`` / ``NetworkTest.memory_upset_rate_curve`` give the same curve for the parameter
memories: every bit of the weight / threshold memories flipped with probability p per run, in place from the first image
on (``PynqBNN.inference_multiple_mem_noise``), per memory kind and layer set.  With ``scheme=`` / ``burst=`` the upsets
hit the PHYSICAL memories of one of the fork's hardened overlays -- three voted modules (TMR), bit-interleaved threshold
lines -- in bursts of adjacent bits; ``NetworkTest.hardening_curve`` compares the schemes at the same rates, the figure a
hardening study reports.  ``hardening_of`` maps an overlay's name to (base network, scheme).

``FaultTest.run_exposure_test`` / ``NetworkTest.scrubbing_curve`` let those upsets ACCUMULATE while the run goes on: the
images are cut into epochs, the rates are per epoch, and the memories are rewritten every ``scrub_every`` epochs
(``PynqBNN.inference_multiple_exposure``) -- the accuracy per epoch tells how often a hardened memory must be scrubbed.

``FaultTest.input_sensitivity`` / ``NetworkTest.input_sensitivity_map`` and ``FaultTest.run_input_noise_test`` /
``NetworkTest.input_upset_rate_curve`` are their twins for the image buffer every classification starts from: every
single bit of the input image flipped alone (``PynqBNN.input_fault_sweep``), and every bit flipped with probability p
(``PynqBNN.inference_multiple_input_noise``).

``FaultTest.propagation`` / ``NetworkTest.propagation_map`` ask where a fault is masked: any of the three single-fault
sweeps with ``PynqBNN.sweep_profile`` on, which adds per fault and layer the images and the activations that differ from
the fault-free ones; ``propagation_curves`` reduces the two arrays to a masking curve and a mean error size per layer.
"""
from collections import namedtuple

import numpy as np

from .. import bnn as _bnn
from .. import util


def propagation_curves(alive, flipped, n_images, first=0):
    """A sweep's propagation profile (PynqBNN.last_sweep_profile: alive[f, l] images, flipped[f, l] activations that
    differ from the fault-free ones after layer l) reduced over the faults, for the columns from `first` on (the first
    layer the sweep evaluates for these faults).  -> (share alive, mean error size), two float lists with an entry per
    column: the share of the faults x n_images (fault, image) pairs still alive after that layer -- the masking curve --
    and the mean of flipped / alive over the faults with alive > 0 there, the activations an image that is still wrong
    has wrong (0.0 where no fault is alive)."""
    alive = np.asarray(alive, np.int64)[:, first:]
    flipped = np.asarray(flipped, np.int64)[:, first:]
    pairs = alive.shape[0] * int(n_images)
    share = alive.sum(axis=0) / float(pairs) if pairs else np.zeros(alive.shape[1])
    live = alive > 0
    size = np.where(live, flipped / np.maximum(alive, 1), 0.0).sum(axis=0) / np.maximum(live.sum(axis=0), 1)
    return [float(x) for x in share], [float(x) for x in size]


# the memory organisations of the fork's hardened overlays (csrc/mem_org.h), by the scheme number the C ABI takes
HARDENING_SCHEMES = ("none", "TMR", "interleaved", "resilient-interleaved")
# the codes of the 16-bit threshold memories (csrc/ecc.h), by the code number the C ABI takes; the project's own model
ECC_CODES = ("", "SEC-DED")
# the codes of the weight memories of the layers >= 1 (csrc/wecc.h), by the weight_code number; the project's own model
WEIGHT_CODES = ("", "SEC-DED weights")
# the column interleave of those code words (csrc/mem_org.h, "column-interleaved code words"), by the weight_interleave number
WEIGHT_INTERLEAVES = ("", "column-interleaved")


# a memory organisation of the exposure campaigns: the numbers the C ABI takes, by HARDENING_SCHEMES, ECC_CODES, WEIGHT_CODES
# and WEIGHT_INTERLEAVES
Organisation = namedtuple("Organisation", "scheme code weight_code weight_interleave")


def organisation(entry):
    """an entry of hardening_curve's / scrubbing_curve's `schemes` -> Organisation: a plain scheme, or a (scheme, code), (scheme,
    code, weight_code) or (scheme, code, weight_code, weight_interleave) tuple; what an entry leaves out is 0"""
    parts = tuple(entry) if isinstance(entry, (tuple, list)) else (entry,)
    return Organisation(*(int(x) for x in parts + (0,) * (4 - len(parts))))


UpsetCounts = namedtuple("UpsetCounts", "weights_physical weights_logical thresholds_physical thresholds_logical corrected detected "
                                        "repaired unrepaired weight_corrected weight_detected weight_repaired weight_unrepaired")


def upset_counts(counts):
    """The counts of a hardened or exposure campaign, [run, (epoch,) layer] + the family's last axes, by name: an
    UpsetCounts of arrays [run, (epoch,) layer], None for the blocks the family does not count.  The columns:

        last axes   column    field
        (2, 2)...   0, 1      weights_physical (bits flipped; with a weight code data plus check bits), weights_logical (bits
                              that differ after voting, de-interleaving and decoding)
                    2, 3      thresholds_physical (with a code data plus check bits), thresholds_logical
        6 ...       4, 5      corrected, detected: threshold words the SEC-DED decoder corrected / found uncorrectable
        8 ...       6, 7      repaired, unrepaired: words the epoch's repair rewrote / of the repaired memories still unlike
                              the loaded ones after it
        12          8 ... 11  weight_corrected, weight_detected, weight_repaired, weight_unrepaired: the same four of the
                              weight code words

    (2, 2) is [weights, thresholds][physical, logical]: columns 0 ... 3 of the wider forms."""
    counts = np.asarray(counts)
    if counts.shape[-1] == 2:
        counts = counts.reshape(counts.shape[:-2] + (4,))
    return UpsetCounts(*(counts[..., i] if i < counts.shape[-1] else None for i in range(len(UpsetCounts._fields))))


def organisation_name(scheme, code=0, weight_code=0, weight_interleave=0):
    return HARDENING_SCHEMES[scheme] + (" + " + ECC_CODES[code] if code else "") + (" + " + WEIGHT_CODES[weight_code] if weight_code else "") + \
        (" " + WEIGHT_INTERLEAVES[weight_interleave] if weight_interleave else "")


def hardening_of(overlay):
    """an overlay's name -> (base network, scheme): "cnvW1A1-TMR" -> ("cnvW1A1", 1), "cnvW2A2" -> ("cnvW2A2", 0)"""
    base, _, suffix = overlay.partition("-")
    if suffix and suffix not in HARDENING_SCHEMES[1:]:
        raise ValueError("unknown hardened overlay: " + overlay)
    return base, HARDENING_SCHEMES.index(suffix) if suffix else 0


class FaultTest:
    class TargetType:
        @staticmethod
        def any():
            return -1

        @staticmethod
        def weights():
            return 0

        @staticmethod
        def thresholds():
            return 1

    def __init__(self, classifier_cls, network, dataset, input_file, labels, runtime=_bnn.RUNTIME_HW):
        self.classifier_cls = classifier_cls
        self.network = network
        self.dataset = dataset
        self.input_file = input_file  # a file path, or a list of PIL images for the non-CIFAR picture sets
        self.labels = labels
        self.runtime = runtime

    def _describe(self, i, num_runs, num_flips, word_size, target_type, target_layers):
        return "{}-{} run {} of {} (flipping {}{} {}(s) in {})".format(
            self.network, self.dataset, i + 1, num_runs, num_flips,
            " weight" if target_type == 0 else " threshold" if target_type == 1 else "",
            "word" if word_size > 1 else "bit",
            "any layer" if not target_layers else "layer(s) {}".format(target_layers))

    def run_test(self, num_runs, num_flips, word_size=1, target_type=-1, target_layers=(), batched=False, seed=0):
        """-> (results per run, usec per image per run, accuracy per run).
        batched: all runs in one call, side by side on the GPU (the usec figure is then the call's, per image of
        every run).  seed != 0: run i seeds the fault planner with seed + i (0: std::random_device), so that
        both forms give the same results."""
        target_layers = list(target_layers)
        if batched:
            return self._run_test_batched(num_runs, num_flips, word_size, target_type, target_layers, seed)
        results, times, accuracies = [], [], []
        for i in range(num_runs):
            classifier = self.classifier_cls(self.network, self.dataset, self.runtime)
            if seed:
                classifier.bnn.interface.bnn_mi355x_set_fault_seed(seed + i)
            print(self._describe(i, num_runs, num_flips, word_size, target_type, target_layers))
            if self.dataset == "cifar10":
                got = classifier.classify_cifars_with_faults(self.input_file, num_flips, word_size, target_type, target_layers)
            elif self.dataset == "mnist":
                got = classifier.classify_mnists_with_faults(self.input_file, num_flips, word_size, target_type, target_layers)
            else:
                got = classifier.classify_images_with_faults(self.input_file, num_flips, word_size, target_type, target_layers)
            results.append(got.tolist())
            times.append(classifier.usecPerImage)
            accuracies.append(util.calculate_accuracy(results[-1], self.labels))
            print("Accuracy:", accuracies[-1])
            print()
        if seed and num_runs:
            classifier.bnn.interface.bnn_mi355x_set_fault_seed(0)  # (the library outlives the classifier: back to the default)
        return (results, times, accuracies)

    def _run_test_batched(self, num_runs, num_flips, word_size, target_type, target_layers, seed):
        classifier = self.classifier_cls(self.network, self.dataset, self.runtime)
        print(self._describe(0, num_runs, num_flips, word_size, target_type, target_layers).replace(
            "run 1 of {}".format(num_runs), "{} run(s) in one call".format(num_runs)))
        if self.dataset == "cifar10":
            got = classifier.classify_cifars_with_faults_runs(self.input_file, num_runs, num_flips, word_size, target_type,
                                                              target_layers, seed)
        elif self.dataset == "mnist":
            got = classifier.classify_mnists_with_faults_runs(self.input_file, num_runs, num_flips, word_size, target_type,
                                                              target_layers, seed)
        else:
            got = classifier.classify_images_with_faults_runs(self.input_file, num_runs, num_flips, word_size, target_type,
                                                              target_layers, seed)
        results = [row.tolist() for row in got]
        times = [classifier.usecPerImage] * num_runs
        accuracies = [util.calculate_accuracy(r, self.labels) for r in results]
        print("Accuracies:", accuracies)
        print()
        return (results, times, accuracies)


    def _classify(self, classifier, method, *args, **kwargs):
        """classifier.classify_<set>_<method>(input, *args, **kwargs) for this test's input set"""
        kind = {"cifar10": "cifars", "mnist": "mnists"}.get(self.dataset, "images")
        return getattr(classifier, "classify_{}{}".format(kind, method))(self.input_file, *args, **kwargs)

    def sensitivity(self, layers, target_type=0, word_size=1):
        """Every distinct single fault of `layers` (target_type 0 weights / 1 thresholds, word_size adjacent bits),
        each alone on the whole input set.  -> (records int32 [k, 8], changed [k]: images whose class the fault
        changes, accuracy [k] in percent), plus the fault-free accuracy as `self.control_accuracy`.  The accuracies
        come from the labels, the fault-free classes and the sparse per-fault differences."""
        if target_type not in (0, 1):
            raise ValueError("sensitivity: target_type must be 0 (weights) or 1 (thresholds)")
        classifier = self.classifier_cls(self.network, self.dataset, self.runtime)
        records = [classifier.bnn.enumerate_faults(l, target_type, word_size) for l in layers]
        records = np.concatenate(records) if records else np.zeros((0, 8), np.int32)
        clean = np.asarray(self._classify(classifier, ""), np.int64)
        labels = np.asarray(list(self.labels), np.int64)
        n = len(labels)
        right = clean[:n] == labels
        changed, diffs = self._classify(classifier, "_fault_sweep", records)
        accuracy = self._accuracies(len(records), diffs, labels, right)
        print("{}-{}: {} single faults in layer(s) {} swept, {} change some image".format(
            self.network, self.dataset, len(records), list(layers), int((changed > 0).sum())))
        return records, changed, accuracy

    def _accuracies(self, k, diffs, labels, right):
        """accuracy in percent of each of k faults from its sparse differences; sets self.control_accuracy"""
        n = len(labels)
        # per fault: the fault-free count of right answers, minus those a changed class breaks, plus those it mends
        delta = np.zeros(k, np.int64)
        img, cls = diffs[:, 1], diffs[:, 2].astype(np.int64)
        ok = img < n
        now = np.zeros(len(diffs), np.int64)
        now[ok] = (cls[ok] == labels[img[ok]]).astype(np.int64) - right[img[ok]].astype(np.int64)
        np.add.at(delta, diffs[:, 0], now)
        self.control_accuracy = 100.0 * right.sum() / n if n else 0.0
        return 100.0 * (right.sum() + delta) / n if n else np.zeros(k)

    def activation_sensitivity(self, layers):
        """Every single activation fault of the outputs of `layers` (any layer but the last): each site x shift alone on
        the whole input set.  -> {layer: dict} with "records" int32 [k, 5] {layer, y, x, channel, shift}, "changed" [k]
        (images whose class the fault changes), "accuracy" [k] in percent, and the same two reshaped to the layer's map,
        "changed map" / "accuracy map" of shape (H, W, C) for 1-bit activations, (H, W, C, 2) for 2-bit ones (the
        shifts).  The fault-free accuracy is `self.control_accuracy`."""
        classifier = self.classifier_cls(self.network, self.dataset, self.runtime)
        per = [classifier.bnn.enumerate_act_faults(l) for l in layers]
        records = np.concatenate(per) if per else np.zeros((0, 5), np.int32)
        clean = np.asarray(self._classify(classifier, ""), np.int64)
        labels = np.asarray(list(self.labels), np.int64)
        right = clean[:len(labels)] == labels
        changed, diffs = self._classify(classifier, "_act_fault_sweep", records)
        accuracy = self._accuracies(len(records), diffs, labels, right)
        out, at = {}, 0
        for layer, rec in zip(layers, per):
            k = len(rec)
            h, w, c = (int(rec[:, i].max()) + 1 for i in (1, 2, 3))
            shifts = int(rec[:, 4].max())
            shape = (h, w, c) if shifts == 1 else (h, w, c, shifts)
            out[layer] = {"records": rec, "changed": changed[at:at + k], "accuracy": accuracy[at:at + k],
                          "changed map": changed[at:at + k].reshape(shape), "accuracy map": accuracy[at:at + k].reshape(shape)}
            at += k
        print("{}-{}: {} activation faults in layer(s) {} swept, {} change some image".format(
            self.network, self.dataset, len(records), list(layers), int((changed > 0).sum())))
        return out


    def run_noise_test(self, num_runs, rates, seed=0):
        """num_runs independent runs with every activation of layer L's output upset with probability rates[L] (a
        scalar: every layer but the last) -> accuracy per run in percent.  Run r draws with seed + r (0:
        std::random_device).  Left behind: self.noise_results (classes, [run, image]), self.noise_counts (upsets,
        [run, layer]) and self.noise_usec (device time per image of every run)."""
        classifier = self.classifier_cls(self.network, self.dataset, self.runtime)
        print("{}-{}: {} run(s) in one call, activation upset rate(s) {}".format(self.network, self.dataset, num_runs, rates))
        results, counts = self._classify(classifier, "_act_noise", num_runs, rates, seed)
        self.noise_results, self.noise_counts, self.noise_usec = results, counts, classifier.usecPerImage
        accuracies = [util.calculate_accuracy(row.tolist(), self.labels) for row in results]
        print("Accuracies:", accuracies)
        print()
        return accuracies

    def run_memory_noise_test(self, num_runs, rates_w, rates_t, seed=0, scheme=None, burst=1, code=0, weight_code=0, weight_interleave=0):
        """weight_interleave 1 (with weight_code 1: the code words column-interleaved, csrc/mem_org.h): the same through
        inference_multiple_iwecc_exposure.  weight_code 1 (SEC-DED (72,64) coded weight memories of the layers >= 1, csrc/wecc.h; any scheme and code): likewise
        one epoch of the exposure campaign, the counts [run, layer, 12] as run_exposure_test's.  code 1 (SEC-DED coded threshold memories, csrc/ecc.h; scheme 0 or 2): the exposure campaign with one epoch, which
        is the one-shot campaign; the counts are then [run, layer, 6] as run_exposure_test's.  scheme (0 ... 3, HARDENING_SCHEMES) or burst > 1: the upsets hit the physical memories of that hardened
        organisation in bursts of `burst` adjacent bits, and the counts are [run, layer, 2, 2: physical bits flipped,
        logical bits that differ after voting and de-interleaving].  Else (today's path, unchanged) num_runs independent runs with every bit of layer L's weight memory flipped with probability rates_w[L] and
        every bit of its threshold memory with rates_t[L] (scalars: every layer; thresholds: every layer that has any), in
        place from the first image on -> (accuracy per run in percent, flips applied [run, layer, 2: weights,
        thresholds]).  Run r draws with seed + r (0: std::random_device).  Left behind: self.mem_noise_results (classes,
        [run, image]), self.mem_noise_counts and self.mem_noise_usec (device time per image of every run)."""
        classifier = self.classifier_cls(self.network, self.dataset, self.runtime)
        print("{}-{}: {} run(s) in one call, memory upset rate(s) weights {} thresholds {}".format(
            self.network, self.dataset, num_runs, rates_w, rates_t))
        if weight_interleave and not weight_code:
            raise ValueError("run_memory_noise_test: weight_interleave 1 needs weight_code 1")
        if weight_code or code:
            print("  memory organisation: {}, bursts of {}".format(organisation_name(scheme or 0, code, weight_code, weight_interleave), burst))
            results, counts = self._classify(classifier, "_exposure", num_runs, rates_w, rates_t, 1 << 30, 0, scheme or 0, burst, seed, code=code,
                                             repair_every=0, weight_code=weight_code, weight_interleave=weight_interleave)
            counts = counts[:, 0]  # (the one epoch)
        else:
            if scheme is not None or burst != 1:
                print("  memory organisation: {}, bursts of {}".format(HARDENING_SCHEMES[scheme or 0], burst))
            results, counts = self._classify(classifier, "_mem_noise", num_runs, rates_w, rates_t, seed, scheme, burst)
        self.mem_noise_results, self.mem_noise_counts, self.mem_noise_usec = results, counts, classifier.usecPerImage
        accuracies = [util.calculate_accuracy(row.tolist(), self.labels) for row in results]
        print("Accuracies:", accuracies)
        print()
        return accuracies, counts

    def run_exposure_test(self, num_runs, rates_w, rates_t, epoch_images, scrub_every=0, scheme=None, burst=1, seed=0, code=0, repair_every=0,
                          weight_code=0, weight_interleave=0):
        """Upsets that accumulate while the run goes on: the images are cut into epochs of `epoch_images`, rates_w[L] /
        rates_t[L] are the probability of an event PER EPOCH (scalars: every layer), an epoch's upsets XOR onto the physical
        state of the hardened organisation `scheme` (None: 0) the earlier epochs left, and every `scrub_every` epochs (0:
        never) the memories are rewritten.  -> (accuracy in percent [run][epoch], over the epoch's images; counts [run,
        epoch, layer, 2: weights, thresholds, 2: physical bits flipped in the epoch, logical bits that differ after it]).
        code 1: the 16-bit threshold memories carry a SEC-DED code (csrc/ecc.h; scheme 0 or 2; weights and CNV layer 0 are
        not coded) and the counts are [run, epoch, layer, 6: weights physical, logical; thresholds physical (data plus check
        bits), logical (after decoding); threshold words corrected; detected as uncorrectable].
        repair_every > 0: before every epoch t > 0 with t % repair_every == 0 that is no rewrite epoch the memories with
        redundancy (TMR modules, coded thresholds) are repaired -- read, voted or decoded, written back -- which fixes only
        what the redundancy covers and locks in what it gets wrong; the counts are then [run, epoch, layer, 8: the six
        above, the words the epoch's repair rewrote, the words of the repaired memories still unlike the loaded ones].
        weight_code 1: the weight memories of every layer but CNV layer 0 carry a SEC-DED (72,64) code (csrc/wecc.h; any
        scheme, code and repair_every; a repair also rewrites status-1 weight code words) and the counts are [run, epoch,
        layer, 12: the eight above, weight code words corrected, detected as uncorrectable, rewritten by the epoch's
        repair, still unlike the loaded ones after it].
        Left behind: self.exposure_results (classes, [run, image]), self.exposure_counts, self.exposure_usec."""
        classifier = self.classifier_cls(self.network, self.dataset, self.runtime)
        print("{}-{}: {} run(s) in one call, epochs of {} images, upset rate(s) per epoch weights {} thresholds {}, {}, bursts of {}, "
              "scrub every {}{}".format(self.network, self.dataset, num_runs, epoch_images, rates_w, rates_t,
                                        organisation_name(scheme or 0, code, weight_code, weight_interleave), burst, scrub_every or "never",
                                        ", repair every {}".format(repair_every) if repair_every else ""))
        results, counts = self._classify(classifier, "_exposure", num_runs, rates_w, rates_t, epoch_images, scrub_every, scheme or 0, burst, seed,
                                         code=code, repair_every=repair_every, weight_code=weight_code, weight_interleave=weight_interleave)
        self.exposure_results, self.exposure_counts, self.exposure_usec = results, counts, classifier.usecPerImage
        accuracies = [[util.calculate_accuracy(row[i: i + epoch_images].tolist(), self.labels[i: i + epoch_images])
                       for i in range(0, results.shape[1], epoch_images)] for row in results]
        print("Accuracies per epoch:", accuracies)
        print()
        return accuracies, counts

    def input_sensitivity(self, records=None):
        """Single input-bit faults: each record {byte, bit} (None: every bit of the image, in site order) flipped alone
        while each image of the input set is classified.  -> (records int32 [k, 2], changed [k]: images whose class the
        flip changes, accuracy [k] in percent), plus the fault-free accuracy as `self.control_accuracy`."""
        classifier = self.classifier_cls(self.network, self.dataset, self.runtime)
        records = classifier.bnn.enumerate_input_faults() if records is None else np.asarray(records, np.int32).reshape(-1, 2)
        clean = np.asarray(self._classify(classifier, ""), np.int64)
        labels = np.asarray(list(self.labels), np.int64)
        right = clean[:len(labels)] == labels
        changed, diffs = self._classify(classifier, "_input_fault_sweep", records)
        accuracy = self._accuracies(len(records), diffs, labels, right)
        print("{}-{}: {} input bits swept, {} change some image".format(
            self.network, self.dataset, len(records), int((changed > 0).sum())))
        return records, changed, accuracy

    def propagation(self, kind, layers=(), target_type=0, word_size=1, records=None):
        """Where single faults are masked.  kind "parameter": every distinct fault of `layers` (target_type 0 weights / 1
        thresholds, word_size adjacent bits); "activation": every site x shift of the outputs of `layers`; "input": every
        bit of the image -- or the given `records` of that kind -- each alone on the whole input set, with the sweep's
        propagation profile recorded (PynqBNN.sweep_profile; the setting found is put back afterwards).  -> dict with
        "records", "changed" [k] (images whose class the fault changes), "alive" and "flipped" int64 [k, layers - 1]
        (PynqBNN.last_sweep_profile) and "images", the size of the input set."""
        methods = {"parameter": ("_fault_sweep", 8), "activation": ("_act_fault_sweep", 5), "input": ("_input_fault_sweep", 2)}
        if kind not in methods:
            raise ValueError('propagation: kind is one of "parameter", "activation", "input"')
        method, width = methods[kind]
        classifier = self.classifier_cls(self.network, self.dataset, self.runtime)
        if records is not None:
            records = np.asarray(records, np.int32).reshape(-1, width)
        elif kind == "input":
            records = classifier.bnn.enumerate_input_faults()
        else:
            per = [classifier.bnn.enumerate_faults(l, target_type, word_size) if kind == "parameter"
                   else classifier.bnn.enumerate_act_faults(l) for l in layers]
            records = np.concatenate(per) if per else np.zeros((0, width), np.int32)
        before = classifier.bnn.sweep_profile(True)
        try:
            changed, _ = self._classify(classifier, method, records, 0)
            alive, flipped = classifier.bnn.last_sweep_profile()
        finally:
            classifier.bnn.sweep_profile(before)
        print("{}-{}: {} {} faults swept with their propagation, {} change some image".format(
            self.network, self.dataset, len(records), kind, int((changed > 0).sum())))
        return {"records": records, "changed": changed, "alive": alive, "flipped": flipped, "images": len(list(self.labels))}

    def run_input_noise_test(self, num_runs, rate, seed=0):
        """num_runs independent runs with every bit of every input image flipped with probability `rate` -> accuracy per
        run in percent.  Run r draws with seed + r (0: std::random_device).  Left behind: self.input_noise_results
        (classes, [run, image]), self.input_noise_counts (bits flipped, [run]) and self.input_noise_usec (device time
        per image of every run)."""
        classifier = self.classifier_cls(self.network, self.dataset, self.runtime)
        print("{}-{}: {} run(s) in one call, input-buffer upset rate {}".format(self.network, self.dataset, num_runs, rate))
        results, counts = self._classify(classifier, "_input_noise", num_runs, rate, seed)
        self.input_noise_results, self.input_noise_counts, self.input_noise_usec = results, counts, classifier.usecPerImage
        accuracies = [util.calculate_accuracy(row.tolist(), self.labels) for row in results]
        print("Accuracies:", accuracies)
        print()
        return accuracies



class CNVFaultTest(FaultTest):
    def __init__(self, network, dataset, input_file, labels, runtime=_bnn.RUNTIME_HW):
        super().__init__(_bnn.CnvClassifier, network, dataset, input_file, labels, runtime)

    @classmethod
    def CIFARTest(cls, network, input_file, labels):
        return cls(network, "cifar10", input_file, labels)

    @classmethod
    def SVHNTest(cls, network, input_file, labels):
        return cls(network, "streetview", input_file, labels)

    @classmethod
    def GTSRBTest(cls, network, input_file, labels):
        return cls(network, "road-signs", input_file, labels)


class LFCFaultTest(FaultTest):
    def __init__(self, network, dataset, input_file, labels, runtime=_bnn.RUNTIME_HW):
        super().__init__(_bnn.LfcClassifier, network, dataset, input_file, labels, runtime)

    @classmethod
    def MNISTTest(cls, network, input_file, labels):
        return cls(network, "mnist", input_file, labels)


class NetworkTest:
    class TestType:
        def __init__(self, target_type, word_size):
            self.target_type = target_type
            self.word_size = word_size
            where = {-1: "any", 0: "weight"}.get(target_type, "threshold")
            self.name = where + " " + ("word" if word_size > 1 else "bit")

        @classmethod
        def any_bit(cls):
            return cls(FaultTest.TargetType.any(), 1)

        @classmethod
        def any_word(cls, word_size=8):
            return cls(FaultTest.TargetType.any(), word_size)

        @classmethod
        def weight_bit(cls):
            return cls(FaultTest.TargetType.weights(), 1)

        @classmethod
        def weight_word(cls, word_size=8):
            return cls(FaultTest.TargetType.weights(), word_size)

        @classmethod
        def threshold_bit(cls):
            return cls(FaultTest.TargetType.thresholds(), 1)

        @classmethod
        def threshold_word(cls, word_size=8):
            return cls(FaultTest.TargetType.thresholds(), word_size)

    def __init__(self, fault_test):
        self.fault_test = fault_test
        self.control = None

    def _run_control(self, batched=False):
        print("Running", self.fault_test.network + "-" + self.fault_test.dataset, "control test")
        _, _, accuracy = self.fault_test.run_test(num_runs=1, num_flips=0, batched=batched)
        self.control = accuracy[0]

    def _raw(self, name, num_runs, num_flips, layers, accuracies):
        return {"network": self.fault_test.network, "dataset": self.fault_test.dataset, "run count": num_runs,
                "flips": num_flips, "control": self.control, "layers": list(layers), "results": {name: accuracies}}

    def _stats(self, merged):
        out = dict(merged)
        out["results"] = {}
        for name, runs in merged["results"].items():
            effective = [a for a in runs if a != merged["control"]]
            entry = {"runs": {"all": runs, "effective": effective}, "effective count": len(effective),
                     "min accuracy": min(runs), "max accuracy": max(runs)}
            if effective:
                entry["avg accuracy"] = sum(runs) / len(runs)
                entry["avg effective accuracy"] = sum(effective) / len(effective)
                entry["accuracy delta"] = merged["control"] - entry["avg accuracy"]
                entry["effective accuracy delta"] = merged["control"] - entry["avg effective accuracy"]
            else:
                entry["avg accuracy"] = merged["control"]
            out["results"][name] = entry
        return out

    def _run_tests(self, folder, num_runs, num_flips, test_types, target_layers, batched=False, seed=0):
        raw = []
        for test in test_types:
            _, _, accuracies = self.fault_test.run_test(num_runs, num_flips, test.word_size, test.target_type, target_layers,
                                                        batched, seed)
            raw.append(self._raw(test.name, num_runs, num_flips, target_layers, accuracies))
            util.write_dict_to_file("{}/temp/{}_results_{}.json".format(folder, self.fault_test.network, test.name.replace(" ", "-")), raw[-1])
        return self._stats(util.dict_of_dicts_merge(*raw))

    def test_network(self, output_folder, num_runs, flip_counts, test_types, target_layers=(), batched=False, seed=0):
        """one statistics file per fault count under output_folder/<network>/<dataset>/<n>flips/.
        batched / seed: see FaultTest.run_test (each test's runs in one call; run i seeded with seed + i)."""
        output_folder = "{}/{}/{}/".format(output_folder, self.fault_test.network, self.fault_test.dataset)
        if self.control is None:
            self._run_control(batched)
        for num_flips in flip_counts:
            folder = "{}/{}flips/".format(output_folder, num_flips)
            stats = self._run_tests(folder, num_runs, num_flips, test_types, target_layers, batched, seed)
            name = "{}/{}_{}".format(folder, self.fault_test.network, self.fault_test.dataset)
            name += "_stats_layer{}.json".format(list(target_layers)) if len(target_layers) > 0 else "_stats.json"
            util.write_dict_to_file(name, stats)

    def sensitivity_map(self, output_folder, layers, test_types):
        """Exhaustive single-fault sweeps (FaultTest.sensitivity): per layer and test type (its target_type: weights or
        thresholds, and word size) one file output_folder/<network>/<dataset>/sensitivity/<network>_layer<L>_<type>.json
        with every fault's record, changed-image count and accuracy, and one per-layer summary file next to them: per
        test type the mean and max changed-image count, the fraction of faults that change any image, mean / min
        accuracy and the fault-free accuracy."""
        folder = "{}/{}/{}/sensitivity/".format(output_folder, self.fault_test.network, self.fault_test.dataset)
        for layer in layers:
            summary = {"network": self.fault_test.network, "dataset": self.fault_test.dataset, "layer": layer, "results": {}}
            for test in test_types:
                if test.target_type not in (0, 1):
                    raise ValueError("sensitivity_map: test types target weights or thresholds, not any")
                records, changed, accuracy = self.fault_test.sensitivity([layer], test.target_type, test.word_size)
                summary["control"] = self.fault_test.control_accuracy
                name = test.name.replace(" ", "-")
                util.write_dict_to_file("{}/{}_layer{}_{}.json".format(folder, self.fault_test.network, layer, name), {
                    "network": self.fault_test.network, "dataset": self.fault_test.dataset, "layer": layer,
                    "test": test.name, "word size": test.word_size, "control": self.fault_test.control_accuracy,
                    "fields": ["target", "layer", "mem", "ind", "thresh", "bit", "word_size", "changed", "accuracy"],
                    "faults": [[int(x) for x in r[1:]] + [int(c), float(a)] for r, c, a in zip(records, changed, accuracy)]})
                k = len(records)
                summary["results"][test.name] = {
                    "faults": k,
                    "mean changed": float(changed.mean()) if k else 0.0,
                    "max changed": int(changed.max()) if k else 0,
                    "fraction changing any image": float((changed > 0).mean()) if k else 0.0,
                    "mean accuracy": float(accuracy.mean()) if k else summary["control"],
                    "min accuracy": float(accuracy.min()) if k else summary["control"]}
            util.write_dict_to_file("{}/{}_layer{}_summary.json".format(folder, self.fault_test.network, layer), summary)

    def activation_sensitivity_map(self, output_folder, layers):
        """Activation-fault sweeps (FaultTest.activation_sensitivity), next to sensitivity_map's files: per layer one
        file output_folder/<network>/<dataset>/sensitivity/<network>_layer<L>_activations.json with the layer's totals
        (sites, faults, mean / max changed images, fraction of faults that change any image, mean / min accuracy, the
        fault-free accuracy) and its vulnerability -- the fraction of images a fault changes, averaged over the shifts --
        per channel (over the pixels) and per pixel (over the channels, an H x W grid), plus every fault's changed
        count in record order."""
        folder = "{}/{}/{}/sensitivity/".format(output_folder, self.fault_test.network, self.fault_test.dataset)
        res = self.fault_test.activation_sensitivity(list(layers))
        n = max(len(list(self.fault_test.labels)), 1)
        for layer, r in res.items():
            cm = r["changed map"].astype(np.float64)
            vul = (cm if cm.ndim == 3 else cm.mean(axis=3)) / n  # (H, W, C)
            k = len(r["records"])
            util.write_dict_to_file("{}/{}_layer{}_activations.json".format(folder, self.fault_test.network, layer), {
                "network": self.fault_test.network, "dataset": self.fault_test.dataset, "layer": layer,
                "control": self.fault_test.control_accuracy, "map": list(vul.shape), "shifts": 1 if cm.ndim == 3 else cm.shape[3],
                "totals": {"sites": int(vul.size), "faults": k,
                           "mean changed": float(r["changed"].mean()) if k else 0.0,
                           "max changed": int(r["changed"].max()) if k else 0,
                           "fraction changing any image": float((r["changed"] > 0).mean()) if k else 0.0,
                           "mean accuracy": float(r["accuracy"].mean()) if k else self.fault_test.control_accuracy,
                           "min accuracy": float(r["accuracy"].min()) if k else self.fault_test.control_accuracy},
                "per channel vulnerability": vul.mean(axis=(0, 1)).tolist(),
                "per pixel vulnerability": vul.mean(axis=2).tolist(),
                "fields": ["layer", "y", "x", "channel", "shift", "changed"],
                "changed": [int(c) for c in r["changed"]]})

    def upset_rate_curve(self, output_folder, num_runs, rates, layers=(), seed=0):
        """The accuracy-versus-upset-rate curve of the datapath (FaultTest.run_noise_test).  `layers`: layer sets -- each
        a list of layers whose outputs are upset, or one layer number; empty: one set, every layer but the last.  Per
        (layer set, rate p) one statistics file in the format test_network writes,
        output_folder/<network>/<dataset>/upsets/<network>_<dataset>_rate<p>_stats[_layer<set>].json: the runs'
        accuracies with min / max / average and the effective runs, plus "stddev accuracy", the nominal "rate" and
        the "effective rate" the runs actually saw (upsets counted on the device / sites exposed), with the upsets per
        layer summed over the runs."""
        ft = self.fault_test
        folder = "{}/{}/{}/upsets/".format(output_folder, ft.network, ft.dataset)
        if self.control is None:  # (rate 0: the fault-free classes)
            self.control = ft.run_noise_test(1, 0.0, seed or 1)[0]
        classifier = ft.classifier_cls(ft.network, ft.dataset, ft.runtime)
        nl = len(classifier.bnn.act_noise_rates(0.0))
        sets = [[int(l)] if np.isscalar(l) else [int(x) for x in l] for l in layers] or [list(range(nl))]
        sites = np.array([len(classifier.bnn.enumerate_act_faults(l)) // (2 if ft.network.endswith("A2") else 1) for l in range(nl)])
        for which in sets:
            for p in rates:
                per_layer = [float(p) if l in which else 0.0 for l in range(nl)]
                accuracies = ft.run_noise_test(num_runs, per_layer, seed)
                name = "upset rate {:g}".format(p)
                stats = self._stats(self._raw(name, num_runs, 0, which, accuracies))
                exposed = float(sites[which].sum()) * num_runs * ft.noise_results.shape[1]
                stats["results"][name].update({
                    "stddev accuracy": float(np.std(accuracies)), "rate": float(p),
                    "effective rate": float(ft.noise_counts[:, which].sum()) / exposed if exposed else 0.0,
                    "upsets per layer": [int(c) for c in ft.noise_counts.sum(axis=0)]})
                out = "{}/{}_{}_rate{:g}_stats".format(folder, ft.network, ft.dataset, p)
                out += ".json" if len(which) == nl else "_layer{}.json".format(which)
                util.write_dict_to_file(out, stats)

    def memory_upset_rate_curve(self, output_folder, num_runs, rates, layers=(), targets=("weights", "thresholds"), seed=0, scheme=None,
                                burst=1):
        """scheme / burst: as run_memory_noise_test takes them (None and 1: today's path); the flips counted are then the
        physical bits.  The accuracy-versus-upset-rate curve of the parameter memories (FaultTest.run_memory_noise_test), per memory
        kind.  `layers`: layer sets -- each a list of layers whose memories are upset, or one layer number; empty: one set,
        every layer (thresholds: every layer that has threshold memory).  Per target one file in the format of
        upset_rate_curve, output_folder/<network>/<dataset>/memory-upsets/<network>_<dataset>_<target>_stats.json, with
        one result per (layer set, rate p): the runs' accuracies with min / max / average and the effective runs, plus
        "stddev accuracy", the nominal "rate", the "effective rate" the runs actually saw (flips applied / bits exposed)
        and the flips per layer summed over the runs."""
        ft = self.fault_test
        folder = "{}/{}/{}/memory-upsets/".format(output_folder, ft.network, ft.dataset)
        if self.control is None:  # (rate 0: the fault-free classes)
            self.control = ft.run_memory_noise_test(1, 0.0, 0.0, seed or 1)[0][0]
        classifier = ft.classifier_cls(ft.network, ft.dataset, ft.runtime)
        nl = len(classifier.bnn.mem_noise_rates(0.0))
        for target in targets:
            t = {"weights": 0, "thresholds": 1}[target]
            bits = np.array([len(classifier.bnn.enumerate_faults(l, t, 1)) for l in range(nl)])
            have = [l for l in range(nl) if bits[l]]
            sets = [[int(l)] if np.isscalar(l) else [int(x) for x in l] for l in layers] or [have]
            raw = []
            extra = {}
            for which in sets:
                for p in rates:
                    per_layer = [float(p) if l in which else 0.0 for l in range(nl)]
                    zeros = [0.0] * nl
                    accuracies, counts = ft.run_memory_noise_test(num_runs, zeros if t else per_layer, per_layer if t else zeros, seed, scheme, burst)
                    if counts.ndim == 4:
                        counts = counts[..., 0]
                    name = "{} upset rate {:g}".format(target, p) + ("" if which == have else " layer{}".format(which))
                    raw.append(self._raw(name, num_runs, 0, which, accuracies))
                    exposed = float(bits[which].sum()) * num_runs
                    extra[name] = {"stddev accuracy": float(np.std(accuracies)), "rate": float(p), "layers": which,
                                   "effective rate": float(counts[:, which, t].sum()) / exposed if exposed else 0.0,
                                   "flips per layer": [int(c) for c in counts[:, :, t].sum(axis=0)]}
            stats = self._stats(util.dict_of_dicts_merge(*raw))
            stats["layers"] = sorted({l for which in sets for l in which})
            for name, e in extra.items():
                stats["results"][name].update(e)
            util.write_dict_to_file("{}/{}_{}_{}_stats.json".format(folder, ft.network, ft.dataset, target), stats)

    def hardening_curve(self, output_folder, num_runs, rates, schemes, bursts=(1,), seed=0):
        """What a hardened memory organisation buys: the accuracy at upset rate p of every weight and threshold memory, per
        (scheme, burst, rate), the same seeds for every scheme.  One file in the format of upset_rate_curve,
        output_folder/<network>/<dataset>/hardening/<network>_<dataset>_hardening_stats.json, with one result
        "<scheme name> burst <b> upset rate <p>" per combination: the runs' accuracies with min / max / average, plus
        "stddev accuracy", "scheme", "burst", "rate" and the "physical bits" flipped and "logical bits" that differ after
        voting and de-interleaving, summed over the runs.  An entry of `schemes` may be a (scheme, code) pair (code 1: SEC-DED
        coded threshold memories): its name is "<scheme name> + SEC-DED", and it also writes "code", "corrected words" and
        "detected words".  A (scheme, code, weight_code) triple (weight_code 1: SEC-DED (72,64) coded weight memories):
        the name holds " + SEC-DED weights", and it also writes "weight code", "corrected weight words" and "detected weight
        words".  A (scheme, code, weight_code, weight_interleave) 4-tuple (weight_interleave 1: those code words
        column-interleaved): the name ends in " column-interleaved", and it also writes "weight interleave"."""
        ft = self.fault_test
        folder = "{}/{}/{}/hardening/".format(output_folder, ft.network, ft.dataset)
        if self.control is None:  # (rate 0: the fault-free classes)
            self.control = ft.run_memory_noise_test(1, 0.0, 0.0, seed or 1)[0][0]
        raw, extra = [], {}
        for org in map(organisation, schemes):
            for burst in bursts:
                for p in rates:
                    accuracies, counts = ft.run_memory_noise_test(num_runs, float(p), float(p), seed, org.scheme, burst, code=org.code,
                                                                  weight_code=org.weight_code, weight_interleave=org.weight_interleave)
                    c = upset_counts(counts)
                    name = "{} burst {} upset rate {:g}".format(organisation_name(*org), burst, p)
                    raw.append(self._raw(name, num_runs, 0, [], accuracies))
                    e = extra[name] = {"stddev accuracy": float(np.std(accuracies)), "scheme": org.scheme, "burst": int(burst), "rate": float(p)}
                    if org.weight_interleave:
                        e["weight interleave"] = org.weight_interleave
                    if org.weight_code:
                        e.update({"weight code": org.weight_code, "corrected weight words": int(c.weight_corrected.sum()),
                                  "detected weight words": int(c.weight_detected.sum())})
                    if org.code:
                        e["code"] = org.code
                    e.update({"physical bits": int(c.weights_physical.sum() + c.thresholds_physical.sum()),
                              "logical bits": int(c.weights_logical.sum() + c.thresholds_logical.sum())})
                    if org.code:
                        e.update({"corrected words": int(c.corrected.sum()), "detected words": int(c.detected.sum())})
        stats = self._stats(util.dict_of_dicts_merge(*raw))
        for name, e in extra.items():
            stats["results"][name].update(e)
        util.write_dict_to_file("{}/{}_{}_hardening_stats.json".format(folder, ft.network, ft.dataset), stats)

    def scrubbing_curve(self, output_folder, num_runs, rates, scrub_intervals, schemes, epoch_images, bursts=(1,), seed=0):
        """How often must the memories be rewritten: the accuracy per epoch while upsets accumulate at rate p per epoch in
        every weight and threshold memory, per (scheme, burst, rate, scrub interval), the same seeds everywhere.  One file
        in the style of hardening_curve, output_folder/<network>/<dataset>/scrubbing/<network>_<dataset>_scrubbing_stats.json,
        with one result "<scheme name> burst <b> upset rate <p> scrub every <S>" per combination: the runs' accuracies over
        ALL images with min / max / average, plus "mean accuracy per epoch" (over the runs), "scheme", "burst", "rate",
        "scrub every", "epoch images" and the "physical bits" flipped (summed over runs and epochs) and "logical bits per
        epoch" that differ after each epoch (summed over the runs).  An entry of `schemes` may be a (scheme, code) pair (code 1:
        SEC-DED coded threshold memories): its name is "<scheme name> + SEC-DED", and it also writes "code" and the
        "corrected words per epoch" and "detected words per epoch" (summed over the runs).  An entry of `scrub_intervals`
        may be a (scrub_every, repair_every) pair (run_exposure_test's repair scrub); with a non-zero repair_every the name
        ends in " repair every <P>" and the result also holds "repair every", "repaired words per epoch" and "unrepaired
        words per epoch" (summed over the runs).  An entry of `schemes` may also be a (scheme, code, weight_code) triple
        (weight_code 1: SEC-DED (72,64) coded weight memories of the layers >= 1): the name holds " + SEC-DED weights", and the
        result also holds "weight code" and the "corrected / detected / repaired / unrepaired weight words per epoch"; a
        (scheme, code, weight_code, weight_interleave) 4-tuple (weight_interleave 1: those code words column-interleaved)
        adds " column-interleaved" to the name and "weight interleave" to the result."""
        ft = self.fault_test
        folder = "{}/{}/{}/scrubbing/".format(output_folder, ft.network, ft.dataset)
        if self.control is None:  # (rate 0: the fault-free classes)
            self.control = ft.run_memory_noise_test(1, 0.0, 0.0, seed or 1)[0][0]
        raw, extra = [], {}
        def per_epoch_sum(a):
            return [int(x) for x in a.sum(axis=(0, 2))]  # (over the runs and the layers)

        for org in map(organisation, schemes):
            for burst in bursts:
                for p in rates:
                    for every in scrub_intervals:
                        every, repair = (int(every[0]), int(every[1])) if isinstance(every, (tuple, list)) else (every, 0)
                        per_epoch, counts = ft.run_exposure_test(num_runs, float(p), float(p), epoch_images, every, org.scheme, burst, seed,
                                                                 code=org.code, repair_every=repair, weight_code=org.weight_code,
                                                                 weight_interleave=org.weight_interleave)
                        c = upset_counts(counts)
                        accuracies = [util.calculate_accuracy(row.tolist(), ft.labels) for row in ft.exposure_results]
                        name = "{} burst {} upset rate {:g} scrub every {}".format(organisation_name(*org), burst, p, every)
                        if repair:
                            name += " repair every {}".format(repair)
                        raw.append(self._raw(name, num_runs, 0, [], accuracies))
                        e = extra[name] = {"mean accuracy per epoch": [float(x) for x in np.mean(np.array(per_epoch, float), axis=0)],
                                           "scheme": org.scheme, "burst": int(burst), "rate": float(p), "scrub every": int(every),
                                           "epoch images": int(epoch_images),
                                           "physical bits": int(c.weights_physical.sum() + c.thresholds_physical.sum()),
                                           "logical bits per epoch": per_epoch_sum(c.weights_logical + c.thresholds_logical)}
                        if org.weight_interleave:
                            e["weight interleave"] = org.weight_interleave
                        if org.weight_code:
                            e.update({"weight code": org.weight_code, "corrected weight words per epoch": per_epoch_sum(c.weight_corrected),
                                      "detected weight words per epoch": per_epoch_sum(c.weight_detected),
                                      "repaired weight words per epoch": per_epoch_sum(c.weight_repaired),
                                      "unrepaired weight words per epoch": per_epoch_sum(c.weight_unrepaired)})
                        if repair:
                            e.update({"repair every": repair, "repaired words per epoch": per_epoch_sum(c.repaired),
                                      "unrepaired words per epoch": per_epoch_sum(c.unrepaired)})
                        if org.code:
                            e.update({"code": org.code, "corrected words per epoch": per_epoch_sum(c.corrected),
                                      "detected words per epoch": per_epoch_sum(c.detected)})
        stats = self._stats(util.dict_of_dicts_merge(*raw))
        for name, e in extra.items():
            stats["results"][name].update(e)
        util.write_dict_to_file("{}/{}_{}_scrubbing_stats.json".format(folder, ft.network, ft.dataset), stats)

    def input_sensitivity_map(self, output_folder):
        """The input-bit sweep (FaultTest.input_sensitivity) over every bit of the image, next to sensitivity_map's files:
        output_folder/<network>/<dataset>/sensitivity/<network>_input.json with the totals (sites, mean / max changed
        images, fraction of bits that change any image, mean / min accuracy, the fault-free accuracy), the vulnerability
        -- the fraction of images a flip changes -- per bit position (over the pixels) and per pixel (over the bits), and
        every site's changed count in site order.  -> the changed counts shaped like the image with a last axis of 8
        bits (bit 0 the LSB): (3, 32, 32, 8) for the CNV networks (planar CHW), (28, 28, 8) for the LFC ones."""
        ft = self.fault_test
        folder = "{}/{}/{}/sensitivity/".format(output_folder, ft.network, ft.dataset)
        records, changed, accuracy = ft.input_sensitivity()
        shape = (3, 32, 32, 8) if len(records) == 3072 * 8 else (28, 28, 8)
        cm = np.asarray(changed).reshape(shape)
        n = max(len(list(ft.labels)), 1)
        vul = cm.astype(np.float64) / n
        k = len(records)
        util.write_dict_to_file("{}/{}_input.json".format(folder, ft.network), {
            "network": ft.network, "dataset": ft.dataset, "control": ft.control_accuracy, "map": list(shape),
            "totals": {"sites": k,
                       "mean changed": float(changed.mean()) if k else 0.0,
                       "max changed": int(changed.max()) if k else 0,
                       "fraction changing any image": float((changed > 0).mean()) if k else 0.0,
                       "mean accuracy": float(accuracy.mean()) if k else ft.control_accuracy,
                       "min accuracy": float(accuracy.min()) if k else ft.control_accuracy},
            "per bit vulnerability": vul.reshape(-1, 8).mean(axis=0).tolist(),
            "per pixel vulnerability": vul.mean(axis=-1).tolist(),
            "fields": ["byte", "bit", "changed"],
            "changed": [int(c) for c in changed]})
        return cm

    def propagation_map(self, output_folder, kind, layers=(), target_type=0, word_size=1):
        """Masking per layer (FaultTest.propagation), next to sensitivity_map's files: per site layer of `layers` (kind
        "input": one site layer, the image) one file output_folder/<network>/<dataset>/sensitivity/<network>_layer<L>_
        <kind>_propagation.json (input: <network>_input_propagation.json) with the totals the other maps give (faults,
        mean / max changed images, fraction of faults that change any image) and, for every downstream layer from the
        first one the sweep evaluates for these faults on, "share alive" -- the share of (fault, image) pairs whose output
        of that layer still differs from the fault-free one, the masking curve -- and "mean error size", the activations
        that differ per image still alive, averaged over the faults alive there (propagation_curves).  -> {site layer:
        the file's dict}."""
        ft = self.fault_test
        folder = "{}/{}/{}/sensitivity/".format(output_folder, ft.network, ft.dataset)
        out = {}
        for layer in (["input"] if kind == "input" else list(layers)):
            r = ft.propagation(kind, [] if kind == "input" else [layer], target_type, word_size)
            first = 0 if kind == "input" else min(layer + (1 if kind == "activation" else 0), r["alive"].shape[1])
            share, size = propagation_curves(r["alive"], r["flipped"], r["images"], first)
            changed, k = r["changed"], len(r["records"])
            out[layer] = {
                "network": ft.network, "dataset": ft.dataset, "kind": kind, "layer": layer, "images": r["images"],
                "totals": {"faults": k,
                           "mean changed": float(changed.mean()) if k else 0.0,
                           "max changed": int(changed.max()) if k else 0,
                           "fraction changing any image": float((changed > 0).mean()) if k else 0.0},
                "downstream layers": list(range(first, r["alive"].shape[1])),
                "share alive": share, "mean error size": size}
            if kind == "parameter":
                out[layer].update({"target": target_type, "word size": word_size})
            name = "{}_input_propagation.json" if kind == "input" else "{}_layer" + str(layer) + "_" + kind + "_propagation.json"
            util.write_dict_to_file(folder + name.format(ft.network), out[layer])
        return out

    def input_upset_rate_curve(self, output_folder, num_runs, rates, seed=0):
        """The accuracy-versus-upset-rate curve of the input buffer (FaultTest.run_input_noise_test).  Per rate p one
        statistics file in the format test_network writes,
        output_folder/<network>/<dataset>/input-upsets/<network>_<dataset>_rate<p>_stats.json: the runs' accuracies with
        min / max / average and the effective runs, plus "stddev accuracy", the nominal "rate", the "effective rate" the
        runs actually saw (bits flipped on the device / bits exposed) and the flips summed over the runs."""
        ft = self.fault_test
        folder = "{}/{}/{}/input-upsets/".format(output_folder, ft.network, ft.dataset)
        if self.control is None:  # (rate 0: the fault-free classes)
            self.control = ft.run_input_noise_test(1, 0.0, seed or 1)[0]
        classifier = ft.classifier_cls(ft.network, ft.dataset, ft.runtime)
        bits = len(classifier.bnn.enumerate_input_faults())
        for p in rates:
            accuracies = ft.run_input_noise_test(num_runs, float(p), seed)
            name = "input upset rate {:g}".format(p)
            stats = self._stats(self._raw(name, num_runs, 0, [], accuracies))
            exposed = float(bits) * num_runs * ft.input_noise_results.shape[1]
            stats["results"][name].update({
                "stddev accuracy": float(np.std(accuracies)), "rate": float(p),
                "effective rate": float(ft.input_noise_counts.sum()) / exposed if exposed else 0.0,
                "flips": int(ft.input_noise_counts.sum())})
            util.write_dict_to_file("{}/{}_{}_rate{:g}_stats.json".format(folder, ft.network, ft.dataset, p), stats)

    def comprehensive_test(self, output_folder, num_runs, flip_counts, target_layers=()):
        """all six combinations of {any, weight, threshold} x {bit, 8-bit word}.  (The reference's version
        forgets to pass an output folder on to test_network, faults.py:254-261; here it is the first argument.)"""
        T = NetworkTest.TestType
        self.test_network(output_folder, num_runs, flip_counts,
                          [T.any_bit(), T.any_word(), T.weight_bit(), T.weight_word(), T.threshold_bit(), T.threshold_word()],
                          target_layers)
