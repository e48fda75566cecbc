/*
 * bnn_mi355x.h -- C ABI of the MI355X-native BNN-PYNQ runtime.
 *
 * One shared object per network, named like the reference's build does
 * (bnn/src/network/make-sw.sh:106-119):
 *     <runtime>-<network>-<platform>.so      e.g. python_sw-cnvW1A1-mi355x.so
 * It drops into bnn/libraries/<platform>/ and is dlopen'ed by the reference's
 * cffi shim (bnn/bnn.py:67-79,108-111) unchanged.
 *
 * PART 1 is exactly the reference's cdef (bnn/bnn.py:69-77); the functions
 * they replace are the extern "C" entry points of
 * bnn/src/network/<net>/sw/main_python.cpp.  PART 2 are extensions for
 * callers that already hold images in memory (host or HBM) and for multi-GPU
 * parameter broadcast; they use plain pointers and sizes only.
 *
 * Error behaviour: the reference throws C++ string literals across the ABI
 * (=> std::terminate).  This library never throws: it prints the same text to
 * stderr and returns NULL / -1 (a behavioural superset).
 * Thread-safety: like the reference, one classifier per loaded .so, calls must
 * not overlap (file-static weights: top.cpp:51-68, rawhls-offload.cpp:52).
 */
#ifndef BNN_MI355X_H
#define BNN_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ PART 1 */

/* Replaces load_parameters (cnvW1A1/sw/main_python.cpp:67-82,
 * lfcW1A1/sw/main_python.cpp:65-75): reads <path>/L-P-weights.bin and
 * L-P-thres.bin (format unchanged), repacks once, uploads to HBM. */
void load_parameters(const char *path);

/* Replaces inference (main_python.cpp:120-139 / lfc 113-133).  `path` is a
 * CIFAR-10 binary file (records of 1+3072 bytes) or an MNIST idx3 file; only
 * the first image is classified.  CNV: results (may be NULL) receives
 * number_class 16-bit scores, return = first maximum.  LFC: results receives a
 * 64-entry one-hot vector at round(log2(output word)), return = that index.
 * usecPerImage (may be NULL): device compute time, inputs resident in HBM. */
int inference(const char *path, int results[64], int number_class, float *usecPerImage);

/* Replaces inference_multiple (main_python.cpp:141-169 / lfc 135-156).
 * Returns a new int[n] of class indices (CNV: first strict maximum floored at
 * 0, foldedmv-offload.h:396-408; LFC: floor(log2(word)), foldedmv-offload.cpp:
 * 202-220) or, CNV with enable_detail != 0, a new int[n*number_class] of
 * scores.  No 10 000-image cap (the reference's INPUT_BUF_ENTRIES limit,
 * foldedmv-offload.h:56-58): the batch is chunked internally.
 * Free with free_results(). */
int *inference_multiple(const char *path, int number_class, int *image_number, float *usecPerImage,
                        int enable_detail);

/* Replaces inference_multiple_with_faults (main_python.cpp:171-223).
 * flip_count == 0: classifies like inference_multiple(enable_detail = 0).
 * flip_count > 0: flip_count faults (word_size adjacent bits of one weight or
 * threshold memory word; target < 0 any, 0 weights, > 0 thresholds; optional
 * list of target layers) at uniformly drawn image indices and memory positions,
 * selection weighted by memory size, addressed and applied exactly like
 * inject_fault / inject_fault_impl (foldedmv-offload.h:146-214).  Faults stay in
 * the loaded parameters until the next load_parameters.  The reference seeds
 * from std::random_device; see bnn_mi355x_set_fault_seed. */
int *inference_multiple_with_faults(const char *path, int number_class, int *image_number,
                                    float *usecPerImage, unsigned int flip_count, int word_size,
                                    int target, int *target_layers, unsigned int num_targets);

/* Replaces free_results (main_python.cpp:225-227). */
void free_results(int *result);

/* Replaces deinit (main_python.cpp:229-231, FoldedMVDeinit): frees the I/O
 * workspace; the loaded parameters stay, as in the reference. */
void deinit(void);

/* ------------------------------------------------------------------ PART 2 */

/* network compiled into this .so ("cnvW1A1", ...), and bytes per input image
 * (3072 planar CHW uint8 for cnv*, 784 for lfc*) */
const char *bnn_mi355x_network(void);
int bnn_mi355x_image_bytes(void);

/* last error text of this library ("" if none) */
const char *bnn_mi355x_last_error(void);

/* select the GPU (HIP ordinal) used by this library instance; call before
 * load_parameters.  Returns 0 on success.  Without the call the library binds to the calling thread's
 * current device at its first use.  Once bound, set_device(the bound ordinal) is a no-op returning 0 and any
 * other ordinal is an error (-1 + last_error). */
int bnn_mi355x_set_device(int ordinal);

/* Packed parameter blob (position-independent bytes, see csrc/packed_params.h).
 * pack: param directory -> blob, host only, touches no GPU (dst may be NULL to
 *       query the size); returns bytes or 0 on error.
 * export: the blob currently loaded; import: upload a blob obtained elsewhere,
 *       e.g. received through an RCCL broadcast from rank 0. */
size_t bnn_mi355x_pack_params(const char *path, void *dst, size_t cap);
size_t bnn_mi355x_export_params(void *dst, size_t cap);
int bnn_mi355x_import_params(const void *src, size_t bytes);
/* params_bytes: the size of this network's blob -- a function of the topology alone, so every rank of a
 *       multi-GPU job can allocate the receive buffer of the ONE broadcast without a size exchange.
 * import_params_device: like import_params, but the blob lies in HBM (e.g. the tensor RCCL broadcast into);
 *       d_src must be on this library's device, hip_stream is the stream that produced it (NULL = default).
 *       The header is validated on the host before anything uses it.
 * params_crc: CRC-32 of the parameter bytes the GPU holds (read back from HBM; 0 + last_error when nothing
 *       is loaded): lets the ranks of a job prove that they classify with identical parameters. */
size_t bnn_mi355x_params_bytes(void);
int bnn_mi355x_import_params_device(const void *d_src, size_t bytes, void *hip_stream);
unsigned int bnn_mi355x_params_crc(void);

/* Classify n images held in HOST memory (n x image_bytes, same byte layout as
 * the bodies of the file formats).  Same return convention and ownership as
 * inference_multiple. */
int *bnn_mi355x_inference_buffer(const uint8_t *images, int n_images, int number_class,
                                 float *usecPerImage, int enable_detail);

/* The LFC networks' input hand-over as the reference's host performs it (binarizeAndPack,
 * bnn/src/library/host/foldedmv-offload.cpp:82-98, called per image at :186-188): n images of 784 uint8 pixels ->
 * n x 13 little-endian 64-bit words, bit i = (pixel i >= 128), bits 784..831 zero.  This is what the entry points
 * that take HOST data (inference_multiple, inference_buffer, inference_raw) run on worker threads so that 104 bytes
 * per image cross the PCIe link instead of 784 (images already in HBM -- inference_device -- are binarised by the
 * kernels).  Host only, touches no GPU; LFC libraries only (-1 + last_error on a CNV library).  Returns 0. */
int bnn_mi355x_binarize_pack(const uint8_t *images, int n_images, uint64_t *words);

/* Raw outputs for n host images: CNV scores[n*64] (16-bit, all 64 neurons of
 * layer 8), LFC words[n] (raw 64-bit output word).  Either may be NULL.
 * Returns 0 on success. */
int bnn_mi355x_inference_raw(const uint8_t *images, int n_images, int16_t *scores, uint64_t *words,
                             float *usecPerImage);

/* Classify n images already resident in HBM, asynchronously on `hip_stream`
 * (a hipStream_t, NULL = the default stream).  d_classes: int32[n] (batched
 * decode); d_scores (CNV, optional): int16[n*64]; d_words (LFC, optional):
 * uint64[n].  All device pointers.  Alignment: d_images 16 bytes (every image then is: 3072 and 784 are
 * multiples of 16; the kernels read them with 128-bit loads), d_classes and d_scores 4 bytes, d_words 8 bytes;
 * a misaligned pointer is refused (-1 + last_error), nothing is launched.  The workspace grows on demand (which
 * synchronises); call bnn_mi355x_reserve first to keep the call fully
 * asynchronous / graph-capturable.  Returns 0 on success.
 * A pass of a CNV net of 16 384 images and more runs its second half on a stream of the library's own (second activation
 * workspace) and joins it into `hip_stream` before anything queued after the call can run: to the caller the call is still
 * one in-order piece of work on `hip_stream` (not while that stream is being captured, then everything stays on it).
 * The activation workspaces belong to the library instance: calls are serialised on the device -- a call on another
 * stream than the previous one first waits (hipStreamWaitEvent) for that call's kernels -- so they never
 * race, but they do not overlap either (a stream handed in here must stay alive until its work is done: the
 * previous call's stream is recognised by its handle).  While `hip_stream` is being captured into a graph the
 * hand-over from an earlier call on another stream is settled on the host (the call blocks until that call's
 * kernels are done) and nothing from outside the capture is recorded into it; a captured graph must not be
 * replayed concurrently with other calls into the same library.  The calling thread's current device is switched to this library's.
 * LFC with d_classes: number_class <= 47 (the device decode is an exact floor(log2); the reference's
 * (unsigned) log2((double) word) differs from it for some words of 48 and more bits, which only the host
 * decode of inference_multiple / inference_buffer reproduces); take d_words beyond that. */
int bnn_mi355x_inference_device(const void *d_images, int n_images, int number_class, int32_t *d_classes,
                                int16_t *d_scores, uint64_t *d_words, void *hip_stream);
int bnn_mi355x_reserve(int max_images);

/* How the entry points that take HOST data (inference_multiple, inference_buffer, inference_raw) move it:
 *  - a single CIFAR image from a file, up to 32 from a host buffer, or up to 1 024 MNIST images: no transfer at all -- the image (LFC: binarised by the calling thread)
 *    is placed in pinned memory the GPU addresses, the one-launch kernels read it over the link and write their results into
 *    pinned memory; one launch, one wait.
 *  - the LFC networks otherwise: worker threads binarise (bnn_mi355x_binarize_pack) into pinned memory, 104 bytes per image
 *    cross the link; chunks of 8 192 images first, doubling up to 32 768.
 *  - the CNV networks otherwise: chunks whose transfer overlaps the previous chunks' stages: 512 images first (the first
 *    transfer is what nothing overlaps), doubling up to 4 096, then growing by half up to 16 384; a call of 8 192 ... 32 767
 *    images ramps down again at its end (512 last).  A file is read by worker threads straight into a ring of pinned pieces, the label
 *    byte of every record dropped on the way (preadv); a host buffer goes through the runtime's pageable path, its copies
 *    issued by a helper thread while the calling thread enqueues stages.
 * A call of three or more chunks runs them alternately on two internal streams ("compute lanes"), each with its own activation
 * workspace; usecPerImage is then the union of the chunks' device intervals over the images.  Results of calls up to 32 768
 * images are written by the last stage into pinned memory, larger ones come back in one transfer at the end.
 * chunk_plan writes the chunk boundaries base[0] = 0 < base[1] < ... < base[k] = n (at most cap of them) and returns k + 1
 * (from_file is accepted for compatibility: both entry points use the same plan since round 4).  Host only; results never
 * depend on the plan (tests/test_gpu_parity.py and tests/test_gpu_host_paths.py walk its edges). */
int bnn_mi355x_chunk_plan(int n_images, int from_file, int *bases, int cap);

/* Which stages of a CNV network one pass of n_images images runs on the matrix cores, with the parameters and switches
 * (BNN_MI355X_CONV, BNN_MI355X_CONV_MFMA_MIN, BNN_MI355X_TAIL_MFMA_MIN, BNN_MI355X_L0, BNN_MI355X_L1) now in force: bit k
 * set = layer k runs as an MFMA kernel (layer 0's int8 forms; layers 1-3 and, from an edge of their own, layers 4-7 as FP4
 * GEMMs), clear = on the integer pipe.  Bit 8 is never set: layer 8 has no matrix form.  The results never tell -- both
 * paths are bit-identical -- so this is how a caller or a test sees which one a size takes.  A pass is what
 * bnn_mi355x_inference_device enqueues on one stream; calls the runtime splits (the chunks of chunk_plan, the two halves of a
 * device call of 16 384 images and more) decide per piece: ask with the piece's size.  The answer is for a pass without a
 * completion word: the host-timed single-image call (BNN_MI355X_DIRECT_TIMING=host) keeps layers 4-8 in one launch on the
 * integer pipe.  The fault-injection entry points always run layers 1-7 on the integer pipe (all but
 * bnn_mi355x_input_noise_campaigns, which classifies its faulted images by this very pass).  0 for the LFC networks, -1
 * before load_parameters.  Host only. */
int bnn_mi355x_matrix_stages(int n_images);

/* Fault campaigns: fix the seed of the fault planner (0 = std::random_device like the
 * reference, the default) and read back the faults of the last
 * inference_multiple_with_faults call as records of 8 ints
 * {image, target (0 weights / 1 thresholds), layer, mem (PE), ind, thresh, bit, word_size};
 * returns the number of faults. */
int bnn_mi355x_set_fault_seed(unsigned long long seed);
int bnn_mi355x_last_faults(int *records, int cap_records);
/* Many campaigns in one call, side by side on the GPU: num_runs independent campaigns over the images of
 * `path`, run r exactly what load_parameters(<current>) + bnn_mi355x_set_fault_seed(seed + r) +
 * inference_multiple_with_faults(...) returns.  Returns a new int[num_runs * n], run-major (free_results).
 * seed == 0: each run seeds from std::random_device; else run r uses seed + r (refused if any seed + r is
 * 0 mod 2^64).  Every run starts from the parameters loaded at the time of the call, faults of earlier calls
 * included; the loaded parameters are NOT changed.  usecPerImage: device time of the whole call / (num_runs * n).
 * Refuses (NULL + last_error) what inference_multiple_with_faults refuses -- the hardened variants, an imported
 * blob, the BNN_MI355X_L1 comparison forms -- and num_runs outside 1 ... 4096.  flip_count == 0: the fault-free
 * classes, once per run.  HBM: num_runs x bnn_mi355x_params_bytes() for the runs' parameter copies.
 * The runs go in waves: in wave k every run classifies the images between its k-th and (k+1)-th fault time, all
 * runs in the same launches.
 * last_campaign_faults: the faults of the last fault_campaigns call as records of 9 ints {run, image, target,
 * layer, mem, ind, thresh, bit, word_size}, run-major, each run in the order bnn_mi355x_last_faults would list
 * it; returns the count. */
int *bnn_mi355x_fault_campaigns(const char *path, int number_class, int num_runs, unsigned long long seed,
                                unsigned int flip_count, int word_size, int target, const int *target_layers,
                                unsigned int num_targets, int *image_number, float *usecPerImage);
int bnn_mi355x_last_campaign_faults(int *records, int cap_records);
/* Host-only helpers of the same machinery (no GPU touched): draw a fault plan; pack a parameter
 * directory with a list of fault records applied (what the GPU holds after those faults). */
int bnn_mi355x_plan_faults(unsigned long long seed, int num_images, unsigned int flip_count, int word_size, int target,
                           const int *target_layers, unsigned int num_targets, int *records, int cap_records);
size_t bnn_mi355x_pack_params_faulty(const char *path, const int *records, int n_faults, void *dst, size_t cap);
/* Exhaustive single-fault sweeps: which bits matter.
 * enumerate_faults: every distinct fault of one layer -- target 0 weights / 1 thresholds, word_size 1..64.
 * "Distinct" = the positions plan_faults can draw, with bit aligned down to a multiple of word_size the way
 * apply_fault does (so no two records have the same effect), ordered by (mem, ind, thresh, bit).  Writes records
 * [first, first + cap_records) in the 8-int format of bnn_mi355x_plan_faults (image = 0); returns the total count
 * (records may be NULL; 0 for the thresholds of a layer without any), -1 + last_error on a bad layer / target /
 * word_size.  Host only.
 * fault_sweep: for each of the n_faults records (8 ints; the image field is ignored: the fault is present for every
 * image) classify every image of `path` with the loaded parameters plus that one fault, independently of the other
 * records.  changed[f] = images whose class differs from the fault-free class.  diffs (optional): triples {fault,
 * image, class} of every changed image in (fault, image) order, at most cap_diffs of them.  Returns the total number
 * of changed (fault, image) pairs (which may exceed cap_diffs), or -1 + last_error.  The loaded parameters,
 * last_faults and last_campaign_faults are unchanged.  Refuses what bnn_mi355x_fault_campaigns refuses (hardened
 * variants, an imported blob, the BNN_MI355X_L1 forms) and records outside their layer's memories, before anything
 * runs on the device.  usecPerImage: device time / (n_faults * n).
 * The fault-free pass runs once and keeps every layer's output; a fault in layer L starts from the fault-free output
 * of layer L-1, and after every layer a (fault, image) pair whose activations equal the fault-free ones is dropped:
 * it keeps the fault-free class.
 * last_sweep_stages: of the last sweep, per layer s the number of (fault, image) pairs layer s has to run: all pairs
 * of the faults in layer s, and those of faults in earlier layers whose activations still differ from the fault-free
 * ones there (the stage runs a few more where cutting a record short would cost more); returns the number of layers
 * (0 before the first sweep). */
long bnn_mi355x_enumerate_faults(int layer, int target, int word_size, long first, int *records, int cap_records);
long bnn_mi355x_fault_sweep(const char *path, int number_class, const int *records, int n_faults, int *changed, int *diffs,
                            long cap_diffs, int *image_number, float *usecPerImage);
int bnn_mi355x_last_sweep_stages(long *pairs_per_stage, int cap);
/* Activation-fault sweeps: which datapath bits matter (a soft error in the stream between two layers, one image).
 * A site is one activation of layer L's output as layer L+1 reads it (CNV layers 1 and 3: after the max-pool), L any
 * layer but the last; records are 5 ints {layer, y, x, channel, shift} in the value domain and HWC order of the
 * oracle's layer_ref (FC layers: y = x = 0, channel = the neuron).  The fault replaces the activation's level index
 * i (1-bit: -1, +1; 2-bit: -1, 0, +1) by (i + shift) mod levels, 1 <= shift < levels: it changes the activation of
 * every image.  This model is the project's own (the reference has none).
 * enumerate_act_faults: every site x shift of layer L ordered by (y, x, channel, shift); writes records
 * [first, first + cap_records) and returns the total (records may be NULL); -1 + last_error for the last layer or a
 * layer out of range.  Host only.
 * act_fault_sweep: for each record, classify every image of `path` with that one activation changed while that image
 * is classified, independently of the other records; changed / diffs / return value / usecPerImage as fault_sweep.
 * The loaded parameters and last_faults / last_campaign_faults / last_sweep_stages are unchanged.  Every record is
 * validated on the host before anything runs on the device.  Refused (-1 + last_error): bad arguments; a record
 * whose layer has no sites (the last one, out of range) or whose site or shift lies outside it (the message names
 * the record); the hardened variants ("not modelled", as every fault entry point); the BNN_MI355X_L1 comparison
 * forms.  An imported blob is fine: activation faults patch no parameter.
 * The fault-free pass runs once and keeps every layer's output; a site in layer L starts at layer L+1 from that
 * output with the site changed, and pairs whose activations return to the fault-free ones are dropped as in
 * fault_sweep.  CNV sites of layers 0, 1 and 2: layer L+1 -- a 3x3 convolution over a map wider than what one changed
 * activation reaches -- is evaluated only inside that window (at most 3x3 conv outputs; behind a max-pool the up to
 * 2x2 pool quads they fall into), over the fault-free layer-(L+1) output; the results are the dense route's bit for bit.
 * Two switches, read at every call: BNN_MI355X_ACT_WINDOW=0 evaluates layer L+1 whole for every site layer, any other
 * value takes the window for every CNV site layer 0..2 (the A/B switch); unset, a (net, site layer) case runs windowed
 * only where that was measured faster than the dense route -- so far none, the default is the dense route.
 * BNN_MI355X_SWEEP_GROUP=<pairs> caps the (site, image) pairs of a run group (tests: several groups and image windows
 * on a few dozen images).  Under BNN_MI355X_TRACE every group prints a second line, "act_fault_sweep window:",
 * with its layer, the pairs whose first stage ran windowed and the output pixels recomputed per pair.
 * last_act_sweep_stages: of the last activation sweep, per layer the (fault, image) pairs it had to run (0 up to
 * layer L of the earliest site); returns the number of layers (0 before the first such sweep). */
long bnn_mi355x_enumerate_act_faults(int layer, long first, int *records, int cap_records);
long bnn_mi355x_act_fault_sweep(const char *path, int number_class, const int *records, int n_faults, int *changed, int *diffs,
                                long cap_diffs, int *image_number, float *usecPerImage);
int bnn_mi355x_last_act_sweep_stages(long *pairs_per_stage, int cap);

/* Datapath upset-rate campaigns: the accuracy when EVERY activation of the stream is upset with probability p.  The
 * random, many-at-once form of the activation-fault model above (sites, their order and `shift` as
 * bnn_mi355x_enumerate_act_faults lists them; the project's own model).  rate_q32[L], L = 0 ... layers - 2:
 * the rate of layer L's output in units of 2^-32 (0: never).  For run seed k, image i (its index in the file), layer L
 * and site s (counting y, x, channel):
 *     u = philox4x32_10(counter {i, L, s >> 2, 0}, key {k & 0xffffffff, k >> 32})[s & 3]
 * with the constants of the Philox paper; the site is upset iff u < rate_q32[L], with shift 1 + (u & 1) for 2-bit
 * activations and 1 for 1-bit ones.  All upsets of layer L's output are applied together, to the map actually flowing
 * in that (run, image) pair -- already disturbed by the upsets of earlier layers -- before layer L + 1 reads it.  The
 * draw keys on the image's index in the file and on nothing else of the call: results do not depend on batch size,
 * grouping of runs or chunking.
 * act_noise_campaigns: num_runs (1 ... 4096) independent runs over the images of `path`, run r with seed + r (refused
 * if that is 0 mod 2^64 for a run; seed == 0: every run's seed from std::random_device, read them back with
 * last_act_noise_seeds).  Returns a new int[num_runs * n] of classes, run-major (free_results).  n_rates must be
 * layers - 1.  All rates 0: the fault-free classes once per run.  The loaded parameters, last_faults,
 * last_campaign_faults and both last_*sweep_stages are unchanged.  Refused (NULL + last_error) before any device work:
 * bad arguments, the hardened variants ("not modelled", as every fault entry point), the BNN_MI355X_L1 comparison
 * forms.  An imported blob is fine: no parameter is patched.  usecPerImage: device time / (num_runs * n).  Every pair
 * runs every layer on the integer-pipe kernels of the fault paths; groups of pairs are bounded by the activation
 * workspace (BNN_MI355X_NOISE_GROUP=<pairs> makes them smaller: tests).
 * last_act_noise_counts: of the last such call, the sites actually upset per [run][layer], run-major, counted on the
 * device by the kernel that applies them; returns runs * (layers - 1) (0 before the first call).
 * last_act_noise_seeds: the runs' seeds of the last call; returns their number.
 * act_noise_mask: host only, touches no GPU.  The upset sites of one (run seed, image, layer) at `rate_q32` as 5-int
 * act_fault_sweep records in site order: writes records [first, first + cap_records) and returns the total (records
 * may be NULL); -1 + last_error for a layer without sites or a negative image / first. */
int *bnn_mi355x_act_noise_campaigns(const char *path, int number_class, int num_runs, unsigned long long seed,
                                    const unsigned int *rate_q32, int n_rates, int *image_number, float *usecPerImage);
int bnn_mi355x_last_act_noise_counts(long *upsets, int cap);
int bnn_mi355x_last_act_noise_seeds(unsigned long long *seeds, int cap);
long bnn_mi355x_act_noise_mask(unsigned long long run_seed, int image, int layer, unsigned int rate_q32, long first,
                               int *records, int cap_records);

/* Input-buffer faults: which pixel bits matter, and the accuracy at input-buffer upset rate p (on the FPGA the DRAM / AXI
 * input buffer; here HBM or pinned memory).  A site is one bit of one input byte, the bytes in the layout of
 * bnn_mi355x_inference_buffer: bnn_mi355x_image_bytes() per image (CNV 3072, planar CHW; LFC 784, row-major); the label
 * byte of a CIFAR record and the idx header are not sites.  Site number s = byte * 8 + bit, bit 0 the LSB: image_bytes * 8
 * sites per image.  A fault XORs that bit while that image is classified -- a faulted image is just another image, so
 * every result below equals what bnn_mi355x_inference_buffer returns for the bytes with those bits flipped on the host.
 * The model is the project's own (the reference has no input injection).  Records are 2 ints {byte, bit}.
 * enumerate_input_faults: every site in site order; writes records [first, first + cap_records) and returns the total
 * (records may be NULL); -1 + last_error for a negative first.  Host only.
 * input_fault_sweep: for each record, classify every image of `path` with that one bit flipped while that image is
 * classified, independently of the other records; changed / diffs / return value / usecPerImage as act_fault_sweep.
 * The loaded parameters and every other last_* state are unchanged.  Every record is validated on the host before
 * anything runs on the device.  Refused (-1 + last_error): bad arguments; a record whose byte or bit lies outside the
 * image (the message names the record); the hardened variants ("not modelled", as every fault entry point); the
 * BNN_MI355X_L1 comparison forms.  An imported blob is fine: no parameter is patched.
 * The fault-free pass runs once and keeps every layer's output; a group's pairs start at layer 0 (LFC: at the binariser)
 * from faulted copies of their images, and pairs whose activations equal the fault-free ones after a layer are dropped as
 * in fault_sweep (an LFC bit 0 ... 6 never survives the binariser's layer: it reads bit 7 only).
 * BNN_MI355X_SWEEP_GROUP=<pairs> caps the (site, image) pairs of a run group as for act_fault_sweep.
 * last_input_sweep_stages: of the last input sweep, per layer the (fault, image) pairs it had to run; returns the number
 * of layers (0 before the first such sweep).
 * Random form.  For run seed k, image i (its index in the file) and site s:
 *     u = philox4x32_10(counter {i, 0xffffffff, s >> 2, 0}, key {k & 0xffffffff, k >> 32})[s & 3]
 * and the bit is flipped iff u < rate_q32 (units of 2^-32).  The second counter word is where act_noise_campaigns puts the
 * layer; no layer has that tag, so the two draws never share a stream.  Results are a function of (seed, run, image index,
 * site) alone: not of batch size, grouping, chunking or the kernel path that runs the network.
 * input_noise_campaigns: num_runs (1 ... 4096) independent runs over the images of `path`, run r with seed + r (refused if
 * that is 0 mod 2^64 for a run; seed == 0: every run's seed from std::random_device, read them back with
 * last_input_noise_seeds).  Returns a new int[num_runs * n] of classes, run-major (free_results).  rate_q32 == 0: the
 * fault-free classes once per run, no upset kernel is launched.  Refused (NULL + last_error) before any device work: bad
 * arguments, the hardened variants ("not modelled"), the BNN_MI355X_L1 comparison forms.  An imported blob is fine.
 * usecPerImage: device time / (num_runs * n).  The (run, image) pairs go in groups of faulted images in a staging buffer
 * (131 072 pairs; BNN_MI355X_NOISE_GROUP=<pairs> makes them smaller: tests), and a group is classified with the loaded,
 * unpatched parameters by the pass bnn_mi355x_inference_device takes for that many images, matrix-core stages included.
 * last_input_noise_counts: of the last such call, the bits actually flipped per run, counted on the device by the kernel
 * that flips them; returns the number of runs (0 before the first call).
 * last_input_noise_seeds: the runs' seeds of the last call; returns their number.
 * input_noise_mask: host only, touches no GPU.  The flipped sites of one (run seed, image) at `rate_q32` as 2-int sweep
 * records in site order: writes records [first, first + cap_records) and returns the total (records may be NULL);
 * -1 + last_error for a negative image / first. */
long bnn_mi355x_enumerate_input_faults(long first, int *records, int cap_records);
long bnn_mi355x_input_fault_sweep(const char *path, int number_class, const int *records, int n_faults, int *changed, int *diffs,
                                  long cap_diffs, int *image_number, float *usecPerImage);
int bnn_mi355x_last_input_sweep_stages(long *pairs_per_stage, int cap);
int *bnn_mi355x_input_noise_campaigns(const char *path, int number_class, int num_runs, unsigned long long seed,
                                      unsigned int rate_q32, int *image_number, float *usecPerImage);
int bnn_mi355x_last_input_noise_counts(long *upsets, int cap);
int bnn_mi355x_last_input_noise_seeds(unsigned long long *seeds, int cap);
long bnn_mi355x_input_noise_mask(unsigned long long run_seed, int image, unsigned int rate_q32, long first, int *records,
                                 int cap_records);

/* Memory upset-rate campaigns: the accuracy when EVERY bit of the weight / threshold memories is upset with probability
 * p (cross-section x fluence), independently per bit -- the random, many-at-once form of the parameter faults of
 * bnn_mi355x_fault_sweep.  The sites of layer L and target (0 weights, 1 thresholds) are the records
 * bnn_mi355x_enumerate_faults(L, target, word_size 1, ...) lists; site s is a record's index in that list:
 *     weights     s = (mem * WMEM + ind) * (SIMD * wbits) + bit
 *     thresholds  s = ((mem * TMEM + ind) * nthr + thresh) * ebits + bit        (ebits 24 for layer 0 of the CNV nets, else 16)
 * (pad bits of the 64-bit file words are no sites; pad columns inside a memory word's SIMD bits are).  For run seed k
 *     u = philox4x32_10(counter {L, target, s >> 2, 1}, key {k & 0xffffffff, k >> 32})[s & 3]
 * and the site is flipped iff u < rate (units of 2^-32: rate_w_q32[L], rate_t_q32[L], one entry per layer).  The
 * activation and input draws have 0 in the fourth counter word: the three models never share a stream.  The parameters
 * of a run are what bnn_mi355x_pack_params_faulty builds from the loaded parameters with every flipped site applied as a
 * word_size-1 record, layer-major, per layer weights then thresholds, in site order; they are in place from the first
 * image to the last (the memory state after the exposure; upsets that arrive while the run goes on: the exposure
 * campaigns below).  Results depend on (seed, run, rates) and the loaded
 * parameters alone, not on batch size, grouping or chunking.  The reference has no rate-based injection: parity is
 * unpinned, the mechanism of a single flip is the pinned one.
 * mem_noise_campaigns: num_runs (1 ... 4096) independent runs over the images of `path`, run r with seed + r (refused if
 * that is 0 mod 2^64 for a run; seed == 0: every run's seed from std::random_device, read them back with
 * last_mem_noise_seeds).  Returns a new int[num_runs * n] of classes, run-major (free_results).  n_rates must be the
 * number of layers; a non-zero threshold rate for a layer without threshold memory is refused.  All rates 0: the
 * fault-free classes once per run, no upset kernel is launched.  The loaded parameters, params_crc, last_faults,
 * last_campaign_faults and every last_*sweep* state are unchanged.  Refused (NULL + last_error) before any device work:
 * bad arguments, the hardened variants ("not modelled"), an imported blob (no raw memories), the BNN_MI355X_L1
 * comparison forms.  usecPerImage: device time / (num_runs * n).  Every run has its own copy of the blob in HBM; the
 * upsets are drawn and applied there by the GPU (layer 0 of the CNV nets by the host), and the (run, image) pairs run the
 * integer-pipe kernels of the fault paths in groups bounded by the activation workspace (BNN_MI355X_NOISE_GROUP=<pairs>
 * makes them smaller: tests).
 * last_mem_noise_counts: of the last such call, the flips actually applied per [run][layer][2: weights, thresholds],
 * counted by the code that applies them; returns runs * layers * 2 (0 before the first call).
 * last_mem_noise_seeds: the runs' seeds of the last call; returns their number.
 * mem_noise_mask: host only, touches no GPU.  The flipped sites of one (run seed, layer, target) at `rate_q32` as 8-int
 * fault records (image 0, word_size 1) in site order: writes records [first, first + cap_records) and returns the total
 * (records may be NULL); 0 for the thresholds of a layer without any; -1 + last_error for a bad layer or target or a
 * negative first.
 * mem_noise_params: the packed blob a run with this seed classifies with, made on the device by the kernels and patches
 * the campaign uses (one copy) and read back: import it elsewhere, diff it.  dst NULL queries the size.  0 + last_error
 * for what the campaign refuses, or a destination too small. */
int *bnn_mi355x_mem_noise_campaigns(const char *path, int number_class, int num_runs, unsigned long long seed,
                                    const unsigned int *rate_w_q32, const unsigned int *rate_t_q32, int n_rates,
                                    int *image_number, float *usecPerImage);
int bnn_mi355x_last_mem_noise_counts(long *flips, int cap);
int bnn_mi355x_last_mem_noise_seeds(unsigned long long *seeds, int cap);
long bnn_mi355x_mem_noise_mask(unsigned long long run_seed, int layer, int target, unsigned int rate_q32, long first,
                               int *records, int cap_records);
size_t bnn_mi355x_mem_noise_params(unsigned long long run_seed, const unsigned int *rate_w_q32,
                                   const unsigned int *rate_t_q32, int n_rates, void *dst, size_t cap);

/* Hardened memory schemes in the memory upset campaigns: what TMR or threshold interleaving buys at an upset rate.  The
 * entry points above keep their meaning (and the variant libraries their refusals); these take the scheme as an argument
 * and are the same code in every library: 0 none, 1 TMR, 2 interleaved, 3 resilient-interleaved.
 * The storage side is the reference's, restated from its host code (csrc/mem_org.h has the tables and the formula):
 *   TMR          three modules for the weight memory of layer 0 and the threshold memories of layers 0-4, else one;
 *   interleaved  (2, 3) the threshold memory of every layer that has one: lines ind (even) and ind + 1 of a PE are stored
 *                as one bit-interleaved pair, by the default pattern (2) or the resilient variants' pattern with the
 *                second element reversed (3); weights are not interleaved; an odd last line is stored as is.
 * Supported: cnvW1A1 and cnvW1A2 with 1, 2, 3; cnvW2A2 with 1 and 3; scheme 0 everywhere.  Refused with the reason in
 * last_error: cnvW2A2 with scheme 2 (the reference interleaves its 64-bit weight elements with a 64-bit pattern for 128
 * positions and reads past the second element: no defined layout) and every LFC library with a scheme other than 0 (the
 * one LFC overlay interleaves 24-bit elements into 16-bit words; its hardware is not in the reference).
 * The PHYSICAL state is what the loader hands the memories: interleaved words, one copy per module.  A physical fault
 * record is 9 ints {image, target, layer, mem, ind, thresh, bit, word_size, module}: inject_fault's read-modify-write on
 * that module's physical word (the layer-0 integer-part quirk included, as is).  The parameters the network computes with
 * are de-interleave(vote(modules)).  The de-interleaver is the inverse permutation (forced: a fault-free hardened overlay
 * computes the base network).  The voter is THE PROJECT'S OWN choice, the reference's being in a fork that is not in its
 * tree: the bitwise majority of the low `ebits` of the three stored words.  Any voter agrees with it while at most one
 * module of a word is hit; where two are hit voters could differ, and such results are this model's alone.
 * The upset model: per-layer rates as above plus a burst width b (1 ... 16).  An event flips b adjacent physical bits of
 * one element of one module: the aligned group g of enumerate_faults(L, target, word_size b), per = ceil(ebits / b)
 * groups per element, the last one clipped to the element.  With e = element * per + g (element as above) and module m
 *     u = philox4x32_10(counter {L, target | m << 1 | (b - 1) << 8, e >> 2, 1}, key {k & 0xffffffff, k >> 32})[e & 3]
 * and the event happens iff u < rate.  m = 0, b = 1 is mem_noise_mask's draw: scheme 0 with burst 1 reproduces
 * mem_noise_campaigns bit for bit.  Events apply layer-major, weights then thresholds, module-major, in event order.
 * hardening_scheme: the scheme this library's name implies (0 for a base network).  Host only.
 * hardening_layout: out = {weight modules, threshold modules, threshold interleave 0 / 2 / 3} of a layer; -1 + last_error
 * for a refused (network, scheme) pair or a bad layer.  Host only.
 * hardened_site: logical -> physical: bit `bit` of line `ind` (of one PE) of the layer's weight (0) or threshold (1)
 * memory is stored in line *p_ind at bit *p_bit.  -1 + last_error for a refused pair or a position outside.  Host only.
 * hardened_mem_noise_mask: the events of one (run seed, layer, target, module) as 9-int physical records (image 0,
 * word_size b, bit = g * b), paged like mem_noise_mask; -1 + last_error for a bad argument.  Host only.
 * pack_params_hardened: the blob after n physical faults applied in the order given (dst NULL queries the size); scheme 0
 * with module 0 is pack_params_faulty.  Host only.
 * hardened_mem_noise_campaigns: mem_noise_campaigns with (scheme, burst): its conventions, refusals (but the variants':
 * the scheme is the argument), grouping and BNN_MI355X_NOISE_GROUP; also refused: burst outside 1 ... 16, a bad scheme or
 * refused pair.  Runs the exposure campaigns' device path (k_xmem_noise_w / k_xmem_noise_t at epoch 0 on zeroed state;
 * layer 0 of the CNV nets on the host through the physical model), scheme 0 included: exposure_campaigns with the whole
 * file as one epoch.  All rates 0: the fault-free classes, no upset kernel is launched.
 * hardened_mem_noise_params: the blob one run classifies with, made by that path and read back.
 * last_hardened_mem_noise_counts: per [run][layer][2: weights, thresholds] two longs: the physical bits flipped (before
 * voting) and the logical bits that differ (after voting and de-interleaving); returns runs * layers * 4.
 * last_hardened_mem_noise_seeds: the runs' seeds of the last such call. */
int bnn_mi355x_hardening_scheme(void);
int bnn_mi355x_hardening_layout(int scheme, int layer, int out[3]);
int bnn_mi355x_hardened_site(int scheme, int layer, int target, int ind, int bit, int *p_ind, int *p_bit);
long bnn_mi355x_hardened_mem_noise_mask(int scheme, int burst, unsigned long long run_seed, int layer, int target, int module,
                                        unsigned int rate_q32, long first, int *records, int cap_records);
size_t bnn_mi355x_pack_params_hardened(const char *path, int scheme, const int *records, int n_faults, void *dst, size_t cap);
int *bnn_mi355x_hardened_mem_noise_campaigns(const char *path, int number_class, int scheme, int burst, int num_runs,
                                             unsigned long long seed, const unsigned int *rate_w_q32,
                                             const unsigned int *rate_t_q32, int n_rates, int *image_number,
                                             float *usecPerImage);
size_t bnn_mi355x_hardened_mem_noise_params(int scheme, int burst, unsigned long long run_seed, const unsigned int *rate_w_q32,
                                            const unsigned int *rate_t_q32, int n_rates, void *dst, size_t cap);
int bnn_mi355x_last_hardened_mem_noise_counts(long *counts, int cap);
int bnn_mi355x_last_hardened_mem_noise_seeds(unsigned long long *seeds, int cap);

/* Exposure campaigns: memory upsets that ACCUMULATE while a run goes on, with scrubbing -- how often must the memories
 * be rewritten?  The campaigns above put every upset in place before the first image; here the physical state of the
 * hardened model (scheme, burst, modules, interleave, voter: all as above) lives on the device between steps.
 * Epochs: a run over n images is cut into epochs of `epoch_images` images; epoch t holds images [t * epoch_images,
 * min(n, (t + 1) * epoch_images)), the last one may be short, E = ceil(n / epoch_images).  E is at most 65 536, and
 * num_runs * E * layers * 4 must stay below 2^31 (the counters' index): refused beyond.
 * Rates are PER EPOCH: rate_w_q32[L], rate_t_q32[L] in units of 2^-32, the probability of an event in one epoch.
 * Draw: the events of epoch t are the hardened campaign's with the epoch in the fourth counter word,
 *     u = philox4x32_10(counter {L, target | m << 1 | (b - 1) << 8, e >> 2, 1 + (t << 8)}, key {k & 0xffffffff, k >> 32})[e & 3]
 * and the event happens iff u < rate.  t = 0 is exactly hardened_mem_noise_mask's draw; the activation and input draws
 * have 0 in that word, so the low byte 1 keeps the streams apart.
 * Order: an epoch's upsets apply to the PHYSICAL state before the epoch's images are classified, XORed onto whatever the
 * state holds; inside an epoch layer-major, weights then thresholds, module-major, in event order; across epochs
 * epoch-major (the order matters only for the layer-0 integer-part quirk, kept as is).
 * Scrubbing: scrub_every = S.  0: never.  S > 0: before the upsets of every epoch t > 0 with t % S == 0 all physical
 * memories return to the loaded parameters -- a full rewrite; the voter-driven repair scrub: repair_exposure_campaigns.
 * The logical parameters of an epoch are de-interleave(vote(modules)) of the physical state.  On the host: the blob of
 * (run k, epoch t) is pack_params_hardened(dir, scheme, records), the records being the concatenation over epochs
 * t' = (last scrub epoch <= t) ... t of exposure_mask's records of that epoch, each in the in-epoch order above.
 * The voter, the epoch granularity and the full-rewrite scrub are the project's own choices (the reference injects at
 * image times into unhardened memories and has no scrub): parity unpinned.
 * exposure_mask: host only.  hardened_mem_noise_mask for one epoch (0 ... 65 535): the same 9-int physical records and
 * paging, the record's image field holding the epoch; with epoch 0 every other field equals that function's.
 * exposure_campaigns: returns int[num_runs * n], run-major (free_results); image j is classified with the state of epoch
 * j / epoch_images.  Seeds, num_runs limits, usecPerImage, grouping (BNN_MI355X_NOISE_GROUP, inside an epoch) and what
 * stays untouched (the loaded parameters, params_crc, the last_* state of every other entry point) follow
 * hardened_mem_noise_campaigns, and so do the refusals: the same (network, scheme) pairs, an imported blob, the
 * BNN_MI355X_L1 comparison forms, burst outside 1 ... 16; also epoch_images < 1, scrub_every < 0 and E beyond the cap.
 * All before any device work, NULL + last_error.  All rates 0: the fault-free classes, no upset kernel or copy is
 * launched.  With epoch_images >= n the call computes hardened_mem_noise_campaigns' classes and counts.
 * exposure_params: the blob run `run_seed` classifies epoch `epoch` with, made on the device by the campaign's own
 * kernels and scrub steps -- one copy stepped through epochs 0 ... epoch -- and read back.  dst NULL queries the size;
 * 0 + last_error for what the campaign refuses, an epoch outside 0 ... 65 535 or a destination too small.
 * last_exposure_counts: per [run][epoch][layer][2: weights, thresholds] two longs: the physical bits flipped IN that
 * epoch, and the logical bits that differ from the loaded parameters AFTER that epoch's upsets; returns runs * E *
 * layers * 4.
 * last_exposure_seeds: the runs' seeds of the last such call. */
long bnn_mi355x_exposure_mask(int scheme, int burst, unsigned long long run_seed, int epoch, int layer, int target,
                              int module, unsigned int rate_q32, long first, int *records, int cap_records);
int *bnn_mi355x_exposure_campaigns(const char *path, int number_class, int scheme, int burst, int num_runs,
                                   unsigned long long seed, const unsigned int *rate_w_q32, const unsigned int *rate_t_q32,
                                   int n_rates, int epoch_images, int scrub_every, int *image_number, float *usecPerImage);
size_t bnn_mi355x_exposure_params(int scheme, int burst, unsigned long long run_seed, const unsigned int *rate_w_q32,
                                  const unsigned int *rate_t_q32, int n_rates, int epoch, int scrub_every, void *dst,
                                  size_t cap);
int bnn_mi355x_last_exposure_counts(long *counts, int cap);
int bnn_mi355x_last_exposure_seeds(unsigned long long *seeds, int cap);

/* Coded threshold memories in the exposure campaigns: a single-error-correcting, double-error-detecting code as an axis
 * orthogonal to the scheme.  The code is the PROJECT'S OWN MODEL (the fork has none; parity unpinned, like the voter and
 * the activation faults): Hamming(21,16) plus an overall parity bit, which is what block RAM ECC is.
 * code: 0 none (every function below is then the exposure function of the same name), 1 SEC-DED.
 * The code: a coded element is a 16-bit threshold word with 6 check bits.  Code word positions are 1 ... 21; positions 1,
 * 2, 4, 8, 16 hold check bits c0 ... c4, the other positions in increasing order (3, 5, 6, 7, 9 ... 15, 17 ... 21) data
 * bits 0 ... 15.  c_j = the XOR of the data bits whose position has bit j set; c5 = the XOR of all 16 data bits and
 * c0 ... c4.  encode(0x0001) = 0x23, encode(0x8000) = 0x15, encode(0xFFFF) = 0x1E, encode(0x1234) = 0x19.
 * Decode (stored data d, stored check c): s = (encode(d) ^ c) & 31, P = parity(d) ^ parity(c).  s = 0 and P = 0: status
 * 0, data d.  P = 1 and s = 0 or a power of two: status 1 (corrected: a check bit was hit), data d.  P = 1 and s a data
 * position: status 1, d with that data bit flipped.  P = 1 and s = 22 ... 31, or P = 0 and s != 0: status 2 (detected,
 * uncorrectable), data d as stored.  Every single error of the 22 bits is restored, none of the 231 doubles is
 * miscorrected, of the 1 540 triples 1 052 are accepted as a correction (the data then wrong) and 488 detected.
 * Which memories: code 1 covers the 16-bit threshold memory of every layer that has one.  TWO LIMITS: weights are not
 * coded (their memory words are SIMD * wbits = 1 ... 32 bits wide: no per-word code makes sense over them; the
 * interleaved schemes leave them alone as well), and the 24-bit threshold memory of CNV layer 0 is not coded (a fault
 * there passes through the reference's integer-part read-back, which rewrites the whole word: no code word survives
 * that).  Layer 0 keeps the uncoded host route; a study that wants it out of the picture sets its rates to 0.
 * Storage: the check bits of an element live in a check memory of their own, of the same (PE, line, threshold) shape, 6
 * bits wide, addressed as MODULE 1 of target 1.  Scheme 0 stores element and check word as they are.  Scheme 2 encodes
 * the logical element, interleaves the data of lines ind, ind + 1 as without a code, and their check words by the same
 * construction at width 6 (pattern 0x555: line ind holds positions 6 ... 11, line ind + 1 positions 0 ... 5); an odd last
 * line is stored as is.  The logical parameters are decode(de-interleave(data), de-interleave(check)).
 * Pairs: code 1 with scheme 0 (every network) and with scheme 2 (cnvW1A1, cnvW1A2).  Refused with the reason: code 1
 * with scheme 1 (TMR plus a code is not modelled) or 3 (the resilient patterns are defined for 32 and 48 positions
 * only), everything the scheme alone refuses, code outside 0 ... 1.
 * Upsets: the data memories draw as in the exposure campaigns (module 0).  The check memory draws by the same
 * construction at element width 6: per_c = ceil(6 / b) groups per element, the last one clipped to 6, e = element *
 * per_c + g,
 *     u = philox4x32_10(counter {L, 1 | 1 << 1 | (b - 1) << 8, e >> 2, 1 + (t << 8)}, key {seed})[e & 3],
 * an event iff u < rate_t_q32[L].  A check event is the 9-int physical record with target 1, module 1, bit = g * b and
 * word_size b: a pure XOR of bits [bit, min(bit + b, 6)) of the check word.  Bursts do not cross from the data memory
 * into the check memory.  Order inside an epoch: layer-major, weights then thresholds, module-major (data, then check),
 * in event order.  Epochs, the scrub (a full rewrite, of data and check words) and the epoch cap are exposure_campaigns'
 * own; the REPAIR scrub that writes the decoder's output back: repair_exposure_campaigns below.
 * ecc_encode / ecc_decode: host only; the 6 check bits / the status, the delivered data in *out_data.
 * ecc_layout: out = {weight modules, threshold modules (2 where coded: data plus check), interleave, check bits 0 / 6};
 * -1 + last_error for a refused pair.
 * ecc_check_site: logical -> physical for bit `bit` (0 ... 5) of the check word of line `ind` (hardened_site answers for
 * data bits); -1 for a layer without a check memory.
 * ecc_exposure_mask: exposure_mask with the code; code 1: module 1 of a coded layer's thresholds lists the check events.
 * pack_params_ecc: load the physical state, apply the 9-int records in order, de-interleave, decode, pack.  Code 0:
 * pack_params_hardened.
 * ecc_exposure_campaigns: exposure_campaigns' conventions and refusals plus those above.  Code 0: its classes, counts
 * (in the first four longs) and seeds bit for bit.  All rates 0: the fault-free classes, no upset kernel launched.  The
 * last_* state is this entry point's own; num_runs * E * layers * 6 must stay below 2^31.
 * ecc_exposure_params: the blob a run classifies epoch `epoch` with, made by the campaign's own kernels and read back.
 * last_ecc_exposure_counts: per [run][epoch][layer] six longs: weights physical, logical; thresholds physical (data plus
 * check bits flipped in the epoch), logical (data bits that differ after decoding); the threshold words whose decode
 * status after the epoch is 1; those whose status is 2 (both 0 for an uncoded layer).  Returns runs * E * layers * 6. */
unsigned int bnn_mi355x_ecc_encode(unsigned int data);
int bnn_mi355x_ecc_decode(unsigned int data, unsigned int check, unsigned int *out_data);
int bnn_mi355x_ecc_layout(int scheme, int code, int layer, int out[4]);
int bnn_mi355x_ecc_check_site(int scheme, int code, int layer, int ind, int bit, int *p_ind, int *p_bit);
long bnn_mi355x_ecc_exposure_mask(int scheme, int code, int burst, unsigned long long run_seed, int epoch, int layer,
                                  int target, int module, unsigned int rate_q32, long first, int *records, int cap_records);
size_t bnn_mi355x_pack_params_ecc(const char *path, int scheme, int code, const int *records, int n_faults, void *dst,
                                  size_t cap);
int *bnn_mi355x_ecc_exposure_campaigns(const char *path, int number_class, int scheme, int code, int burst, int num_runs,
                                       unsigned long long seed, const unsigned int *rate_w_q32,
                                       const unsigned int *rate_t_q32, int n_rates, int epoch_images, int scrub_every,
                                       int *image_number, float *usecPerImage);
size_t bnn_mi355x_ecc_exposure_params(int scheme, int code, int burst, unsigned long long run_seed,
                                      const unsigned int *rate_w_q32, const unsigned int *rate_t_q32, int n_rates, int epoch,
                                      int scrub_every, void *dst, size_t cap);
int bnn_mi355x_last_ecc_exposure_counts(long *counts, int cap);
int bnn_mi355x_last_ecc_exposure_seeds(unsigned long long *seeds, int cap);

/* Repair scrubs in the exposure campaigns: the scrub a system that flies TMR or a code really has.  scrub_every's full
 * rewrite needs the golden copy; a REPAIR reads a word, votes or decodes it, and writes the result back.  Like the voter
 * and the code it is this project's own model (csrc/mem_org.h "repair scrubs", csrc/ecc.h): parity unpinned.
 * repair_every = P >= 0 goes next to scrub_every = S: before the upsets of epoch t > 0 a full rewrite happens if S > 0 and
 * t % S == 0 (and then no repair in that epoch); otherwise a repair happens if P > 0 and t % P == 0.  A repair visits
 * every physical memory that has redundancy:
 *   TMR memories (layer 0's weights, the thresholds of layers 0-4 under scheme 1): the low `ebits` of all three modules'
 *     words become their bitwise majority (the voter);
 *   coded threshold memories (code 1), per logical element: with (d, c) the de-interleaved data and check words and
 *     st = ecc_decode(d, c, &d'): st = 1, d' and ecc_encode(d') are stored (scheme 2: re-interleaved; only the element's
 *     own bits of the two physical lines change); st = 0 or 2, nothing is written;
 *   every other memory is untouched: the weights of layers >= 1, single-module thresholds, uncoded memories (CNV layer 0
 *     under code 1 included).
 * So it fixes only what the redundancy covers, and locks in what the redundancy gets wrong (a TMR bit hit in two
 * modules; a triple error the decoder accepts: a status-1 result is always a valid code word).  The delivered parameters
 * are the same before and after a repair.
 * ecc_repair: host only; the decode status, and in *out_data / *out_check what a repair leaves stored of (data, check).
 * pack_params_repair: pack_params_ecc with two MARKER records among the 9-int records, told by their layer field: -1
 * repair all memories now, -2 rewrite all memories from the loaded parameters now (the other eight ints are not read).
 * Without markers it is pack_params_ecc byte for byte; any other negative layer is refused, naming the record.  The
 * blob of (run, epoch t) is pack_params_repair of the concatenation over epochs 0 ... t of [the epoch's marker, if one is
 * due] + ecc_exposure_mask's records of that epoch in the in-epoch order.  Host only.
 * repair_exposure_campaigns: ecc_exposure_campaigns' conventions and refusals, plus repair_every < 0 and num_runs * E *
 * layers * 8 >= 2^31; TMR plus a code stays refused.  repair_every 0: that function's classes, six counts, seeds and
 * blobs bit for bit.  The last_* state is this entry point's own.
 * repair_exposure_params: the blob a run classifies epoch `epoch` with, made by the campaign's own steps and read back.
 * last_repair_exposure_counts: per [run][epoch][layer] eight longs: the six of last_ecc_exposure_counts, then [6] the
 * logical words the repair of that epoch rewrote (TMR: words where some module differed from the vote, counted once;
 * coded: status-1 words) and [7] the words of the layer's repaired memories whose stored state still differs from the
 * loaded one after the repair (TMR: vote != loaded; coded: left at status 2, or a wrong code word, written now or locked
 * in earlier).  Both 0 in an epoch without a repair and for a layer without redundancy; CNV layer 0 counts weights and
 * thresholds together, the other layers thresholds.  Returns runs * E * layers * 8. */
int bnn_mi355x_ecc_repair(unsigned int data, unsigned int check, unsigned int *out_data, unsigned int *out_check);
size_t bnn_mi355x_pack_params_repair(const char *path, int scheme, int code, const int *records, int n_faults, void *dst,
                                     size_t cap);
int *bnn_mi355x_repair_exposure_campaigns(const char *path, int number_class, int scheme, int code, int burst,
                                          int num_runs, unsigned long long seed, const unsigned int *rate_w_q32,
                                          const unsigned int *rate_t_q32, int n_rates, int epoch_images, int scrub_every,
                                          int repair_every, int *image_number, float *usecPerImage);
size_t bnn_mi355x_repair_exposure_params(int scheme, int code, int burst, unsigned long long run_seed,
                                         const unsigned int *rate_w_q32, const unsigned int *rate_t_q32, int n_rates,
                                         int epoch, int scrub_every, int repair_every, void *dst, size_t cap);
int bnn_mi355x_last_repair_exposure_counts(long *counts, int cap);
int bnn_mi355x_last_repair_exposure_seeds(unsigned long long *seeds, int cap);

/* Coded WEIGHT memories in the exposure campaigns: a third axis `weight_code` next to `scheme` and `code`.  0 none; 1
 * SEC-DED (72,64) -- Hamming(71,64) plus an overall parity bit, what block RAM ECC is -- over the weight memory of every
 * layer but CNV layer 0 (every layer >= 1 of the CNV nets, all four of the LFC nets).  Like the voter, the threshold code
 * and the repair it is this project's own model (csrc/wecc.h, csrc/mem_org.h "coded weight memories"): parity unpinned.
 *   Code word positions are 1 ... 71; positions 1, 2, 4, ..., 64 hold check bits c0 ... c6, the others in increasing order
 *   data bits 0 ... 63; c7 is the XOR of all data bits and c0 ... c6.  Decode, with s the syndrome and P the overall
 *   parity: P = 0, s = 0: status 0; P = 1 and s = 0 or a power of two: status 1, data as stored; P = 1 and s a data
 *   position: status 1, that bit flipped; P = 1 and s > 71, or P = 0 and s != 0: status 2, data as stored.
 * Code word q of a layer is sites [64 q, 64 q + 64) of its weight memory in the PE-major site order of
 * enumerate_faults (2-bit weights: a site is one bit of an ap_int<2> field, a code word covers 32 columns).  Its 8 check
 * bits are element q of a check memory of the layer's own, (PE, code word of the PE) shaped, addressed as MODULE 1 of
 * target 0.  The data memory's events are exactly the uncoded campaign's records; the check memory draws by the same
 * construction at element width 8 with module 1 in the counter word, at the layer's weight rate: record fields mem = PE,
 * ind = code word of the PE, bit = g * burst, word_size = burst, an event the XOR of bits [bit, min(bit + burst, 8)).
 * The logical weights are decode(data, check).  A repair epoch stores, per code word at status 1, the delivered data
 * and its check bits, and writes nothing at status 0 or 2; a full rewrite clears the weight memories like every other.
 * CNV layer 0 is not coded (3- or 6-bit elements, the host route, replicated by TMR).  weight_code 1 goes with every
 * (scheme, code, repair_every) combination repair_exposure_campaigns accepts, TMR included.
 * wecc_encode / wecc_decode / wecc_repair: host only; the 8 check bits; the decode status and in *out_data the delivered
 * data; the status and what a repair leaves stored of (data, check).
 * wecc_layout: out[0] 1 where the layer's weight memory is coded, out[1] its code words per PE, out[2] its check bits (8
 * or 0).  Returns 0, or -1 + last_error for a weight_code outside 0 ... 1 or a bad layer.  Host only.
 * wecc_exposure_mask: ecc_exposure_mask plus weight_code; module 1 of target 0 lists a coded layer's check events.
 * pack_params_wecc: pack_params_repair plus weight_code: the same 9-int records and -1 / -2 markers.  Host only.
 * wecc_exposure_campaigns: repair_exposure_campaigns' arguments, conventions and refusals plus weight_code (outside
 * 0 ... 1: refused before a device is looked for) and num_runs * E * layers * 12 >= 2^31.
 * wecc_exposure_params: the blob a run classifies epoch `epoch` with.
 * last_wecc_exposure_counts: per [run][epoch][layer] twelve longs: the eight of last_repair_exposure_counts (weights
 * physical [0] now counts data plus check bits, weights logical [1] the data bits that differ after decoding), then the
 * weight code words [8] at status 1 and [9] at status 2 after the epoch, [10] those the epoch's repair rewrote and [11]
 * those whose stored state still differs from the loaded one after the repair.  Returns runs * E * layers * 12.
 * With weight_code 0 every one of these returns its predecessor's result bit for bit ([8] ... [11] are 0); the last_*
 * state is these entry points' own. */
unsigned int bnn_mi355x_wecc_encode(unsigned long long data);
int bnn_mi355x_wecc_decode(unsigned long long data, unsigned int check, unsigned long long *out_data);
int bnn_mi355x_wecc_repair(unsigned long long data, unsigned int check, unsigned long long *out_data,
                           unsigned int *out_check);
int bnn_mi355x_wecc_layout(int weight_code, int layer, int out[3]);
long bnn_mi355x_wecc_exposure_mask(int scheme, int code, int weight_code, int burst, unsigned long long run_seed,
                                   int epoch, int layer, int target, int module, unsigned int rate_q32, long first,
                                   int *records, int cap_records);
size_t bnn_mi355x_pack_params_wecc(const char *path, int scheme, int code, int weight_code, const int *records,
                                   int n_faults, void *dst, size_t cap);
int *bnn_mi355x_wecc_exposure_campaigns(const char *path, int number_class, int scheme, int code, int weight_code,
                                        int burst, int num_runs, unsigned long long seed, const unsigned int *rate_w_q32,
                                        const unsigned int *rate_t_q32, int n_rates, int epoch_images, int scrub_every,
                                        int repair_every, int *image_number, float *usecPerImage);
size_t bnn_mi355x_wecc_exposure_params(int scheme, int code, int weight_code, int burst, unsigned long long run_seed,
                                       const unsigned int *rate_w_q32, const unsigned int *rate_t_q32, int n_rates,
                                       int epoch, int scrub_every, int repair_every, void *dst, size_t cap);
int bnn_mi355x_last_wecc_exposure_counts(long *counts, int cap);
int bnn_mi355x_last_wecc_exposure_seeds(unsigned long long *seeds, int cap);

/* COLUMN-INTERLEAVED code words over the coded weight memories: a fourth axis `weight_interleave`.  0 none (everything
 * above, unchanged); 1 column-interleaved.  It needs weight_code 1 and covers exactly the layers weight_code 1 covers.
 * Why: a burst stays inside one element, and with weight_code 1 alone all its bits land in one code word -- an aligned
 * burst of 2 in an even-width element flips an even number of bits of it, the overall parity never fires and nothing is
 * corrected.  Real block RAM ECC stripes adjacent columns over different code words.  The project's own model
 * (csrc/mem_org.h "column-interleaved code words"), like the code it lays out: parity unpinned.
 *   Depth, per layer: D = gcd(16, code words per PE) (16 the widest burst); an odd count gives D = 1, coded and not
 *   interleaved.  Group G of a layer is D consecutive code words' worth of storage in the site order: data sites
 *   [64 D G, 64 D (G + 1)), check elements [D G, D (G + 1)).  The site at offset p of the group is data bit p / D of code
 *   word p % D of the group; the check bit at offset r = 8 * element + bit is check bit r / D of code word r % D.  The
 *   weights stay where they were and the upsets are unchanged: the events of both memories are weight_code 1's records,
 *   which wecc_exposure_mask lists (there is no mask entry point of this family).  A burst of b bits lands in min(b, D)
 *   code words.  Delivery, repair and rewrite are weight_code 1's, per code word over the gathered bits.
 * iwecc_layout: out[0 ... 2] are wecc_layout's, out[3] the depth (0 where the layer is not coded, 1 where coded and not
 * interleaved).  Returns 0, or -1 + last_error.  Host only.
 * iwecc_site: module 0: index a data site of the layer's weight memory; module 1: index a check bit, 8 * element + bit.
 * out[0] the code word of the layer (PE-major), out[1] the bit of the code word (0 ... 63, or 0 ... 7).  Returns 0, or -1 +
 * last_error for a bad argument or a layer that is not coded.  Host only.
 * pack_params_iwecc: pack_params_wecc plus weight_interleave.  Host only.
 * iwecc_exposure_campaigns / _params: wecc_exposure_campaigns / _params plus weight_interleave behind weight_code.
 * Refused before a device is looked for: weight_interleave outside 0 ... 1, and weight_interleave 1 without weight_code 1.
 * last_iwecc_exposure_counts: the twelve longs of last_wecc_exposure_counts; [8] ... [11] count code words after
 * gathering, not physical 64-site words; [0] is weight_code 1's, the events being the same.
 * With weight_interleave 0 every one of these returns its wecc predecessor's result bit for bit; the last_* state is
 * these entry points' own. */
int bnn_mi355x_iwecc_layout(int weight_code, int weight_interleave, int layer, int out[4]);
int bnn_mi355x_iwecc_site(int weight_code, int weight_interleave, int layer, int module, long index, long out[2]);
size_t bnn_mi355x_pack_params_iwecc(const char *path, int scheme, int code, int weight_code, int weight_interleave,
                                    const int *records, int n_faults, void *dst, size_t cap);
int *bnn_mi355x_iwecc_exposure_campaigns(const char *path, int number_class, int scheme, int code, int weight_code,
                                         int weight_interleave, int burst, int num_runs, unsigned long long seed,
                                         const unsigned int *rate_w_q32, const unsigned int *rate_t_q32, int n_rates,
                                         int epoch_images, int scrub_every, int repair_every, int *image_number,
                                         float *usecPerImage);
size_t bnn_mi355x_iwecc_exposure_params(int scheme, int code, int weight_code, int weight_interleave, int burst,
                                        unsigned long long run_seed, const unsigned int *rate_w_q32,
                                        const unsigned int *rate_t_q32, int n_rates, int epoch, int scrub_every,
                                        int repair_every, void *dst, size_t cap);
int bnn_mi355x_last_iwecc_exposure_counts(long *counts, int cap);
int bnn_mi355x_last_iwecc_exposure_seeds(unsigned long long *seeds, int cap);

/* Propagation profiles of the single-fault sweeps: where a fault is masked.  With S the network's layers a profile has
 * S - 1 columns, one per layer with an output map -- the maps bnn_mi355x_enumerate_act_faults has sites in: CNV column
 * l = the output of layer l, l = 0 ... 7 (layers 1 and 3: after the max-pool); LFC column l = the output of layer l,
 * l = 0 ... 2 (the binarised input is no column).  For record f of a sweep over n images
 *     alive[f][l]   = the images whose layer-l output differs from the fault-free layer-l output of that image,
 *     flipped[f][l] = the activations (one channel of one pixel) that differ, summed over those images:
 * 1-bit maps, the differing bits of the packed rows; 2-bit maps, the channels whose level differs (the stages write the
 * level 0 in one form only, so the (sign, non-zero) bits differ exactly where the levels do).  Columns before the first
 * layer the sweep evaluates for the record are 0; that layer is L for a parameter fault in layer L, L + 1 for an
 * activation site of layer L, 0 for an input site.  So a parameter fault in the last layer and an activation site of
 * the last hidden layer have all-zero rows: changed[f] is their only result.  Dropping the pairs whose activations
 * equal the fault-free ones loses nothing: such a pair has the fault-free output at every later layer, so the profile
 * equals the one of classifying every pair through every layer.  The counts come from the compare that prunes the
 * pairs (a kernel that counts the differing activations where the default one only notes that there are some).
 * sweep_profile: 1: the single-fault sweeps called from now on (fault_sweep, act_fault_sweep, input_fault_sweep) also
 * record a propagation profile; 0 (the default): they do not.  Returns the previous setting.  Host only.
 * last_sweep_profile: the profile of the last sweep that ran with profiling on, rows in the order of that call's
 * records.  Writes rows [first, first + cap_rows) of `columns` longs each into alive and flipped (either may be NULL),
 * *columns (may be NULL) = layers - 1.  Returns the number of rows of the profile (0 before the first profiled sweep),
 * -1 + last_error for a negative first.  A profiled sweep that fails leaves no profile; a sweep with profiling off
 * leaves the previous one in place.  Host only. */
int bnn_mi355x_sweep_profile(int enable);
long bnn_mi355x_last_sweep_profile(long first, long *alive, long *flipped, long cap_rows, int *columns);

/* The step before the path: CnvClassifier.image_to_cifar (bnn/bnn.py:226-242) on the
 * device.  The reference shrinks a picture with PIL's Image.thumbnail((32, 32), ANTIALIAS) -- Lanczos-3,
 * Pillow's 8-bit fixed-point two-pass resampler -- pastes it centred on a white 32x32 canvas and writes
 * a CIFAR-10 record: label byte 1, then the R, G, B planes (3073 bytes).  These two entry points do the
 * same for decoded pictures in host memory; the records are bit-identical to Pillow's
 * (tests/test_image_to_cifar.py).  CNV libraries only.
 *   pixels[i]: heights[i] rows of widths[i] pixels of bands[i] bytes (1 = mode "L", 3 = "RGB", 4 = "RGBA":
 *              resampled with premultiplied alpha like Image.resize does, the alpha channel then dropped),
 *              rows row_strides[i] bytes apart (row_strides NULL: packed rows);
 *   records:   n_images x 3073 bytes, host.
 * Pictures of other modes (palette, LA, CMYK, ...) stay with PIL on the host, like in the reference.
 * thumbnail_size: the size Image.thumbnail((32, 32)) gives a width x height picture; returns 1 when
 * the picture is resampled, 0 when it already fits (out = in). */
int bnn_mi355x_thumbnail_size(int width, int height, int *out_w, int *out_h);
int bnn_mi355x_images_to_cifar(const uint8_t *const *pixels, const int *widths, const int *heights, const int *bands,
                               const long *row_strides, int n_images, uint8_t *records);

/* Locate objects in a scene (CNV-BNN_Road-Signs.ipynb cells 13-16): every window of ONE picture becomes a CIFAR-10
 * record -- and, with classify_windows, a class -- in one call.  The notebook tiles a street picture into overlapping
 * windows, crops each one (im.crop(bound)) and classifies the crops; here the picture goes to the device once, all
 * windows of one size share one pair of coefficient tables and one kernel launch (csrc/window_kernels.hip), and
 * classify_windows never brings the records back.  CNV libraries only (-1 / NULL + last_error on an LFC library).
 *   pixels, width, height, bands, row_stride: the picture, as one picture of images_to_cifar (bands 1 = "L", 3 = "RGB",
 *              4 = "RGBA"; row_stride 0 = packed rows).  It is not modified.
 *   boxes:     n_windows x 4 ints (left, upper, right, lower), exactly what Image.crop takes.
 * tile_boxes: the notebook's tiling rule for ONE window size; host only, touches no GPU.  stride = size / 4, x_tiles =
 *       width / stride, y_tiles = height / stride; rows are the outer loop, columns the inner one; a box is kept when
 *       right <= width && lower < height.  The notebook is strict on the height and not on the width (a window may
 *       touch the right edge of the picture but not the lower one); that is reproduced as it is.  Returns the number of
 *       boxes of that size and writes at most `cap` of them (boxes may be NULL); -1 + last_error for size < 4.  A
 *       640 x 480 picture gives 962 boxes of 64 and 368 of 96: the 1 330 the notebook prints.
 * windows_to_cifar: record i (3073 bytes, host) is byte-identical to what image_to_cifar writes for
 *       Image.fromarray(pixels).crop(boxes[i]); records come in the caller's order whatever grouping runs inside.
 * classify_windows: the same records, but their 3072-byte bodies stay in HBM and the pass bnn_mi355x_inference_device
 *       enqueues runs on them on the same stream; the classes (or, with enable_detail, number_class scores per window)
 *       come back in one copy.  Return convention and ownership as bnn_mi355x_inference_buffer (free with
 *       free_results).  usecPerImage: the device time of the classification pass per window, as in the other entry
 *       points; usecPreprocess (may be NULL): the device time of the uploads and the window kernels, per window.
 * Refused, before anything touches the GPU, with -1 / NULL + last_error naming the first offending box: a box with
 * right <= left or lower <= upper; a box that leaves the picture (Pillow would pad it with zeros; the notebook filters
 * such boxes out, so they are not modelled); bands other than 1, 3, 4; a row stride shorter than a row; null pointers
 * with n_windows > 0.  n_windows == 0 succeeds.
 * Windows whose horizontal-pass output (height x out_w x bands bytes) exceeds BNN_MI355X_WINDOW_LDS_BYTES, and windows
 * Pillow resamples vertical pass first (height > 100 x width), go one by one through the kernels of images_to_cifar. */
#define BNN_MI355X_WINDOW_LDS_BYTES 32768
long bnn_mi355x_tile_boxes(int width, int height, int size, int *boxes, long cap);
int bnn_mi355x_windows_to_cifar(const uint8_t *pixels, int width, int height, int bands, long row_stride, const int *boxes,
                                int n_windows, uint8_t *records);
int *bnn_mi355x_classify_windows(const uint8_t *pixels, int width, int height, int bands, long row_stride, const int *boxes,
                                 int n_windows, int number_class, float *usecPerImage, float *usecPreprocess,
                                 int enable_detail);

/* Scan a scene densely: every 32 x 32 window of a picture at stride 4, from ONE pass over the whole picture
 * (csrc/scan_kernels.hip; the model: csrc/scan.h).  All CNV convolutions are "valid" 3 x 3 and the two pools
 * 2 x 2, so layers 0-5 are fully convolutional: layer-5 pixel (i, j) of the picture holds the 256 bits the per-window pass
 * computes for the record cut at columns 4i .. 4i + 31, rows 4j .. 4j + 31, and layers 6-8 with the decode run on those as on
 * nx * ny images.  Window (i, j) of a result -- raster order, j the outer index -- equals, bit for bit on all 64 raw scores,
 * what bnn_mi355x_inference_buffer returns for that record.  cnvW1A1 libraries only: -1 / NULL + last_error on cnvW1A2 and
 * cnvW2A2 ("... the dense scan is built for cnvW1A1 only") and on LFC libraries.
 *   planes:    the picture as a "large CIFAR record body": planar uint8 [3][height][width], packed.
 *   grid:      nx = (width - 32) / 4 + 1, ny = (height - 32) / 4 + 1; the up to 3 columns and rows beyond
 *              32 + 4 (nx - 1) x 32 + 4 (ny - 1) are not read.
 * scan_grid: host only; -1 + last_error for a side below 32.
 * scan_boxes: host only.  The level rule of scan_scene for ONE window size (8 or more, a multiple of 8): the picture is
 *       resized to level_w = width * 32 / size, level_h = height * 32 / size (integer division; refused below 32) and
 *       cell (i, j) of that level's scan is the window (i size / 8, j size / 8, i size / 8 + size, j size / 8 + size) of the
 *       picture -- always inside it.  Returns the number of boxes and writes at most `cap` of them (boxes may be NULL; 4
 *       ints each, rows outer); level_w / level_h may be NULL; -1 + last_error for a refused size or level.
 * scan_planes: host picture in, `new int[]` of nx * ny classes (or, with enable_detail, number_class scores per window)
 *       out.  Return convention and ownership as bnn_mi355x_inference_buffer (free with free_results); usecPerImage: the
 *       device time of the whole pass per window.
 * scan_device: the same on a picture already in HBM (d_planes packed as above), enqueued on hip_stream under the
 *       serialisation rules of bnn_mi355x_inference_device: d_classes (nx * ny ints) and d_scores (nx * ny x 64 int16)
 *       may each be NULL; the maps live in a workspace of the library that every scan call shares.  The workspace for the
 *       picture's size must exist before a stream capture begins (a first call of that size allocates it).
 * scan_scene: a pyramid.  One upload of an interleaved picture (pixels, width, height, bands, row_stride as for
 *       windows_to_cifar, bands 1 = "L" -- the grey plane in all three -- or 3 = "RGB"; RGBA is refused here); for each of
 *       the n_sizes window sizes the picture is resized to its level like Image.resize((level_w, level_h), Image.LANCZOS) of
 *       Pillow 12, byte for byte (a level of the picture's own size is taken as it is), and scanned, all on one stream.
 *       Results are size-major, then raster; boxes_out receives every window's box (4 ints; size it with scan_boxes).
 *       usecPerImage: the scans' device time per window; usecPreprocess (may be NULL): the upload's and the resizes'.
 * debug_scan_stage: test hook, the twin of bnn_mi355x_debug_stage_output: runs stages 0..stage (0..5 = layers 0..5) on the
 *       picture and copies that stage's map as it lies in HBM -- [map_h][map_w][dwords], dwords = 2, 2, 4, 4, 8, 8 per pixel,
 *       bit-packed HWC -- to out; returns the bytes, or -1 (cap too small included).
 * scan_resize: one level on its own, for any output size (1 .. BNN_MI355X_SCAN_MAX_SIDE a side): the planar picture
 *       [3][out_h][out_w] (host) the scan of that level reads, i.e. Image.resize((out_w, out_h), Image.LANCZOS) of the
 *       interleaved picture with the bands apart.  Exists so that the resize can be compared with Pillow by itself.
 * Limits, refused before anything touches the GPU: a side of the picture (or of a level) above BNN_MI355X_SCAN_MAX_SIDE;
 * more than BNN_MI355X_SCAN_MAX_WINDOWS windows in one picture (or level); maps of more than BNN_MI355X_SCAN_MAX_MAP_BYTES
 * for one picture (or level).  Also refused: sides below 32, null pointers, number_class outside 1..64.  Workspaces are
 * grow-only. */
#define BNN_MI355X_SCAN_MAX_SIDE 8192
#define BNN_MI355X_SCAN_MAX_WINDOWS 1048576
#define BNN_MI355X_SCAN_MAX_MAP_BYTES 134217728
int bnn_mi355x_scan_grid(int width, int height, int *nx, int *ny);
long bnn_mi355x_scan_boxes(int width, int height, int size, int *boxes, long cap, int *level_w, int *level_h);
int *bnn_mi355x_scan_planes(const uint8_t *planes, int width, int height, int number_class, int *nx, int *ny, float *usecPerImage,
                            int enable_detail);
int bnn_mi355x_scan_device(const void *d_planes, int width, int height, int number_class, int32_t *d_classes, int16_t *d_scores,
                           void *hip_stream);
int *bnn_mi355x_scan_scene(const uint8_t *pixels, int width, int height, int bands, long row_stride, const int *sizes, int n_sizes,
                           int number_class, int *boxes_out, float *usecPerImage, float *usecPreprocess, int enable_detail);
long bnn_mi355x_debug_scan_stage(const uint8_t *planes, int width, int height, int stage, void *out, size_t cap, int *map_w, int *map_h);
int bnn_mi355x_scan_resize(const uint8_t *pixels, int width, int height, int bands, long row_stride, int out_w, int out_h,
                           uint8_t *planes);

/* Scan a clip: n_frames pictures of ONE size (a video, a camera feed) and n_sizes window sizes in one call, every (frame,
 * level) map through ONE launch per stage of layers 0-5 and layers 6-8 with the decode ONCE on all windows
 * (csrc/scan_clip_kernels.hip; the model: csrc/scan_clip.h, DESIGN.md 9 "Clip scan").  The levels, grids and boxes are
 * scan_scene's, and frame f of a result equals, bit for bit on all 64 raw scores, what bnn_mi355x_scan_scene returns for
 * frame f; with n_frames = 1 the call merges the levels of one scene.  cnvW1A1 libraries only, refused elsewhere in the
 * scan's two messages.
 *   clip:      frames of interleaved uint8, bands 1 ("L") or 3 ("RGB") as for scan_scene; rows row_stride bytes apart
 *              (0 = packed), frames frame_stride bytes apart (0 = packed: height rows at the row stride); a frame stride
 *              shorter than that is refused.
 *   maps:      map m = f * n_sizes + k is frame f at sizes[k].  Results are frame-major, then size-major, then raster:
 *              the windows of map m are [first[m], first[m] + nx_k * ny_k), first the running sum in map order.
 *   layout:    stage s (0..5) of map m lies at byte offset off[s][m] of buffer s & 1, off[s][m] the sum of the bytes of
 *              the earlier maps of that stage ([map_h][map_w][dwords] each, as debug_scan_stage describes them); every
 *              offset is a multiple of 8 and off[5][m] = 32 first[m].
 * scan_clip: one upload of the clip; per level ONE pair of resize launches for all frames (Pillow's LANCZOS, byte for byte,
 *       as scan_scene; the frames share the level's tables); six stage launches; layers 6-8 and the decode once.  Returns a
 *       `new int[]` of windows classes (or, with enable_detail, number_class scores per window), return convention and
 *       ownership as scan_scene (free with free_results).  boxes_out receives ONE frame's boxes, exactly what scan_scene
 *       writes (they are the same for every frame).  usecPerImage: the device time of the stages per window;
 *       usecPreprocess (may be NULL): the upload's and the resizes'.
 * scan_clip_capacity: host only.  The largest n_frames one scan_clip call accepts for RGB frames of this size with these
 *       window sizes (L frames: at least as many); 0 + last_error when even one frame is refused, -1 + last_error on a
 *       library that does not scan.
 * scan_clip_layout: host only.  Returns the number of maps M = n_frames * n_sizes (-1 + last_error when the clip is
 *       refused) and writes, each pointer optional: map_w, map_h and offsets as [M][6] (map m, stage s at m * 6 + s), first
 *       and level_size (the map's window size) as [M], buf_bytes[2] the bytes of the two map buffers.
 * debug_scan_clip_stage: test hook, the twin of debug_scan_stage: runs the resizes and stages 0..stage on the clip and
 *       copies that stage's whole buffer region -- every map packed as the layout says -- to out; returns the bytes, or -1
 *       (cap too small included).
 * Limits, refused before anything touches the GPU: every frame and every level stays inside the scan's per-picture limits;
 * n_frames outside 1 .. BNN_MI355X_SCAN_CLIP_MAX_FRAMES; more than BNN_MI355X_SCAN_MAX_WINDOWS windows over all maps; either
 * map buffer above BNN_MI355X_SCAN_MAX_MAP_BYTES; an uploaded clip (n_frames x width x height x bands) above
 * BNN_MI355X_SCAN_CLIP_MAX_BYTES; what scan_scene refuses, in its words.  Workspaces are grow-only and shared with the scan's. */
#define BNN_MI355X_SCAN_CLIP_MAX_FRAMES 4096
#define BNN_MI355X_SCAN_CLIP_MAX_BYTES 1073741824
int *bnn_mi355x_scan_clip(const uint8_t *pixels, int n_frames, long frame_stride, int width, int height, int bands, long row_stride,
                          const int *sizes, int n_sizes, int number_class, int *boxes_out, float *usecPerImage, float *usecPreprocess,
                          int enable_detail);
int bnn_mi355x_scan_clip_capacity(int width, int height, const int *sizes, int n_sizes);
int bnn_mi355x_scan_clip_layout(int width, int height, const int *sizes, int n_sizes, int n_frames, int *map_w, int *map_h, long *offsets,
                                long *first, int *level_size, long *buf_bytes);
long bnn_mi355x_debug_scan_clip_stage(const uint8_t *pixels, int n_frames, long frame_stride, int width, int height, int bands, long row_stride,
                                      const int *sizes, int n_sizes, int stage, void *out, size_t cap);

/* Detect objects: the windows of a frame and their scores become a short list of boxes, each with a class and a score --
 * threshold, order, cap and greedy non-maximum suppression, on the device (csrc/detect_kernels.hip; the model:
 * csrc/detect.h, DESIGN.md 9 "Detections").  The model is this project's own (the reference notebook draws every window
 * that fires, CNV-BNN_Road-Signs.ipynb cells 14 and 16); it is pure integer, and the device results equal the host's
 * byte for byte.
 *   inputs:    per frame n windows with a box (left, upper, right, lower) each -- 0 <= left < right <= 65535, likewise
 *              upper < lower; ONE frame's boxes, shared by all frames -- and number_class scores each.
 *   class:     by_score = 0: the decode's class (the first strict maximum over the first number_class scores, floored at
 *              0: scores <= 0 never beat class 0).  by_score = 1: class_mask has exactly one bit k and the class is k
 *              whatever the argmax (cell 16's rule, result[i][14] > 455).
 *   candidate: the class is in class_mask and score[class] > min_score (-32769 admits every window).
 *   order:     score descending, then window index ascending (size-major, then raster, as everywhere in the scan).  Only
 *              the first max_candidates take part; n_candidates[f] counts all that passed, so a cut is visible.
 *   suppress:  walk the order and keep a candidate unless an already kept candidate OF THE SAME CLASS has
 *              inter * iou_den > iou_num * union (strictly, 64-bit integers); iou_num == iou_den never suppresses.  Stop
 *              after max_det kept candidates.
 *   output:    dets [frames][max_det][8]: left, upper, right, lower, class, score, window index in the frame, window
 *              size (right - left); the rows of a frame past counts[f] are zero.  counts, n_candidates: [frames].
 * detect_windows_host: the model on the host; any library, no GPU.  scores: int [frames][n][number_class], what every
 *       *_details call returns; values outside int16 are refused.  Returns 0, -1 + last_error.
 * detect_windows: the same arguments through the kernels on uploaded boxes and scores; only the lists come back.  CNV
 *       libraries (all three; no parameters need be loaded).  usecDetect (may be NULL): the device time of the detection
 *       launches per frame.
 * detect_clip: scan_clip's upload, resizes, six stage launches and layers 6-8 with the decode writing classes AND scores,
 *       then the detection launches on the same stream; nothing but dets, counts and n_candidates is downloaded.  One
 *       scene is a clip of one frame.  cnvW1A1 only, refused elsewhere in the scan's words; whatever scan_clip refuses is
 *       refused here.  usecPerImage, usecPreprocess: as scan_clip; usecDetect: as detect_windows.
 * Refused before anything touches the GPU, the message naming the argument: null pointers; frames outside 1 ..
 * BNN_MI355X_SCAN_CLIP_MAX_FRAMES; n below 1 or n x frames above BNN_MI355X_SCAN_MAX_WINDOWS; number_class outside 1..64;
 * a class_mask of 0 or with a bit at or above number_class; by_score other than 0 / 1, or 1 with several bits in the
 * mask; iou_den outside 1 .. 65536; iou_num outside 0 .. iou_den; max_candidates outside 1 ..
 * BNN_MI355X_DETECT_MAX_CANDIDATES; max_det outside 1 .. max_candidates; an empty, inverted or out-of-range box; a score
 * outside int16.  Workspaces are grow-only. */
#define BNN_MI355X_DETECT_MAX_CANDIDATES 4096
typedef struct {
  uint64_t class_mask;
  int by_score, min_score, iou_num, iou_den, max_candidates, max_det;
} bnn_mi355x_detect_opts;
int bnn_mi355x_detect_windows_host(const int *boxes, int n, const int *scores, int frames, int number_class, const bnn_mi355x_detect_opts *opts,
                                   int *dets, int *counts, int *n_candidates);
int bnn_mi355x_detect_windows(const int *boxes, int n, const int *scores, int frames, int number_class, const bnn_mi355x_detect_opts *opts,
                              int *dets, int *counts, int *n_candidates, float *usecDetect);
int bnn_mi355x_detect_clip(const uint8_t *pixels, int n_frames, long frame_stride, int width, int height, int bands, long row_stride,
                           const int *sizes, int n_sizes, int number_class, const bnn_mi355x_detect_opts *opts, int *dets, int *counts,
                           int *n_candidates, float *usecPerImage, float *usecPreprocess, float *usecDetect);

/* Camera frames: the clip entry points on frames as a camera or a decoder delivers them, from host memory or from HBM
 * (csrc/pixfmt_kernels.hip; the model: csrc/pixfmt.h, DESIGN.md 9 "Camera frames").  Everything is exact: the frames
 * become the packed RGB frames scan_clip uploads, and everything behind that is scan_clip's code on the same bytes.
 *   format 0 RGB, 1 L   the `bands` 3 and 1 of scan_clip.
 *          2 BGR        3 bytes a pixel, reversed (OpenCV).
 *          3 NV12       a Y plane of `height` rows at row_stride, then interleaved Cb Cr of height / 2 rows at the same
 *                       stride.
 *          4 I420       a Y plane, then a Cb plane of height / 2 rows at row_stride / 2, then a Cr plane likewise.
 *          5 YUYV       Y0 Cb Y1 Cr, 2 bytes a pixel.
 *   Chroma is replicated to the 2 x 2 (NV12, I420) or 2 x 1 (YUYV) pixels it covers; there is no interpolation.
 *   range 0  JFIF full range, byte for byte Pillow's convert("RGB") from mode YCbCr: T_c[i] = (int)(c * 64 * (i - 128) + 0.5)
 *            for c = 1.402, -0.34414, -0.71414, 1.772; R = clip8(Y + (T_1.402[Cr] >> 6)), G = clip8(Y + ((T_-.34414[Cb] +
 *            T_-.71414[Cr]) >> 6)), B = clip8(Y + (T_1.772[Cb] >> 6)).
 *   range 1  BT.601 video range, this project's own statement (parity unpinned): C = Y - 16, D = Cb - 128, E = Cr - 128,
 *            R = clip8((298 C + 409 E + 128) >> 8), G = clip8((298 C - 100 D - 208 E + 128) >> 8), B = clip8((298 C + 516 D +
 *            128) >> 8).  Every shift is arithmetic; range is ignored for RGB, L and BGR.
 *   row_stride, frame_stride: bytes, 0 = packed (the planes of one frame follow one another, and so do the frames).
 * unpack_frames_host: the model on the host; any library, no GPU.  rgb_out: [n_frames][height][width][3].
 * unpack_frames: the kernel on uploaded frames, the RGB comes back.  CNV libraries (no parameters need be loaded).
 *       usecUnpack (may be NULL): the device time of the launch per frame.
 * scan_clip_frames, detect_clip_frames: scan_clip and detect_clip with the struct in place of (n_frames, frame_stride, width,
 *       height, bands, row_stride).  RGB and L are the older entry points bit for bit; the other formats are uploaded as they
 *       are (1.5 to 2 bytes a pixel, scan_clip's one-copy-when-evenly-spaced rules) and unpacked on the device.
 * scan_clip_device, detect_clip_device: the same with d_pixels in HBM.  The work is enqueued on hip_stream under
 *       bnn_mi355x_inference_device's hand-over rules; the call then WAITS for the stream and returns the classes / scores
 *       or the lists on the host, as the host calls do.  The caller's memory is only read, where it lies (packed RGB or L
 *       frames are resized in place, strided ones take one device-to-device copy); no alignment is asked for.  A stream
 *       that is being captured is refused: a graph cannot record the wait or the host results.
 * cnvW1A1 only for the four clip calls, refused elsewhere in the scan's words.  Refused before anything touches the GPU,
 * the message naming the argument: null pointers; an unknown format or range; width or height outside 1 ..
 * BNN_MI355X_SCAN_MAX_SIDE; an odd width (NV12, I420, YUYV) or height (NV12, I420); n_frames outside 1 ..
 * BNN_MI355X_SCAN_CLIP_MAX_FRAMES; a row_stride shorter than a row or, for I420, odd; a frame_stride shorter than a
 * frame; raw frames or RGB frames above BNN_MI355X_SCAN_CLIP_MAX_BYTES; what scan_clip / detect_clip refuse, in their
 * words.  Workspaces are grow-only; bnn_mi355x_scan_clip_capacity holds for every format. */
#define BNN_MI355X_FORMAT_RGB 0
#define BNN_MI355X_FORMAT_L 1
#define BNN_MI355X_FORMAT_BGR 2
#define BNN_MI355X_FORMAT_NV12 3
#define BNN_MI355X_FORMAT_I420 4
#define BNN_MI355X_FORMAT_YUYV 5
typedef struct {
  int format, range, width, height, n_frames;
  long row_stride, frame_stride;
} bnn_mi355x_frames;
int bnn_mi355x_unpack_frames_host(const bnn_mi355x_frames *frames, const void *pixels, uint8_t *rgb_out);
int bnn_mi355x_unpack_frames(const bnn_mi355x_frames *frames, const void *pixels, uint8_t *rgb_out, float *usecUnpack);
int *bnn_mi355x_scan_clip_frames(const bnn_mi355x_frames *frames, const void *pixels, const int *sizes, int n_sizes, int number_class, int *boxes_out,
                                 float *usecPerImage, float *usecPreprocess, int enable_detail);
int bnn_mi355x_detect_clip_frames(const bnn_mi355x_frames *frames, const void *pixels, const int *sizes, int n_sizes, int number_class,
                                  const bnn_mi355x_detect_opts *opts, int *dets, int *counts, int *n_candidates, float *usecPerImage,
                                  float *usecPreprocess, float *usecDetect);
int *bnn_mi355x_scan_clip_device(const bnn_mi355x_frames *frames, const void *d_pixels, const int *sizes, int n_sizes, int number_class, int *boxes_out,
                                 float *usecPerImage, float *usecPreprocess, int enable_detail, void *hip_stream);
int bnn_mi355x_detect_clip_device(const bnn_mi355x_frames *frames, const void *d_pixels, const int *sizes, int n_sizes, int number_class,
                                  const bnn_mi355x_detect_opts *opts, int *dets, int *counts, int *n_candidates, float *usecPerImage,
                                  float *usecPreprocess, float *usecDetect, void *hip_stream);

/* Read handwriting(LFC-BNN_MNIST_Webcam.ipynb and LFC-BNN_Chars_Webcam.ipynb, cells 9-13): ONE picture and N boxes
 * become N MNIST-format records (28 x 28 bytes) -- and, with classify_glyphs, N classes -- in one call.  The notebooks
 * do this by hand with PIL for one camera frame, through two temporary files; here the picture goes to the device once
 * (csrc/glyph_kernels.hip) and classify_glyphs never brings the records back.  LFC libraries only (-1 / NULL +
 * last_error on a CNV library).  Every step is Pillow's arithmetic, bit for bit (Pillow 12):
 *   1 greyscale   L = (R 19595 + G 38470 + B 7471 + 0x8000) >> 16; alpha is ignored, L pictures are taken as they are
 *   2 contrast    m = (2 sum(L) + n) / (2 n) over the WHOLE picture of n pixels (int(ImageStat.mean + 0.5)); v = blend(m,
 *                 v, contrast)
 *   3 brightness  v = blend(0, v, brightness).  blend(a, b, f) = float(a) + f * float(b - a) in single precision, the
 *                 multiply and the add rounded separately; 0 for t <= 0, 255 for t >= 255, else truncated.  A factor
 *                 of exactly 1.0 leaves the plane alone.
 *   4 threshold   v = v > threshold ? 255 : 0 (the chars notebook's 180); -1: none
 *   5 ink box     inside a box, the bounding box of the pixels != 255 (getbbox of the inverse; the notebooks' 80-pixel
 *                 white border only shifts it).  No ink at all: the whole box, status 1, a record with no ink.
 *   6 fit         (w, h) the ink box, ratio = min(28. / h, 28. / w): square -> (28, 28), taller -> (int(w ratio), 28),
 *                 wider -> (28, int(h ratio)); Image.resize of the crop with `filter` 3 (BICUBIC, Pillow's default) or
 *                 0 (NEAREST, the default of the notebooks' 2018 Pillow).  An output dimension of 0 (aspect above 28)
 *                 is status 2, where Pillow raises ValueError: the record is not written, the class is -1.
 *   7 paste       at (int((28 - w') / 2), int((28 - h') / 2)) on white.  The notebooks forget the paste for a SQUARE
 *                 ink box and hand the net a blank record; square_blank = 1 reproduces that, 0 pastes it.
 *   8 record      784 bytes, row-major: 255 where the pasted pixel is exactly 0, 1 everywhere else.
 *   pixels, width, height, bands, row_stride: the picture, as for windows_to_cifar.  It is not modified.
 *   boxes:     n_boxes x 4 ints (left, upper, right, lower) as Image.crop takes them; n_boxes == 0 or boxes == NULL:
 *              the whole picture is the one box (and one record / class comes back).
 *   opts:      the notebooks' values are {3, 4.0, -1, 3, 0} (MNIST) and {5, 2.0, 180, 3, 0} (chars).
 * enhance_picture: steps 1-4; out_L: height x width bytes (host), what the notebooks display; out_mean (may be NULL): m.
 * glyphs_to_mnist: records: n x 784 bytes (host); ink_boxes (may be NULL): n x 4 ints, the ink boxes in picture
 *       coordinates; status (may be NULL): n ints, 0 / 1 / 2 as above.
 * classify_glyphs: the same records stay in HBM and the pass bnn_mi355x_inference_device enqueues runs on them on the
 *       same stream; the classes come back in one copy (with number_class > 47 the words do, and are decoded on the
 *       host like everywhere else).  Return convention, ownership and the two times as classify_windows.
 * Refused before anything touches the GPU, worded like the window entry points: bad boxes (the first one is named), bands,
 * row stride, picture size, null pointers; factors that are not finite or are negative; a threshold outside -1..255; a
 * filter other than 0 / 3.
 * Ink boxes whose horizontal-pass output (height x w' bytes) exceeds BNN_MI355X_GLYPH_LDS_BYTES keep it in a global
 * temporary instead of LDS.
 * glyph_fit, resample_coeffs: host only, touch no GPU (tests).  glyph_fit: step 6 and 7 for a (width, height) ink box,
 *       out (may be NULL) = {w', h', paste x, paste y, status}; returns the status (0 or 2).  resample_coeffs: Pillow's
 *       8-bit fixed-point coefficient table of one axis (k = round(2^22 w), `ksize` ints per output, zero padded) and
 *       its bounds (first input index, tap count per output); returns ksize, -1 for another filter or a size below 1;
 *       kk is written when cap_kk >= out_size x ksize ints, bounds (2 x out_size ints) when it is not NULL. */
#define BNN_MI355X_GLYPH_LDS_BYTES 32768
typedef struct {
  float contrast, brightness;
  int threshold, filter, square_blank;
} bnn_mi355x_glyph_opts;
int bnn_mi355x_glyph_fit(int width, int height, int out[5]);
int bnn_mi355x_resample_coeffs(int filter, int in_size, int out_size, int *kk, int *bounds, int cap_kk);
int bnn_mi355x_enhance_picture(const uint8_t *pixels, int width, int height, int bands, long row_stride,
                               const bnn_mi355x_glyph_opts *opts, uint8_t *out_L, int *out_mean);
int bnn_mi355x_glyphs_to_mnist(const uint8_t *pixels, int width, int height, int bands, long row_stride, const int *boxes,
                               int n_boxes, const bnn_mi355x_glyph_opts *opts, uint8_t *records, int *ink_boxes, int *status);
int *bnn_mi355x_classify_glyphs(const uint8_t *pixels, int width, int height, int bands, long row_stride, const int *boxes,
                                int n_boxes, const bnn_mi355x_glyph_opts *opts, int number_class, float *usecPerImage,
                                float *usecPreprocess, int *status);

/* Find the glyphs of a picture: the connected components of its ink, labelled on the device on the enhanced L plane that
 * the glyph entry points make there (csrc/component_kernels.hip), so that reading a frame is ONE call: upload, enhance,
 * label, boxes, records, classes.  The reference has no segmentation; the model is this project's own (csrc/components.h):
 *   ink        a pixel of the enhanced plane (steps 1-4 above) is ink iff its value is below ink_level (1..255; at 255
 *              this is step 5's rule "!= 255")
 *   adjacency  two different ink pixels are adjacent iff |dx| <= reach_x and |dy| <= reach_y (1..BNN_MI355X_FIND_MAX_REACH
 *              each); the glyphs are the connected components.  Reach (1, 1) is 8-connectivity; a larger reach_y joins
 *              the dot of an "i" to its stem and the bars of an "=".
 *   component  its first pixel (smallest y * width + x), its box (left, upper, right, lower; right and lower exclusive,
 *              as classify_glyphs takes boxes), its number of ink pixels
 *   filter     components of fewer than min_pixels (>= 1) ink pixels are dropped
 *   order      0: ascending first pixel (raster order); 1: ascending (left, upper, first pixel), the reading order of one
 *              line
 *   cap        (>= 1) the first min(cap, total) components in that order are returned; total is the return value and may
 *              exceed cap
 *   find:      NULL is {255, 1, 1, 1, 0}.
 *   boxes:     cap x 4 ints; pixel_counts (may be NULL): cap ints; labels (may be NULL): height x width int32, the index
 *              of the pixel's component in the returned order, -1 for background, for filtered components and for
 *              components beyond the cap.
 * find_glyphs_host: host only, touches no GPU, any library: the model's plain two-pass union-find statement on an L plane
 *       the caller already has (rows row_stride bytes apart, 0: width).  Returns total, -1 + last_error.
 * find_glyphs: picture -> enhanced plane (opts as for classify_glyphs) -> components, on the device.  Returns total.
 * read_glyphs: the same, then the records of the found boxes and the LFC pass on the same stream: exactly the classes
 *       and status classify_glyphs returns for the boxes find_glyphs returns (a glyph's record is the crop of its box: a
 *       neighbour's ink inside the box is part of it).  Returns min(cap, total) classes -- ownership, return convention,
 *       the two times and status (may be NULL, cap ints) as classify_glyphs -- and writes *n_found = total and the boxes.
 *       With no component the result is non-null and empty.  Two host round trips: the component list, the ink boxes.
 * find_glyphs and read_glyphs are LFC only.  Refused before anything touches the GPU: what the glyph entry points
 * refuse; ink_level, a reach, min_pixels, order or cap out of range; a picture of more than BNN_MI355X_FIND_MAX_PIXELS
 * pixels (an int32 label per pixel and 16 bytes of lists per pixel on the device).
 * last_find_usec: device time of the labelling launches (ink words .. compacted list) of the last find_glyphs /
 *       read_glyphs call, in microseconds. */
#define BNN_MI355X_FIND_MAX_PIXELS 16777216
#define BNN_MI355X_FIND_MAX_REACH 16
typedef struct {
  int ink_level, reach_x, reach_y, min_pixels, order;
} bnn_mi355x_find_opts;
int bnn_mi355x_find_glyphs_host(const uint8_t *plane, int width, int height, long row_stride, const bnn_mi355x_find_opts *find,
                                int *boxes, int *pixel_counts, int32_t *labels, int cap);
int bnn_mi355x_find_glyphs(const uint8_t *pixels, int width, int height, int bands, long row_stride,
                           const bnn_mi355x_glyph_opts *opts, const bnn_mi355x_find_opts *find, int *boxes, int *pixel_counts,
                           int32_t *labels, int cap);
int *bnn_mi355x_read_glyphs(const uint8_t *pixels, int width, int height, int bands, long row_stride,
                            const bnn_mi355x_glyph_opts *opts, const bnn_mi355x_find_opts *find, int number_class, int cap,
                            int *n_found, int *boxes, float *usecPerImage, float *usecPreprocess, int *status);
float bnn_mi355x_last_find_usec(void);

/* Read a page: lines of text, every glyph masked to its own ink.  read_glyphs reads ONE line of glyphs whose boxes do
 * not touch; these entry points lift both limits.  The reference has no segmentation; like the labelling above, the
 * model is this project's own (csrc/page.h):
 *   mask = 1   Glyph g is a component find returned.  Its picture is the enhanced plane with every pixel that does not
 *              belong to component g replaced by 255: other components, filtered components, components beyond the cap,
 *              and background, grey values in [ink_level, 255) included.  Steps 5-8 run on that picture with g's box as
 *              the box.  Every member pixel is < ink_level <= 255, so the ink box IS the component's box: status 1
 *              cannot occur; status 2 and square_blank work as before.  Slanted strokes, a dot inside a "0" or a speck
 *              dropped by min_pixels no longer move a neighbour's ink box, scale and class.
 *   mask = 0   read_glyphs' crop rule: whatever lies inside the box is part of the record.
 *   line_order = 1   The components kept by min_pixels (before the cap), each with box (l, u, r, b) and first pixel f,
 *              are visited in ascending (u, f).  Each line has a band [top, bottom).  For a visited component of height
 *              h = b - u and each existing line, ov = min(b, bottom) - max(u, top); the component joins the line with
 *              the largest ov among the lines with 2 ov >= min(h, bottom - top), on a tie the line created first, and
 *              the band's bottom becomes max(bottom, b) (the top never moves, because of the visiting order).  If no
 *              line qualifies it opens a new line [u, b).  Lines are numbered in creation order (ascending top); inside
 *              a line the glyphs go in ascending (l, u, f); the output is line 0, then line 1, ...; the cap takes the
 *              first min(cap, total) in that order.  find->order is not used (it must still be 0 or 1).  More than
 *              BNN_MI355X_PAGE_MAX_LINE_COMPONENTS kept components are refused -- the one refusal that needs the
 *              labelling's answer, so it comes after the device has worked: raise min_pixels.  Known limit: a dot above a
 *              stem is a line of its own unless reach_y joins it to the stem.
 *   line_order = 0   find->order, as read_glyphs; every line[i] and gap[i] is 0, a word_gap above 0 is refused.
 *   word_gap   gap[i] = 1 iff word_gap > 0, glyph i is not the first of its line and l_i - max(r of the earlier glyphs of
 *              its line) >= word_gap; else 0.
 *   page:      NULL is {1, 1, 0}.
 *   line[i], gap[i]: of output glyph i; cap ints each, either may be NULL.
 * order_lines: host only, touches no GPU, any library: the line model on n boxes the caller has (boxes: n x 4, first: n
 *       ints, ties in (u, f) or (l, u, f) go by input index).  order[i] = the input index of output glyph i; line and gap
 *       may be NULL.  Returns 0, -1 + last_error (null pointers, a negative n or word_gap, an empty or inverted box, n
 *       above BNN_MI355X_PAGE_MAX_LINE_COMPONENTS).
 * page_to_mnist: records to the host (tests, display): min(cap, total) x 784 bytes, a status-2 glyph's record stays as
 *       the caller left it; *n_found = total; boxes: cap x 4; status (may be NULL): cap ints.  Returns 0, -1.
 * read_page: LFC only; the records stay in HBM and the LFC pass runs on them on the same stream.  Return convention,
 *       ownership, the two times and status as read_glyphs.  Under the mask: upload, enhance, label, collect, ONE host
 *       round trip (the component list down; descriptors, keys and tables up), the record kernel
 *       (csrc/page_kernels.hip), the pass -- no ink-box launch, no second round trip.  Without the mask: exactly
 *       read_glyphs' sequence on the ordered boxes; with page = {0, 0, 0} exactly read_glyphs.
 * Refused before anything touches the GPU: what read_glyphs refuses; a mask or line_order other than 0 / 1; a negative
 * word_gap; a word_gap without line_order.  last_find_usec covers these calls too. */
#define BNN_MI355X_PAGE_MAX_LINE_COMPONENTS 65536
typedef struct {
  int mask, line_order, word_gap;
} bnn_mi355x_page_opts;
int bnn_mi355x_order_lines(const int *boxes, const int *first, int n, int word_gap, int *order, int *line, int *gap);
int bnn_mi355x_page_to_mnist(const uint8_t *pixels, int width, int height, int bands, long row_stride,
                             const bnn_mi355x_glyph_opts *opts, const bnn_mi355x_find_opts *find,
                             const bnn_mi355x_page_opts *page, int cap, int *n_found, int *boxes, uint8_t *records, int *status,
                             int *line, int *gap);
int *bnn_mi355x_read_page(const uint8_t *pixels, int width, int height, int bands, long row_stride,
                          const bnn_mi355x_glyph_opts *opts, const bnn_mi355x_find_opts *find,
                          const bnn_mi355x_page_opts *page, int number_class, int cap, int *n_found, int *boxes, int *line,
                          int *gap, float *usecPerImage, float *usecPreprocess, int *status);

/* Test hook: run the stages 0..stage on n host images (n <= 32768) and copy that stage's output,
 * exactly as it sits in HBM (bit-packed activation layout), to dst.  CNV: stage L =
 * layer L (0..7, after the max-pool where there is one); LFC: stage 0 = binarised input, stage
 * L+1 = layer L (L <= 2).  Returns the bytes per image, or -1. */
long bnn_mi355x_debug_stage_output(const uint8_t *images, int n_images, int stage, void *dst, size_t cap);

/* Per-stage device timing with HIP events on the stream the kernels run on
 * (used by bench.py for the roofline line).  profile(1) makes every later
 * inference call bracket each stage with events; profile_read waits for them,
 * writes the SUM of each stage's milliseconds over all chunks enqueued since
 * the last read (n_chunks of them) and returns the number of stages, or -1. */
int bnn_mi355x_profile(int enable);
int bnn_mi355x_profile_read(float *ms_per_stage, int cap, int *n_chunks);
const char *bnn_mi355x_stage_name(int stage);

#ifdef __cplusplus
}
#endif
#endif
