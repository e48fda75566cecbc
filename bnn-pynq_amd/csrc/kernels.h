// kernels.h -- launch interface of kernels.hip (host side).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "topology.h"

namespace bnn {

struct CnvLaunch {
  const uint8_t *images;      // device, n x 3072 bytes, planar CHW uint8 (CIFAR-10 record bodies)
  int n;
  void *buf0, *buf1;          // device ping-pong activation buffers (cnv_workspace_bytes per image)
  const uint32_t *rows[9];    // device, per-layer packed rows (packed_params.h)
  const uint8_t *l0_mfma;     // device, layer-0 MFMA table (packed_params.h); null: integer-pipe k_conv0
  const uint8_t *l1_mfma;     // device, cnvW1A1 layer 1 as FP4 MFMA operands (l1_mfma_table); null: the XNOR-popcount kernel.
                              // Side experiment only (BNN_MI355X_L1=mfma): never the default path.
  const uint8_t *conv_mfma;   // device, layers 1-7 as FP4 MFMA operands (cnvW1A1: conv_mfma_table, the 2-bit nets:
                              // conv_mfma_a2_table); null: the XNOR-popcount kernels only (BNN_MI355X_CONV=valu, and the
                              // fault-injection paths)
  bool l1_literal;            // cnvW1A1, BNN_MI355X_L1=lds: layer 1 in the north-star's literal formulation (comparison figure only)
  bool has_two;               // cnvW2A2: some row holds a weight of -2 (fault injection): the -2-aware kernel variants
  int16_t *scores;            // device, n x 64, may be null
  int32_t *classes;           // device, n, may be null
  int number_class;
  hipStream_t stream;
  hipEvent_t *events;         // optional: kCnvStages+1 events, recorded around every stage
  int last_stage;             // run stages 0..last_stage only (debug / per-layer tests); kCnvStages-1 = all
  hipEvent_t t0, t1;          // optional (both or neither): the batch's device time is t0 -> t1 (see LfcLaunch)
  // optional, n == 1 only (one image: the last launch is one block): a word in pinned host memory that the last kernel
  // sets to done_seq behind its results -- the host spins on it; no t0 / t1 packets are queued then
  unsigned *done_flag;
  unsigned done_seq;
  // run stages first_stage..last_stage only: stage k > 0 reads stage k-1's output where the full pass leaves it
  // (stage_output_bytes).  The dense scan (scan_kernels.h) enters at stage 6, on the layer-5 map of a whole picture.
  int first_stage = 0;
};

struct LfcLaunch {
  const uint8_t *images;      // device, n x 784 bytes -- or, `packed`, n x 13 binarised words (csrc/pack_inputs.h), 8-byte aligned
  bool packed;
  int n;
  void *buf0, *buf1;
  const uint32_t *rows[4];
  uint64_t *words;            // device, n raw output words (required)
  int32_t *classes;           // device, n, may be null
  int number_class;
  hipStream_t stream;
  hipEvent_t *events;         // optional: kLfcStages+1 events
  int last_stage;             // run stages 0..last_stage only; kLfcStages-1 = all
  // optional (both or neither): the batch's device time is t0 -> t1.  Several launches: events recorded in front of
  // the first and behind the last.  ONE launch (k_lfc_fused*, k_lfc_block_s): the dispatch's own start / end
  // timestamps (hipExtLaunchKernelGGL) -- what a kernel trace reports for it -- instead of two more packets around
  // it, whose processing would be booked as compute (3.5 us on a 7 us kernel).
  hipEvent_t t0, t1;
  // t0 / t1 may be bound to the one dispatch (above).  Only for a call that is ONE chunk: hipEventElapsedTime between
  // such events of DIFFERENT dispatches is not an interval a multi-chunk call could place its chunks by; those get
  // ordinary recorded events around the launch.
  bool t_dispatch;
  unsigned *done_flag;        // as CnvLaunch::done_flag (n == 1: the one-block form of k_lfc_fused*)
  unsigned done_seq;
};

// layer-0 MFMA table (packed_params.h): the tile-form operands sit behind the pixel-form ones
constexpr int kL0TileOffset = 2 * 64 * 32, kL0BigBytes = 2 * 32 * 2 * 16;

constexpr int kCnvStages = 9;  // conv0, L1..L7, L8+decode
constexpr int kLfcStages = 6;  // binarize, L0..L3, decode
const char *stage_name(bool is_cnv, int stage);

size_t stage_output_bytes(bool is_cnv, int abits, int stage, int *in_buf1);
void cnv_workspace_bytes(int abits, size_t *buf0, size_t *buf1);
void lfc_workspace_bytes(int abits, size_t *buf0, size_t *buf1);

// cnvW1A1 layer 1 for the matrix pipe (side experiment): A operands of v_mfma_scale_f32_32x32x64_f8f6f4 with
// FP4 (E2M1) weights -- +1 = 0x2, -1 = 0xA -- [tap 0..8][neuron tile 0..1][lane 0..63][16 bytes], lane (r, h)
// holding channels 32h..32h+31 of neuron 32*tile + r; then the accumulator seeds [tile][h][16] floats
// -(theta + 1) with theta = 576 - 2 * t the threshold on the signed sum (the row's t is the XNOR form's
// "mismatches < t").  rows: layer 1 of the packed blob (host pointer).  Returns the table's bytes.
constexpr size_t kL1MfmaWeights = 9 * 2 * 64 * 16, kL1MfmaBytes = kL1MfmaWeights + 2 * 2 * 16 * 4;
void l1_mfma_table(const uint32_t *rows, uint8_t *dst);

// cnvW1A1 layers 1-3 for the matrix pipe (the throughput path from conv_mfma_min() images on): one table
// per layer, each [k step][neuron tile][lane 0..63][16 bytes] of FP4 weights (k step = tap * (Cin / 64) + 64-channel
// block; lane (r, h) holds channels 32h..32h+31 of the step for neuron 32 * tile + r), then the seeds [tile][h][16]
// floats -(theta + 1).  Layer 1's table is laid out as l1_mfma_table's.  Made on the device from the packed rows.
constexpr size_t kConvMfmaL2Off = kL1MfmaBytes, kConvMfmaL3Off = kConvMfmaL2Off + 9 * 4 * 64 * 16 + 4 * 32 * 4,
                 kTailMfmaL4Off = kConvMfmaL3Off + 18 * 4 * 64 * 16 + 4 * 32 * 4;
// ... and layers 4-7 (k_tail_mfma, from tail_mfma_min() images on) behind them, in the same form: k step = the layer's ks-th
// 64 inputs (layer 4: tap * 2 + 64-channel block; layers 5-7: the image's ks-th 64 bits), 8 / 8 / 16 / 16 neuron tiles
constexpr size_t kTailMfmaL5Off = kTailMfmaL4Off + 18 * 8 * 64 * 16 + 8 * 32 * 4, kTailMfmaL6Off = kTailMfmaL5Off + 36 * 8 * 64 * 16 + 8 * 32 * 4,
                 kTailMfmaL7Off = kTailMfmaL6Off + 4 * 16 * 64 * 16 + 16 * 32 * 4, kConvMfmaBytes = kTailMfmaL7Off + 8 * 16 * 64 * 16 + 16 * 32 * 4;
// rows: device pointers to cnvW1A1's packed layers (rows[1..7] are read); enqueued on s
hipError_t conv_mfma_table(const uint32_t *const rows[9], uint8_t *dst, hipStream_t s);

// The same for cnvW1A2 and cnvW2A2 (k_conv_mfma_a2): per layer the weights [k step][neuron tile][lane][16 bytes] (FP4 -1, 0,
// +1, and -2 where cnvW2A2's row marks it), then the seeds [tile][h][16] floats -(t0 + 1/2), then [tile][h][16] floats t1 - t0.
constexpr size_t kConvMfmaA2L2Off = 9 * 2 * 64 * 16 + 2 * 64 * 4, kConvMfmaA2L3Off = kConvMfmaA2L2Off + 9 * 4 * 64 * 16 + 4 * 64 * 4,
                 kTailMfmaA2L4Off = kConvMfmaA2L3Off + 18 * 4 * 64 * 16 + 4 * 64 * 4;
constexpr size_t kTailMfmaA2L5Off = kTailMfmaA2L4Off + 18 * 8 * 64 * 16 + 8 * 64 * 4, kTailMfmaA2L6Off = kTailMfmaA2L5Off + 36 * 8 * 64 * 16 + 8 * 64 * 4,
                 kTailMfmaA2L7Off = kTailMfmaA2L6Off + 4 * 16 * 64 * 16 + 16 * 64 * 4, kConvMfmaA2Bytes = kTailMfmaA2L7Off + 8 * 16 * 64 * 16 + 16 * 64 * 4;
// rows: device pointers to the net's packed layers (rows[1..7] are read: AR_TB rows for cnvW1A2, AR_TT for cnvW2A2)
hipError_t conv_mfma_a2_table(NetId net, const uint32_t *const rows[9], uint8_t *dst, hipStream_t s);

// bit k set: stage k of run_cnv(net, a) runs on the matrix pipe (layer 0's MFMA forms count).  Decided by the code that
// run_cnv itself decides with; nothing is launched.
int cnv_matrix_stages(NetId net, const CnvLaunch &a);

// enqueue all stages of one batch on a.stream; returns the launch error, if any
hipError_t run_cnv(NetId net, const CnvLaunch &a);
hipError_t run_lfc(NetId net, const LfcLaunch &a);

// Many fault campaigns side by side (bnn_mi355x_fault_campaigns).  Run r has its own copy of the blob in HBM,
// `stride` bytes behind run r-1's.  One multi-run launch classifies a SEGMENT of images per record: `len`
// resident images from `image` on, with run `run`'s parameters, their activations at slots slot..slot+len-1 of
// the activation buffers; results land at run * n + image.  The stage kernels' MULTI instantiations take the
// record from blockIdx.y.
struct MultiSeg { int run, image, slot, len; };
struct MultiLaunch {
  const uint8_t *images;      // device, the call's resident images (every run classifies the same ones)
  const MultiSeg *segs;       // device, this launch's records (at most 65 535)
  int nsegs, max_len, total;  // records; the longest segment; images over all of them (<= the workspace's capacity)
  int n;                      // images per run
  void *buf0, *buf1;          // activation buffers (cnv/lfc_workspace_bytes per image, `total` images)
  const uint32_t *rows[9];    // run 0's copy: per-layer packed rows
  const uint8_t *l0_mfma;     // run 0's copy: layer-0 MFMA table (CNV); null: integer-pipe k_conv0
  size_t stride;              // bytes between two runs' copies (a multiple of 256)
  bool has_two;               // cnvW2A2: some run's copy holds a weight of -2 (the -2-aware instantiations)
  int32_t *classes;           // CNV: device, class per image of every run (run-major)
  uint64_t *words;            // LFC: device, raw output word per image of every run (run-major)
  int number_class;
  hipStream_t stream;
  // run the stages of layers first..last only (bnn_mi355x_fault_sweep); layer l's stage reads layer l-1's output where
  // the full pass leaves it (stage_output_bytes).  LFC: layer 0's stage includes the binariser.
  int first = 0, last = 1 << 30;
};
hipError_t run_cnv_multi(NetId net, const MultiLaunch &a);
hipError_t run_lfc_multi(NetId net, const MultiLaunch &a);

// copy `bytes` from staging + src to copies + dst for each span (one block per span); offsets and sizes are multiples of 4
struct PatchSpan { uint64_t dst; uint32_t src, bytes; };
hipError_t scatter_patches(const uint8_t *staging, const PatchSpan *spans, int nspans, uint8_t *copies, hipStream_t s);

// Single-fault sweeps (bnn_mi355x_fault_sweep).  Row (q, j) of a broadcast, j < rows: dst + q * dst_run_stride +
// j * row_bytes <- src + j * row_bytes, for q < runs (row_bytes a multiple of 4).
hipError_t sweep_broadcast(const uint8_t *src, size_t row_bytes, int rows, int runs, uint8_t *dst, size_t dst_run_stride,
                           hipStream_t s);
// alive[slot] = 1 for every image of the records whose `row_bytes` (a multiple of 16) at act + slot * row_bytes differ
// from base + image * row_bytes; other entries are left as they are.  One wave per image.
hipError_t sweep_mark(const uint8_t *act, const uint8_t *base, int row_bytes, const MultiSeg *segs, int nsegs, int max_len,
                      uint8_t *alive, hipStream_t s);
// sweep_mark that also counts (bnn_mi355x_sweep_profile): `alive` as above, and for every record counts[2 * run] += its
// images that differ, counts[2 * run + 1] += the activations that differ in them -- differing bits of a 1-bit map,
// channels whose (sign, non-zero) pair differs of a `two_bit` one (16-byte units of 64 channels).  The caller zeroes counts.
hipError_t sweep_profile(const uint8_t *act, const uint8_t *base, int row_bytes, bool two_bit, const MultiSeg *segs, int nsegs, int max_len,
                         uint8_t *alive, unsigned long long *counts, hipStream_t s);
// run q < runs: counts[q] = #{j < win : classes[q * n + j] != base[j]}.  sweep_emit: the pairs {j, classes[q * n + j]} of
// those images to out + 2 * offsets[q] ..., in image order (counts as sweep_count left them).
hipError_t sweep_count(const int32_t *classes, const int32_t *base, int n, int win, int runs, int *counts, hipStream_t s);
hipError_t sweep_emit(const int32_t *classes, const int32_t *base, int n, int win, int runs, const int *counts, const long long *offsets,
                      int *out, hipStream_t s);

// Activation-fault sweeps (bnn_mi355x_act_fault_sweep).  The site of run q: in the 16-byte unit `unit` of an output
// row, activation bit `bit` (0..127 of the unit's four dwords: 1-bit maps; 0..63 of the (sign, non-zero) u64 pair:
// 2-bit maps) -- its level index i becomes (i + shift) mod levels.
struct ActPatch { uint32_t unit, bit, shift, pad; };
// For every record: act + (slot + j) * row_bytes <- base + (image + j) * row_bytes with run `run`'s site changed,
// j < len (all records of a launch as long as max_len or shorter; row_bytes a multiple of 16).
hipError_t act_seed(const uint8_t *base, int row_bytes, bool two_bit, const MultiSeg *segs, int nsegs, int max_len, const ActPatch *patches,
                    uint8_t *act, hipStream_t s);

// The layer right after an activation site, evaluated only inside the window the site reaches (CNV, `layer` = the
// site's layer + 1 = 1, 2 or 3).  Run q's site: pixel (y, x) of the layer-(layer-1) map, channel 64 * word + bit, level
// index i -> (i + shift) mod levels.  `base`: the fault-free output rows of layer-1 of ALL the call's images (image i at
// i * row bytes, 16-byte aligned).  For every record and j < len the launch recomputes, from base's rows of image
// `image + j` with the site changed in registers, the act_window_pixels(layer) output pixels of slot `slot + j` the site
// can reach (9 conv pixels; pooled layers: the up to 2 x 2 pooled pixels = 16 conv pixels) and overwrites those words
// of the slot's row in the layer's output buffer (where run_cnv_multi leaves it); the rest of the row -- the
// fault-free output, put there by sweep_broadcast -- is left as it is.  Of `a`: segs, nsegs, max_len, total, buf0,
// buf1, rows, stride and stream are read (cnvW2A2's window kernels are -2-aware whether or not a row holds a -2).
struct ActWinSite { int y, x, word, bit, shift, pad[3]; };
int act_window_pixels(int layer);
hipError_t act_window(NetId net, int layer, const MultiLaunch &a, const uint8_t *base, const ActWinSite *sites);

// Random activation upsets (bnn_mi355x_act_noise_campaigns).  In place on the `row_bytes` per image of a layer's packed
// output at act + (slot + j) * row_bytes, j < len, for every record: each site upset where act_noise_block (act_faults.h)
// of (seeds[run], image + j, layer, site) says so for `rate_q32`; counts[run * nlayers + layer] += the sites upset.
// Nothing is launched for rate 0.
hipError_t act_noise(uint8_t *act, int row_bytes, bool two_bit, const MultiSeg *segs, int nsegs, int max_len, const unsigned long long *seeds,
                     int layer, uint32_t rate_q32, unsigned long long *counts, int nlayers, hipStream_t s);

// Input-buffer faults (bnn_mi355x_input_fault_sweep, bnn_mi355x_input_noise_campaigns): faulted copies of the call's
// resident images (`image_bytes` each, a multiple of 16; both pointers 16-byte aligned) in a staging buffer that the
// stages then read as images.
// input_seed: for every record, staged + (slot + j) * image_bytes <- images + (image + j) * image_bytes with run `run`'s
// bit flipped, j < len: patch.unit the 16-byte lane of the image, patch.bit 0..127 inside it (shift is not read).
hipError_t input_seed(const uint8_t *images, int image_bytes, const MultiSeg *segs, int nsegs, int max_len, const ActPatch *patches,
                      uint8_t *staged, hipStream_t s);
// input_noise: pair p = pair0 + k, k < npairs, is run p / n on image p % n; staged + k * image_bytes <- that image with
// every bit flipped where act_noise_block of (seeds[run], image, kInputNoiseTag, site) says so for `rate_q32`
// (input_faults.h); counts[run] += the bits flipped.  Nothing is launched for rate 0.
hipError_t input_noise(const uint8_t *images, int image_bytes, unsigned long long pair0, int npairs, int n, const unsigned long long *seeds,
                       uint32_t rate_q32, unsigned long long *counts, uint8_t *staged, hipStream_t s);

// Random upsets of the parameter memories (bnn_mi355x_mem_noise_campaigns; the model: mem_faults.h).  All three work in
// place on `runs` copies of the blob, run q at copies + q * stride (a multiple of 256), on one layer whose weight
// elements are not int8 and whose threshold elements are 16 bits wide: `offset` ... `kw` as the blob's header has them,
// `pe` / `tmem` the layer's fold (row n lies in PE n % pe, at fold n / pe), `layer` its index.  Nothing is launched
// for rate 0.  counts: [run][nlayers][2: weights, thresholds], += the sites flipped.
struct MemNoiseLayer { uint32_t offset, row_dwords, rows, kw, pe, tmem, layer; };
// weights: every site of the layer's rows flipped where the draw of (seeds[run], layer, 0, site) says so; two_bit: AR_TT
// rows (three planes and a flag dword, set where a word now holds a -2)
hipError_t mem_noise_w(uint8_t *copies, size_t stride, int runs, const unsigned long long *seeds, const MemNoiseLayer &L, bool two_bit,
                       uint32_t rate_q32, unsigned long long *counts, int nlayers, hipStream_t s);
// AR_TT rows: every row's flag dword recomputed from its "weight is -2" plane (a flip can also remove a -2)
hipError_t mem_noise_flags(uint8_t *copies, size_t stride, int runs, const MemNoiseLayer &L, hipStream_t s);
// thresholds: raw[n * nthr + i] is the low 16 bits of neuron n's i-th threshold word in the loaded memories (device)
hipError_t mem_noise_t(uint8_t *copies, size_t stride, int runs, const unsigned long long *seeds, const MemNoiseLayer &L, int nthr, Arith arith,
                       bool signed_bb, const uint16_t *raw, uint32_t rate_q32, unsigned long long *counts, int nlayers, hipStream_t s);

// The upsets of a memory organisation, with bursts, over epochs (bnn_mi355x_hardened_mem_noise_campaigns and the
// *_exposure_* entry points; the model: mem_org.h), scheme 0 with burst 1 included: the events of `epoch` (bursts of `burst`
// physical bits) XORed onto the state the earlier epochs left in the copies; a one-shot campaign is epoch 0 on zeroed
// state.  counts: this epoch's [nlayers][2: weights, thresholds][2] entries of run 0 (zeroed by the caller), run q's
// `run_stride` longs behind: [0] += the physical bits flipped in this epoch (before voting), [1] += the logical bits that
// differ from the loaded parameters after it (after voting and de-interleaving), over all of the memory.
// weights of a layer >= 1 (one module, not interleaved): ebits = SIMD * wbits bits per memory word (a divisor of 64);
// `loaded` the loaded blob in HBM (8-byte aligned), compared word for word at the copy's offsets
hipError_t xmem_noise_w(uint8_t *copies, size_t stride, int runs, const unsigned long long *seeds, const MemNoiseLayer &L, bool two_bit,
                        int ebits, int burst, uint32_t rate_q32, int epoch, const uint8_t *loaded, unsigned long long *counts, size_t run_stride,
                        hipStream_t s);
// 16-bit thresholds: `modules` 1 or 3 (bitwise majority), `interleave` 0, 2 or 3; raw as for mem_noise_t; state holds
// runs * rows * nthr words (run-major, lane n * nthr + i), the accumulated hit masks of the modules, 16 bits each; zero
// where the copies hold the loaded parameters
hipError_t xmem_noise_t(uint8_t *copies, size_t stride, int runs, const unsigned long long *seeds, const MemNoiseLayer &L, int nthr, Arith arith,
                        bool signed_bb, const uint16_t *raw, int modules, int interleave, int burst, uint32_t rate_q32, int epoch,
                        unsigned long long *state, unsigned long long *counts, size_t run_stride, hipStream_t s);
// 16-bit thresholds of a coded layer (SEC-DED: ecc.h), in xmem_noise_t's place: a state word holds the accumulated hit
// masks of the element's 16 data bits (low 16) and 6 check bits (bits 16 ... 21); interleave 0 or 2.  ecc: this epoch's
// [layer][2: words with decode status 1, 2] of run 0, run q's ecc_stride longs behind
hipError_t emem_noise_t(uint8_t *copies, size_t stride, int runs, const unsigned long long *seeds, const MemNoiseLayer &L, int nthr, Arith arith,
                        bool signed_bb, const uint16_t *raw, int interleave, int burst, uint32_t rate_q32, int epoch, unsigned long long *state,
                        unsigned long long *counts, size_t run_stride, unsigned long long *ecc, size_t ecc_stride, hipStream_t s);

// The repair scrub of the exposure campaigns (bnn_mi355x_repair_exposure_campaigns; the model: mem_org.h, "repair
// scrubs"): ONE launch rewrites the state words of every layer that has redundancy, in place of a full rewrite's copy and
// memset.  An entry per such layer: its state words (xmem_noise_t's or emem_noise_t's: runs * lanes of them) at
// camp + state_off (8-byte aligned), lanes = rows * nthr, kind, and the layer's index for the counters.  TMR: the three
// 16-bit hit masks become their bitwise majority; coded: (data mask, check mask) becomes ecc_repair's.  rep: this epoch's
// [layer][2: words rewritten, words whose state still differs from the loaded one] of run 0, run q's rep_stride longs
// behind.  The copies are not touched: a repair does not change the delivered parameters.
enum : uint32_t { RK_SKIP = 0, RK_TMR = 1, RK_CODED = 2 };
constexpr int kRepairEntries = 9;
struct RepairEntry { unsigned long long state_off; uint32_t lanes, kind, layer, depth; };  // (depth: iwrepair_state's alone, else 0)
struct RepairTable { RepairEntry e[kRepairEntries]; };
hipError_t repair_state(uint8_t *camp, const RepairTable &tab, int entries, int runs, unsigned long long *rep, size_t rep_stride, hipStream_t s);

// Coded weight memories (SEC-DED (72,64): wecc.h; bnn_mi355x_wecc_exposure_campaigns; the model: mem_org.h, "coded weight
// memories"), wecc_kernels.hip.  wmem_noise_w goes in xmem_noise_w's place for a coded layer, same geometry and
// arguments; state holds runs * rows * kw * (two_bit ? 2 : 1) code words (run-major, lane-major, a lane's code words
// one after the other), each a pair of longs: the accumulated hit mask of the 64 data sites, and of the 8 check bits;
// zero where the copies hold the loaded parameters.  counts[0] += the data and check bits flipped, [1] += the data bits
// that differ after decoding.  wst: this epoch's [layer][4: code words at status 1, at status 2, rewritten by the
// epoch's repair, still unlike the loaded ones after it] of run 0, run q's wst_stride longs behind.
hipError_t wmem_noise_w(uint8_t *copies, size_t stride, int runs, const unsigned long long *seeds, const MemNoiseLayer &L, bool two_bit,
                        int ebits, int burst, uint32_t rate_q32, int epoch, const uint8_t *loaded, unsigned long long *state,
                        unsigned long long *counts, size_t run_stride, unsigned long long *wst, size_t wst_stride, hipStream_t s);
// The repair of the coded weight memories: ONE launch over (code word, run, coded layer) applies wecc_repair to the state
// pairs; entries as for repair_state (state_off the layer's pairs, lanes its code words per run; kind RK_CODED).  The
// copies are not touched.
hipError_t wrepair_state(uint8_t *camp, const RepairTable &tab, int entries, int runs, unsigned long long *wst, size_t wst_stride, hipStream_t s);

// Column-interleaved coded weight memories (bnn_mi355x_iwecc_exposure_campaigns; the model: mem_org.h, "column-interleaved
// code words"), iwecc_kernels.hip.  iwmem_noise_w goes in wmem_noise_w's place for a layer of interleave depth `depth`
// (1, 2, 4, 8 or 16; 1: the same result as wmem_noise_w): same arguments, same state size and place, but a lane per CODE
// WORD'S WORTH of storage numbered in SITE order (lane q: sites [64 q, 64 q + 64) and check element q), and a state pair
// means the accumulated PHYSICAL hit masks of those 64 sites and that check element; the depth adjacent lanes of a group
// exchange them into code word patterns, decode, and exchange the remaining errors back.  The code words per run must be
// a multiple of 64 (a wave is whole or absent): hipErrorInvalidValue otherwise.  counts and wst as for wmem_noise_w, the
// status counters per code word after gathering.
hipError_t iwmem_noise_w(uint8_t *copies, size_t stride, int runs, const unsigned long long *seeds, const MemNoiseLayer &L, bool two_bit,
                         int ebits, int burst, int depth, uint32_t rate_q32, int epoch, const uint8_t *loaded, unsigned long long *state,
                         unsigned long long *counts, size_t run_stride, unsigned long long *wst, size_t wst_stride, hipStream_t s);
// The repair of interleaved coded weight memories, in wrepair_state's place (not next to it): entries as there, with the
// layer's depth in RepairEntry::depth and lanes a multiple of 64.
hipError_t iwrepair_state(uint8_t *camp, const RepairTable &tab, int entries, int runs, unsigned long long *wst, size_t wst_stride, hipStream_t s);

}  // namespace bnn
