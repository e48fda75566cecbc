// mem_org.h -- how the fork's hardened overlays ORGANISE their parameter memories, and upsets of that physical state
// (bnn_mi355x_hardened_mem_noise_campaigns).
//
// Schemes: 0 none, 1 TMR, 2 interleaved, 3 resilient-interleaved.  The storage side is the reference's host code,
// restated here as tables: the module counts of FINNTopology in the variants' main_python.cpp, the interleaved memories
// and their patterns of FoldedMVLoadInterleavedLayerMem / InterleavedLoadArgs / interleave.h.
//   TMR           three modules for the weight memory of layer 0 and for the threshold memories of layers 0-4; every
//                 other memory has one.
//   interleaved   the threshold memory of every layer that has one; weights are not interleaved.  Lines ind (even) and
//                 ind + 1 of one PE, same threshold index, form a pair.  With T the element width (24: layer 0, else 16)
//                 position q in [0, 2T) of the pair holds e1's bit o1[popcount(pattern[0..q))] where pattern[q] is set
//                 (e1 = line ind), else e2's bit o2[q - popcount(pattern[0..q))] (e2 = line ind + 1).  Line ind stores
//                 positions T ... 2T-1, line ind + 1 positions 0 ... T-1.  An odd last line is stored as is.
//                 Scheme 2: pattern 0x5555..., both orders the identity.  Scheme 3: the patterns below, o1 the identity,
//                 o2 reversed.
// Supported: cnvW1A1 and cnvW1A2 with schemes 1, 2, 3; cnvW2A2 with 1 and 3.  Refused: cnvW2A2 with scheme 2 (the
// reference interleaves its WEIGHTS with the default pattern bitset<2W>(0x5555555555555555), which for W = 64 covers 64
// of the 128 positions; its loader then reads past the end of e2: there is no defined layout to model) and every LFC
// network (the one LFC overlay interleaves layer 0 with a 24-bit element into ap_int<16> words; what its hardware
// makes of that is in an hlslib fork the reference tree does not hold).  Scheme 0 is every network's.
//
// The PHYSICAL state is what FoldedMVMemSet is handed at load: interleaved words, one copy per module.  A physical fault
// is a fault record plus a module: apply_fault's read-modify-write on that module's physical word, the layer-0
// integer-part quirk included, as is.  The LOGICAL parameters the network computes with are
//     de-interleave(vote(modules)).
// The de-interleaver is the inverse permutation: it is forced, a fault-free hardened overlay computes the base network.
// The voter is the project's own choice, the reference's being in the absent fork: the BITWISE MAJORITY of the low
// `ebits` of the three stored words.  Any voter agrees with it while at most one module of a word is hit; with two
// modules hit (the same bit or not) voters could differ, and results for such words are this model's, not the fork's.
//
// The upset model (parameters: a rate per layer and target, a burst width b = 1 ... 16): an EVENT flips b adjacent
// physical bits of one element of one module -- the aligned group g of enumerate_faults(L, target, word_size b), per =
// ceil(ebits / b) groups per element, the last one clipped to the element.  With `element` numbered as in mem_faults.h,
//     e = element * per + g
//     u = philox4x32_10(counter {L, target | m << 1 | (b - 1) << 8, e >> 2, 1}, key {seed})[e & 3];  event iff u < rate
// for module m.  Module 0 with b = 1 is mem_faults.h's draw and site numbering.  Events apply layer-major, per layer
// weights then thresholds, module-major, in event order.
#pragma once
#include <stdint.h>

#include <string>

#include "faults.h"
#include "packed_params.h"
#include "topology.h"

#ifndef BNN_HD
#define BNN_HD
#endif

namespace bnn {

enum : int { HS_NONE = 0, HS_TMR = 1, HS_INTERLEAVED = 2, HS_RESILIENT = 3 };
constexpr int kMaxBurst = 16;

struct MemOrg { int w_modules, t_modules, t_interleave; };  // t_interleave: 0, 2 or 3

// "" and the organisation of one layer's memories, else why this (network, scheme, layer) is refused
std::string hardening_layout(const NetSpec &net, int scheme, int layer, MemOrg &out);
// the scheme an overlay's name implies: 0 for a base network
int hardening_scheme_of(const char *name);

// the interleave pattern of a pair of T-bit elements (bit q set: position q holds a bit of e1)
BNN_HD inline uint64_t interleave_pattern(int il, int T) {
  if (il == HS_INTERLEAVED) return 0x5555555555555555ull & ((1ull << (2 * T)) - 1);
  return T == 24 ? 0x888AAAAAAEEEull : 0x88AAAAEEull;
}

// The word_size-b fault counter word of the draw above.
BNN_HD inline uint32_t hardened_draw_word(int target, int module, int burst) {
  return (uint32_t)target | (uint32_t)module << 1 | (uint32_t)(burst - 1) << 8;
}

// Logical -> physical: bit `bit` of the T-bit element in line `ind` (of `lines` lines of one PE) is stored in line
// *p_ind at bit *p_bit.  il 0: the identity.  Shared by the host model and the kernel (k_hmem_noise_t).
BNN_HD inline void interleave_site(int il, int T, int lines, int ind, int bit, int *p_ind, int *p_bit) {
  const int a = ind & ~1;
  if (il == 0 || a + 1 >= lines) {
    *p_ind = ind;
    *p_bit = bit;
    return;
  }
  const uint64_t pat = interleave_pattern(il, T);
  // the rank among e1's (set) or e2's (clear) positions: o1 the identity; o2 the identity (2) or reversed (3)
  const bool first = ind == a;
  int rank = first || il == HS_INTERLEAVED ? bit : T - 1 - bit, q = 0;
  for (; q < 2 * T - 1; q++)  // (bounded: a bit outside the element ends at the last position)
    if ((((pat >> q) & 1) != 0) == first && rank-- == 0) break;
  *p_ind = q >= T ? a : a + 1;
  *p_bit = q >= T ? q - T : q;
}

// Physical -> logical, the inverse: the bit stored in line p_ind at p_bit is bit *bit of line *ind's element.
BNN_HD inline void interleave_source(int il, int T, int lines, int p_ind, int p_bit, int *ind, int *bit) {
  const int a = p_ind & ~1;
  if (il == 0 || a + 1 >= lines) {
    *ind = p_ind;
    *bit = p_bit;
    return;
  }
  const uint64_t pat = interleave_pattern(il, T);
  const int q = p_ind == a ? T + p_bit : p_bit;
  const int ones = __builtin_popcountll(pat & ((1ull << q) - 1));
  if ((pat >> q) & 1) {
    *ind = a;
    *bit = ones;
  } else {
    *ind = a + 1;
    *bit = il == HS_INTERLEAVED ? q - ones : T - 1 - (q - ones);
  }
}

// ---- exposure campaigns (bnn_mi355x_exposure_campaigns): upsets that accumulate, with scrubbing ---------------------------
// A run over n images is cut into EPOCHS of `epoch_images` images: epoch t holds images [t * epoch_images,
// min(n, (t + 1) * epoch_images)), the last one may be short, E = ceil(n / epoch_images) <= kMaxEpochs.  Rates are per
// epoch.  The events of epoch t are the draw above with the epoch in the fourth counter word,
//     u = philox4x32_10(counter {L, target | m << 1 | (b - 1) << 8, e >> 2, 1 + (t << 8)}, key {seed})[e & 3],
// so t = 0 is hardened_mem_noise_mask's draw, and the low byte 1 still keeps the stream apart from the activation and
// input draws (0 there).  An epoch's upsets XOR onto whatever the PHYSICAL state holds, before the epoch's images are
// classified; the order inside an epoch is the one above, across epochs epoch-major (it matters for the layer-0
// integer-part quirk of apply_fault alone).  scrub_every = S > 0: before the upsets of every epoch t > 0 with t % S == 0
// all physical memories return to the loaded parameters (a full rewrite; a voter-driven repair is not modelled); S = 0
// never.  The logical parameters of an epoch are de-interleave(vote(modules)) of the state.  On the host: the blob of
// (run, epoch t) is pack_params_hardened of the masks of epochs (last scrub epoch <= t) ... t, concatenated.
// The epoch granularity, the full-rewrite scrub and the voter are the project's own choices: parity unpinned.
constexpr int kMaxEpochs = 1 << 16;  // (the epoch shares its counter word with the tag byte: below 2^24)
BNN_HD inline uint32_t exposure_tag(uint32_t epoch) { return 1u + (epoch << 8); }  // (kMemNoiseTag in the low byte)
// the last epoch <= t whose upsets met freshly written memories
inline int exposure_first_epoch(int t, int scrub_every) { return scrub_every > 0 ? t - t % scrub_every : 0; }

// ---- host only from here ---------------------------------------------------------------------------------------------

struct PhysFault { Fault f; int module; };

// The physical memories of layers [l0, l1): mod[m] holds module m's words in RawParams' own shape (a memory with one
// module lives in mod[0]; threshold words are the interleaved ones).
struct PhysParams {
  int l0 = 0, l1 = 0;
  RawParams mod[3];
};
// what the loader stores from the parameter files
void phys_load(const NetSpec &net, int scheme, const RawParams &raw, int l0, int l1, PhysParams &out);
// one physical fault; returns apply_fault's result, -1 also for a module the memory does not have
int phys_apply(const NetSpec &net, int scheme, PhysParams &p, const PhysFault &pf);
// de-interleave(vote(modules)) into out.w[l], out.t[l] for l in [l0, l1).  A memory with one module and no interleave
// is copied word for word; a voted or de-interleaved word holds its element's bits alone.
void phys_logical(const NetSpec &net, int scheme, const PhysParams &p, RawParams &out);

// element width in bits of a layer's weight (target 0) or threshold (target 1) memory; 0: no threshold memory
int mem_element_bits(const LayerSpec &L, int target);
// bits an event of group `bit / burst` flips: burst, less where the element ends
inline int event_width(int ebits, int burst, int bit) { return ebits - bit < burst ? ebits - bit : burst; }

// the events of one (run seed, layer, target, module) in event order as physical faults (image 0, word_size burst);
// returns their number (0: thresholds of a layer without any), -1 for a bad scheme, burst, layer, target or module;
// writes events first .. first + cap - 1 to out (which may be null).  epoch: the exposure campaigns' (above); the
// records' image field holds it
long hardened_mem_noise_mask(const NetSpec &net, int scheme, int burst, uint64_t run_seed, int layer, int target, int module,
                             uint32_t rate_q32, long first, PhysFault *out, long cap, int epoch = 0);

}  // namespace bnn
