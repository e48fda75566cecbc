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

#include "ecc.h"
#include "wecc.h"
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
// *p_ind at bit *p_bit.  il 0: the identity.  Shared by the host model and the kernels (k_xmem_noise_t, k_emem_noise_t).
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
// all physical memories return to the loaded parameters (a full rewrite; the repair that reads, votes or decodes and
// writes back: "repair scrubs" below); S = 0 never.  The logical parameters of an epoch are de-interleave(vote(modules)) of the state.  On the host: the blob of
// (run, epoch t) is pack_params_hardened of the masks of epochs (last scrub epoch <= t) ... t, concatenated.
// The epoch granularity, the full-rewrite scrub and the voter are the project's own choices: parity unpinned.
constexpr int kMaxEpochs = 1 << 16;  // (the epoch shares its counter word with the tag byte: below 2^24)
BNN_HD inline uint32_t exposure_tag(uint32_t epoch) { return 1u + (epoch << 8); }  // (kMemNoiseTag in the low byte)
// the last epoch <= t whose upsets met freshly written memories
inline int exposure_first_epoch(int t, int scrub_every) { return scrub_every > 0 ? t - t % scrub_every : 0; }

// ---- coded threshold memories (bnn_mi355x_ecc_exposure_campaigns): the code of ecc.h on top of a scheme -----------------
// `code` is 0 (none: everything above, unchanged) or 1 (SEC-DED).  Code 1 covers the 16-bit threshold memory of every
// layer that has one -- the memories the interleaved schemes cover; weights and the 24-bit thresholds of CNV layer 0 are
// not coded (ecc.h says why), and layer 0 keeps the uncoded host route.
// Storage: the 6 check bits of a threshold element live in a CHECK MEMORY of their own, of the same (PE, line,
// threshold) shape, addressed as module 1 of target 1 (the supported schemes give threshold memories one module).
// Scheme 0 stores element and check word as they are.  Scheme 2 encodes the LOGICAL element, then interleaves the data
// of lines ind, ind + 1 as above and their check words by the same construction at width 6 (interleave_site(2, 6, ...):
// pattern 0x555, line ind holds positions 6 ... 11, line ind + 1 positions 0 ... 5); an odd last line is stored as is.
// The logical parameters are decode(de-interleave(data), de-interleave(check)).
// Supported: code 1 with scheme 0 (every network) and with scheme 2 (where scheme 2 is supported).  Refused: code 1 with
// scheme 1 (TMR plus a code is not modelled) or 3 (the resilient patterns are defined for 32 and 48 positions only).
// Upsets: the data memories draw as above (module 0); the check memory draws by the same construction at element width
// 6 with module 1 in the counter word: per_c = ceil(6 / b) groups per element, e = element * per_c + g, an event a pure
// XOR of bits [g * b, min(g * b + b, 6)) of the check word, at the layer's threshold rate.  Bursts do not cross from
// the data memory into the check memory.  Order inside an epoch: module-major, data then check.
// Counts per (run, epoch, layer), six: the four above (thresholds: physical = data plus check bits flipped, logical = data
// bits that differ after decoding), then the threshold words whose decode status after the epoch is 1, and 2.
// The storage in a check memory of its own and the draw are the project's own choices.
BNN_HD inline uint32_t ecc_check_groups(int burst) { return (uint32_t)((kEccCheckBits + burst - 1) / burst); }

// ---- repair scrubs (bnn_mi355x_repair_exposure_campaigns): read, vote or decode, write back ---------------------------
// The full rewrite above needs the golden copy; a system that flies TMR or a code scrubs by reading a word, voting or
// decoding it and writing the result back.  repair_every = P >= 0 goes next to scrub_every = S: before the upsets of epoch
// t > 0 a full rewrite happens if S > 0 and t % S == 0 (as above, and then there is no repair in that epoch); otherwise a
// REPAIR happens if P > 0 and t % P == 0.  A repair visits every physical memory that has redundancy:
//   TMR memories (three modules: layer 0's weights, the thresholds of layers 0-4 under scheme 1): for every word, v is
//     the bitwise majority of the low `ebits` of the three stored words -- the voter of phys_logical -- and the low
//     `ebits` of all three modules become v.
//   Coded threshold memories (code 1), per LOGICAL element: with (d, c) the de-interleaved data and check words and
//     st = ecc_decode(d, c, &d'): st = 1, data d' and check ecc_encode(d') are stored (scheme 2: re-interleaved; only the
//     element's own bits of the two physical lines change); st = 0 or 2, nothing is written (ecc_repair, ecc.h).
//   Every other memory is untouched: the weights of layers >= 1, single-module thresholds (layers 5-7 under TMR),
//     uncoded memories, CNV layer 0 under code 1 included.
// So a repair fixes only what the redundancy covers, and it locks in what the redundancy gets wrong: a TMR bit hit in two
// modules, a triple error the decoder accepts as a correction -- valid stored states that no later repair touches.  In
// error-pattern terms (what k_repair_state applies to the state words of k_xmem_noise_t / k_emem_noise_t):
//     TMR    (m0, m1, m2) -> (v, v, v), v = maj(m0, m1, m2)
//     coded  (dm, cm) -> (m, ecc_encode(m)) when ecc_decode(dm, cm, &m) is 1, else unchanged (the code is linear: ecc.h)
// The logical parameters are the same before and after a repair: it changes only what later upsets meet.
// Counts per (run, epoch, layer), eight: the six above, then [6] the logical words the repair of that epoch rewrote (TMR:
// words where some module differed from the vote, counted once; coded: status-1 words) and [7] the words of the layer's
// repaired memories whose stored state still differs from the loaded one after the repair (TMR: vote != loaded; coded:
// left at status 2, or a wrong code word -- one this repair wrote or an earlier one locked in).  Both 0 in an epoch
// without a repair and for a layer without redundancy; CNV layer 0 counts weights and thresholds together.
// On the host: MARKER records among the 9-int records (bnn_mi355x_pack_params_repair), layer -1 "repair all memories
// now", layer -2 "rewrite all memories from the loaded parameters now"; the blob of (run, epoch t) is that of the
// concatenation over epochs 0 ... t of [the epoch's marker, if one is due] + the epoch's records in the in-epoch order.
// TMR plus a code stays refused.  Like the voter and the code, the repair is the project's own model: parity unpinned.
enum : int { kMarkRepair = -1, kMarkRewrite = -2 };
inline bool exposure_rewrites(int t, int scrub_every) { return t > 0 && scrub_every > 0 && t % scrub_every == 0; }
inline bool exposure_repairs(int t, int scrub_every, int repair_every) {
  return t > 0 && repair_every > 0 && t % repair_every == 0 && !exposure_rewrites(t, scrub_every);
}

// ---- coded weight memories (bnn_mi355x_wecc_exposure_campaigns): the code of wecc.h over the weights of layers >= 1 -----
// `weight_code` is a third axis next to scheme and code: 0 (none: everything above, unchanged) or 1 (SEC-DED (72,64)).
// Weight code 1 covers the weight memory of every layer but CNV layer 0 -- every layer >= 1 of the CNV nets, all four of
// the LFC nets (their layer 0 runs on the device path).  CNV layer 0 is not coded: its element width (3 or 6 bits) does
// not divide 64, it lives on the host route, and TMR already replicates it; it is treated as the threshold code treats it.
// CODE WORD q of a layer is sites [64 q, 64 q + 64) of its weight memory in the PE-major site order of enumerate_faults
// and k_xmem_noise_w (site = element * ebits + bit, element = pe * WMEM + ind; ebits divides 64, and a PE holds a
// multiple of 64 sites, so no code word straddles PEs): 64 / ebits whole elements.  For 2-bit weights a site is one bit
// of an ap_int<2> field, so a code word covers 32 columns.
// Storage: the 8 check bits of code word q are element q of a CHECK MEMORY of the layer's own -- (PE, code word of the
// PE) shaped, WMEM * ebits / 64 words per PE -- addressed as module 1 of target 0 (no scheme gives the weights of these
// layers a second module).  The logical weights are decode(data, check).
// Upsets: the data memory draws exactly as above (module 0: the uncoded campaign's records, same counter words, same
// order); the check memory draws by the same construction at element width 8 with module 1 in the counter word: per_c =
// ceil(8 / b) groups per element, e = q * per_c + g, an event a pure XOR of bits [g * b, min(g * b + b, 8)) of the check
// word, at the layer's weight rate.  Bursts do not cross elements, so they cross neither code words nor from one memory
// into the other.  Order inside an epoch: module-major, data then check.
// Repair (a repair epoch), per code word: status 1 stores the delivered data and its wecc_encode, status 0 or 2 writes
// nothing; a full rewrite clears the weight state like every other memory.  weight_code 1 goes with every (scheme, code,
// repair_every) combination the repair route accepts, TMR included.
// Counts per (run, epoch, layer), twelve: the eight above (weights physical = data plus check bits flipped, weights
// logical = data bits that differ after decoding), then [8] / [9] the weight code words whose decode status after the
// epoch is 1 / 2, [10] the code words the epoch's repair rewrote (status 1) and [11] those whose stored state still
// differs from the loaded one after the repair; [10] and [11] are 0 in an epoch without a repair.
// A check-memory record: target 0, module 1, mem the PE, ind the code word of the PE, bit g * b, word_size b.
// Like the voter, the threshold code and the repair this is the project's own model: parity unpinned.
BNN_HD inline uint32_t wecc_check_groups(int burst) { return (uint32_t)((kWeccCheckBits + burst - 1) / burst); }
//
// COLUMN-INTERLEAVED code words (bnn_mi355x_iwecc_exposure_campaigns): a fourth axis `weight_interleave`, 0 (none:
// everything above, unchanged) or 1; it needs weight_code 1 and covers exactly the layers weight_code 1 covers.  Why: a
// burst stays inside one element, and above its bits all land in one code word -- an aligned burst of 2 in an even-width
// element always flips an even number of bits of it, so the overall parity never fires and nothing is corrected.  Real
// block RAM ECC stripes adjacent columns over different code words; this is that.
// Depth: per layer D = gcd(kMaxBurst = 16, code words per PE (wecc_words_per_pe)); an odd count gives D = 1, coded and not
// interleaved (in the five nets every coded layer's count is even: D is 2, 8 or 16).  D divides the code words per PE, so
// no group straddles PEs.
// GROUP G of a layer is D consecutive code words' worth of storage in the site order above: its data memory is sites
// [64 D G, 64 D (G + 1)), its check memory elements [D G, D (G + 1)), 8 bits each.  Only the MEMBERSHIP changes:
//   data   the site at offset p of the group (0 <= p < 64 D) is data bit p / D of code word p % D of the group
//   check  the bit at offset r = 8 * element + bit of the group's check elements (0 <= r < 8 D) is check bit r / D of code
//          word r % D of the group
// so columns adjacent in a memory word lie in different code words, as far apart as D allows.  The weights stay where
// they were (site s is the same weight), and so does every upset: the events of both memories are exactly weight_code
// 1's records (bnn_mi355x_wecc_exposure_mask lists them).  A burst of b bits lands in min(b, D) different code words.
// Delivery is wecc_decode per code word over the gathered bits, the corrected bit scattered back to its site; a repair is
// wecc_repair per code word, status 1 writing the delivered data and fresh check bits to their scattered places; a full
// rewrite clears everything.  Orthogonal to (scheme, code, repair_every).  The twelve counts keep their meaning; [8] ...
// [11] count CODE WORDS AFTER GATHERING, not physical 64-site words; [0] is weight_code 1's, the events being the same.
// Consequences: one event of any width <= D leaves every code word at status <= 1 and the delivered weights the loaded
// ones; an aligned burst of 2 D in an element that wide puts two flipped bits into each of the D code words (status 2 for
// all, nothing corrected): the depth's limit.  The project's own model, like the code it lays out: parity unpinned.
enum : int { WI_NONE = 0, WI_COLUMNS = 1 };
// data: offset p in [0, 64 D) of a group <-> (code word of the group, data bit); check likewise with r in [0, 8 D)
BNN_HD inline void iwecc_member(int depth, int offset, int *word, int *bit) {
  *word = offset % depth;
  *bit = offset / depth;
}
BNN_HD inline int iwecc_offset(int depth, int word, int bit) { return bit * depth + word; }

// ---- host only from here ---------------------------------------------------------------------------------------------

// hardening_layout plus the code: "" and the organisation, else why (network, scheme, code, layer) is refused.
// check_bits: 6 where the layer's threshold memory is coded (then t_modules counts the check memory: 2), else 0
struct EccOrg { MemOrg org; int check_bits; };
std::string ecc_layout(const NetSpec &net, int scheme, int code, int layer, EccOrg &out);
// the code words per PE of a layer's weight memory where weight_code covers it, else 0 (weight_code 0, CNV layer 0)
int wecc_words_per_pe(const NetSpec &net, int weight_code, int layer);
// "" or why the weight code is refused
std::string wecc_check(int weight_code);
// "" or why the pair is refused (wecc_check's reasons first)
std::string iwecc_check(int weight_code, int weight_interleave);
// the interleave depth of a layer's coded weight memory: 0 not coded, 1 coded and not interleaved (weight_interleave 0, or
// an odd count of code words per PE), else gcd(kMaxBurst, code words per PE)
int wecc_depth(const NetSpec &net, int weight_code, int weight_interleave, int layer);
// the code word of the layer (PE-major) and the bit of it that a site holds: module 0 a data site of the weight memory
// (bit 0 ... 63), module 1 a bit 8 * element + bit of the check memory (bit 0 ... 7); false for a layer that is not coded
// or an index outside the memory.  iwecc_site_of is the inverse: the site (or check bit index) of (code word, bit)
bool iwecc_site(const NetSpec &net, int weight_code, int weight_interleave, int layer, int module, long index, long *word, int *bit);
long iwecc_site_of(const NetSpec &net, int weight_code, int weight_interleave, int layer, int module, long word, int bit);

struct PhysFault { Fault f; int module; };

// The physical memories of layers [l0, l1): mod[m] holds module m's words in RawParams' own shape (a memory with one
// module lives in mod[0]; threshold words are the interleaved ones).
struct PhysParams {
  int l0 = 0, l1 = 0;
  RawParams mod[3];
};
// what the loader stores from the parameter files.  code 1: the check memory of a coded layer in mod[1].t[l], filled
// from the logical elements
// weight_code 1: the check memory of a coded layer's weights in mod[1].w[l] ([pe][code word of the PE])
// weight_interleave 1: the check bits at their interleaved places (element [pe][D G + i] of the PE's groups)
void phys_load(const NetSpec &net, int scheme, const RawParams &raw, int l0, int l1, PhysParams &out, int code = 0, int weight_code = 0,
               int weight_interleave = 0);
// one physical fault; returns apply_fault's result, -1 also for a module the memory does not have.  A record of a check
// memory (code 1, target 1, module 1) XORs bits [bit, min(bit + word_size, 6)) of the check word, bit aligned as there
// weight_code 1: a record of a weight check memory (target 0, module 1) likewise at width 8
int phys_apply(const NetSpec &net, int scheme, PhysParams &p, const PhysFault &pf, int code = 0, int weight_code = 0);
// de-interleave(vote(modules)) into out.w[l], out.t[l] for l in [l0, l1).  A memory with one module and no interleave
// is copied word for word; a voted or de-interleaved word holds its element's bits alone.  code 1: a coded layer's
// words end with the decode (they hold the 16 delivered bits alone); status, where given, counts per layer the words
// decoded with status 1 ([l][0]) and 2 ([l][1])
// weight_code 1: a coded layer's weight words end with the decode of their code words; wstatus the same counts for them
void phys_logical(const NetSpec &net, int scheme, const PhysParams &p, RawParams &out, int code = 0, long (*status)[2] = nullptr,
                  int weight_code = 0, long (*wstatus)[2] = nullptr, int weight_interleave = 0);
// one repair ("repair scrubs" above) of the memories of layers [l0, l1) that have redundancy, in place.  counts, where
// given, receives per layer [l][0] the words rewritten and, with `loaded` (phys_load's result for the same arguments),
// [l][1] the words of the repaired memories whose stored state still differs from the loaded one afterwards.
// weight_code 1: the coded weight memories are repaired too, counted apart in wcounts (code words)
void phys_repair(const NetSpec &net, int scheme, int code, PhysParams &p, int l0, int l1, long (*counts)[2],
                 const PhysParams *loaded = nullptr, int weight_code = 0, long (*wcounts)[2] = nullptr, int weight_interleave = 0);
// the records of bnn_mi355x_pack_params_repair, 9 ints each, applied to p in order: a fault record through phys_apply, a
// marker (layer kMarkRepair / kMarkRewrite) as a repair of all memories / a return to `loaded`.  "" or why a record is
// refused, naming it; every layer field is checked before anything is applied
std::string phys_replay(const NetSpec &net, int scheme, int code, const PhysParams &loaded, PhysParams &p, const int *records, int n,
                        int weight_code = 0, int weight_interleave = 0);

// element width in bits of a layer's weight (target 0) or threshold (target 1) memory; 0: no threshold memory
int mem_element_bits(const LayerSpec &L, int target);
// bits an event of group `bit / burst` flips: burst, less where the element ends
inline int event_width(int ebits, int burst, int bit) { return ebits - bit < burst ? ebits - bit : burst; }

// the events of one (run seed, layer, target, module) in event order as physical faults (image 0, word_size burst);
// returns their number (0: thresholds of a layer without any), -1 for a bad scheme, burst, layer, target or module;
// writes events first .. first + cap - 1 to out (which may be null).  epoch: the exposure campaigns' (above); the
// records' image field holds it.  code 1: module 1 of a coded layer's thresholds lists the check memory's events;
// weight_code 1: module 1 of a coded layer's weights likewise.  weight_interleave changes no event (only which code word
// a bit belongs to): it is checked (-1 for a pair iwecc_check refuses) and otherwise without effect
long hardened_mem_noise_mask(const NetSpec &net, int scheme, int burst, uint64_t run_seed, int layer, int target, int module,
                             uint32_t rate_q32, long first, PhysFault *out, long cap, int epoch = 0, int code = 0, int weight_code = 0,
                             int weight_interleave = 0);

}  // namespace bnn
