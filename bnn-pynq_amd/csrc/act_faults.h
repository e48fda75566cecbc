// act_faults.h -- single faults in the inter-layer activation stream (bnn_mi355x_act_fault_sweep).
//
// A site is one activation of layer L's output as layer L+1 reads it (CNV layers 1 and 3: after the max-pool), for
// every layer but the last.  The fault replaces the activation's level index i (1-bit: -1, +1; 2-bit: -1, 0, +1) by
// (i + shift) mod levels, 1 <= shift < levels: a sign flip, or the next / the one after next of the three levels.
// The reference holds no activation-fault model (its TargetType::Activations means threshold memories): this one
// is the project's own.
#pragma once
#include <stdint.h>

#include <string>

#include "topology.h"

namespace bnn {

struct ActSite { int layer, y, x, channel, shift; };

// layer L's output map as the next layer reads it: h x w pixels of c channels, `levels` values per activation
struct ActShape { int h, w, c, levels; };

// false for the last layer (scores / words, no activations) or a layer out of range
bool act_shape(const NetSpec &net, int layer, ActShape *s);

// every site x shift of layer L ordered by (y, x, channel, shift); returns their number, -1 for a layer without
// sites; writes sites first .. first + cap - 1 to out
long enumerate_act_faults(const NetSpec &net, int layer, long first, ActSite *out, long cap);

// "" when the record names a site and a shift of a layer that has them, else the reason
std::string check_act_fault(const NetSpec &net, const ActSite &s);

// Random upsets of the same sites (bnn_mi355x_act_noise_campaigns): every site of layer L's output is upset with
// probability rate / 2^32, independently per (run seed k, image i, layer L, site s), s counting (y, x, channel):
//   u = philox4x32_10(counter {i, L, s >> 2, 0}, key {k & 0xffffffff, k >> 32})[s & 3];  upset iff u < rate,
// with shift 1 + (u & 1) for 2-bit activations, 1 for 1-bit ones.  The host (act_noise_mask) and the kernel that
// applies the upsets (kernels.hip, k_act_noise) both call act_noise_block: one block serves four consecutive sites.
// `tag` is the fourth counter word: 0 for the activation and the input draws, 1 for the parameter memories' (mem_faults.h),
// whose first three words are (layer, target, block) -- so the models never share a stream.
#ifndef BNN_HD
#define BNN_HD
#endif
BNN_HD inline void act_noise_block(uint32_t key0, uint32_t key1, uint32_t image, uint32_t layer, uint32_t block, uint32_t out[4],
                                   uint32_t tag = 0) {
  uint32_t c0 = image, c1 = layer, c2 = block, c3 = tag;
#pragma unroll
  for (int r = 0; r < 10; r++) {  // Philox4x32-10 (Salmon et al., SC'11)
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ key0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ key1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    key0 += 0x9E3779B9u;
    key1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// the upset sites of one (run seed, image, layer) in site order, as sweep records; returns their number, -1 for a
// layer without sites; writes upsets first .. first + cap - 1 to out
long act_noise_mask(const NetSpec &net, uint64_t run_seed, int image, int layer, uint32_t rate_q32, long first, ActSite *out, long cap);

}  // namespace bnn
