// mem_faults.h -- random upsets of the parameter memories at a rate per bit (bnn_mi355x_mem_noise_campaigns).
//
// The sites of layer L and target (0 weights, 1 thresholds) are the records enumerate_faults(net, L, target,
// word_size 1, ...) lists, site s being a record's index in that list:
//   weights     s = (mem * WMEM + ind) * (SIMD * wbits) + bit
//   thresholds  s = ((mem * TMEM + ind) * nthr + thresh) * ebits + bit      (ebits 24 for thr24 layers, else 16)
// For run seed k every site is flipped with probability rate / 2^32, independently:
//   u = philox4x32_10(counter {L, target, s >> 2, 1}, key {k & 0xffffffff, k >> 32})[s & 3];  flip iff u < rate
// (act_noise_block of act_faults.h with the fourth counter word 1: the activation and input draws have 0 there).  A
// run's parameters are what apply_fault makes of the loaded memories with every flipped site applied as a word_size-1
// record -- layer-major, per layer weights then thresholds, in site order -- present from the first image on.
// Host only: mem_noise_mask is the statement of the draw the tests restate, and what the campaign itself calls for
// layer 0 of the CNV nets; the other layers' sites are drawn on the device by the same routine (kernels.hip,
// k_mem_noise_w / k_mem_noise_t).
#pragma once
#include <stdint.h>

#include "faults.h"
#include "topology.h"

namespace bnn {

constexpr uint32_t kMemNoiseTag = 1;  // the fourth counter word of the draw

// number of sites; 0 for the thresholds of a layer without any, -1 for a bad layer or target
long mem_noise_sites(const NetSpec &net, int layer, int target);

// the flipped sites of one (run seed, layer, target) in site order as fault records (image 0, word_size 1); returns
// their number, -1 for a bad layer or target; writes flips first .. first + cap - 1 to out (which may be null)
long mem_noise_mask(const NetSpec &net, uint64_t run_seed, int layer, int target, uint32_t rate_q32, long first, Fault *out, long cap);

}  // namespace bnn
