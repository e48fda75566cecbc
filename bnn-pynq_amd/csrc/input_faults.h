// input_faults.h -- faults in the image buffer every classification starts from (bnn_mi355x_input_fault_sweep,
// bnn_mi355x_input_noise_campaigns); host only.
//
// A site is one bit of one input byte, the bytes in the layout of bnn_mi355x_inference_buffer (CNV: 3072 per image,
// planar CHW; LFC: 784, row-major); the label byte of a CIFAR record and the idx header are not sites.  Site number
// s = byte * 8 + bit, bit 0 the LSB.  A fault XORs that bit while that image is classified.  The reference holds no
// input injection: this model is the project's own.
#pragma once
#include <stdint.h>

#include <string>

#include "topology.h"

namespace bnn {

struct InputSite { int byte, bit; };

inline long input_sites(const NetSpec &net) { return (long)net.image_bytes() * 8; }

// every site in site order; returns their number; writes sites first .. first + cap - 1 to out
long enumerate_input_faults(const NetSpec &net, long first, InputSite *out, long cap);

// "" when the record names a site, else the reason
std::string check_input_fault(const NetSpec &net, const InputSite &s);

// Random upsets of the same sites (bnn_mi355x_input_noise_campaigns): every site is flipped with probability
// rate / 2^32, independently per (run seed k, image i, site s):
//   u = philox4x32_10(counter {i, 0xffffffff, s >> 2, 0}, key {k & 0xffffffff, k >> 32})[s & 3];  flipped iff u < rate.
// The second counter word is where act_noise_block takes the layer: no layer has that tag, so the draws of an
// activation campaign and of an input campaign never share a stream.  The host (input_noise_mask) and the kernel that
// flips the bits (kernels.hip, k_input_noise) both call act_noise_block (act_faults.h) with it.
constexpr uint32_t kInputNoiseTag = 0xffffffffu;

// the flipped sites of one (run seed, image) in site order, as sweep records; returns their number; writes flips
// first .. first + cap - 1 to out
long input_noise_mask(const NetSpec &net, uint64_t run_seed, int image, uint32_t rate_q32, long first, InputSite *out, long cap);

}  // namespace bnn
