// input_faults.cpp -- site tables of the input-buffer faults (input_faults.h); host only.
#include "input_faults.h"

#include <algorithm>

#include "act_faults.h"

namespace bnn {

long enumerate_input_faults(const NetSpec &net, long first, InputSite *out, long cap) {
  const long total = input_sites(net);
  for (long s = std::max(first, 0L), k = 0; out && s < total && k < cap; s++, k++) out[k] = InputSite{(int)(s >> 3), (int)(s & 7)};
  return total;
}

std::string check_input_fault(const NetSpec &net, const InputSite &s) {
  if (s.byte < 0 || s.byte >= net.image_bytes())
    return "input site: byte must be 0 ... " + std::to_string(net.image_bytes() - 1) + " (the image's bytes as bnn_mi355x_inference_buffer takes them)";
  if (s.bit < 0 || s.bit > 7) return "input site: bit must be 0 ... 7 (0 the LSB)";
  return "";
}

long input_noise_mask(const NetSpec &net, uint64_t run_seed, int image, uint32_t rate_q32, long first, InputSite *out, long cap) {
  const long sites = input_sites(net);  // (a multiple of 128: the kernel's 16-byte lanes)
  long total = 0;
  if (rate_q32 == 0) return 0;
  for (long b = 0; 4 * b < sites; b++) {
    uint32_t u[4];
    act_noise_block((uint32_t)run_seed, (uint32_t)(run_seed >> 32), (uint32_t)image, kInputNoiseTag, (uint32_t)b, u);
    for (int e = 0; e < 4; e++) {
      if (u[e] >= rate_q32) continue;
      const long s = 4 * b + e;
      if (out && total >= first && total - first < cap) out[total - first] = InputSite{(int)(s >> 3), (int)(s & 7)};
      total++;
    }
  }
  return total;
}

}  // namespace bnn
