// mem_faults.cpp -- see mem_faults.h (host only).
#include "mem_faults.h"

#include "act_faults.h"

namespace bnn {

long mem_noise_sites(const NetSpec &net, int layer, int target) { return enumerate_faults(net, layer, target, 1, 0, nullptr, 0); }

long mem_noise_mask(const NetSpec &net, uint64_t run_seed, int layer, int target, uint32_t rate_q32, long first, Fault *out, long cap) {
  const long sites = mem_noise_sites(net, layer, target);
  if (sites < 0) return -1;
  long total = 0;
  if (rate_q32 == 0) return 0;
  for (long b = 0; 4 * b < sites; b++) {
    uint32_t u[4];
    act_noise_block((uint32_t)run_seed, (uint32_t)(run_seed >> 32), (uint32_t)layer, (uint32_t)target, (uint32_t)b, u, kMemNoiseTag);
    for (int e = 0; e < 4 && 4 * b + e < sites; e++) {
      if (u[e] >= rate_q32) continue;
      if (out && total >= first && total - first < cap) enumerate_faults(net, layer, target, 1, 4 * b + e, out + (total - first), 1);
      total++;
    }
  }
  return total;
}

}  // namespace bnn
