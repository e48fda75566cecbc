// act_faults.cpp -- site tables of the activation-fault sweeps (act_faults.h); host only.
#include "act_faults.h"

#include <algorithm>

namespace bnn {

bool act_shape(const NetSpec &net, int layer, ActShape *s) {
  if (layer < 0 || layer + 1 >= net.nlayers) return false;
  const LayerSpec &L = net.L[layer];
  const int d = L.pool ? L.ofm_dim / 2 : L.ofm_dim;
  *s = ActShape{d, d, L.ofm_ch, L.out_planes == 2 ? 3 : 2};
  return L.out_planes > 0;
}

long enumerate_act_faults(const NetSpec &net, int layer, long first, ActSite *out, long cap) {
  ActShape s;
  if (!act_shape(net, layer, &s)) return -1;
  const long shifts = s.levels - 1, total = (long)s.h * s.w * s.c * shifts;
  for (long i = std::max(first, 0L), k = 0; out && i < total && k < cap; i++, k++) {
    long e = i / shifts;
    ActSite a{};
    a.layer = layer;
    a.shift = (int)(i - e * shifts) + 1;
    a.channel = (int)(e % s.c);
    e /= s.c;
    a.x = (int)(e % s.w);
    a.y = (int)(e / s.w);
    out[k] = a;
  }
  return total;
}

std::string check_act_fault(const NetSpec &net, const ActSite &a) {
  ActShape s;
  if (!act_shape(net, a.layer, &s))
    return "activation site: layer " + std::to_string(a.layer) + " has no activation sites (the last layer and layers out of range have none)";
  if (a.y < 0 || a.y >= s.h || a.x < 0 || a.x >= s.w || a.channel < 0 || a.channel >= s.c)
    return "activation site outside layer " + std::to_string(a.layer) + "'s output map (" + std::to_string(s.h) + " x " +
           std::to_string(s.w) + " x " + std::to_string(s.c) + ")";
  if (a.shift < 1 || a.shift >= s.levels)
    return "activation site: shift must be 1 ... " + std::to_string(s.levels - 1) + " for layer " + std::to_string(a.layer);
  return "";
}

long act_noise_mask(const NetSpec &net, uint64_t run_seed, int image, int layer, uint32_t rate_q32, long first, ActSite *out, long cap) {
  ActShape s;
  if (!act_shape(net, layer, &s)) return -1;
  const long sites = (long)s.h * s.w * s.c;  // (a multiple of 32 for every layer of the five networks)
  long total = 0;
  if (rate_q32 == 0) return 0;
  for (long b = 0; 4 * b < sites; b++) {
    uint32_t u[4];
    act_noise_block((uint32_t)run_seed, (uint32_t)(run_seed >> 32), (uint32_t)image, (uint32_t)layer, (uint32_t)b, u);
    for (int e = 0; e < 4 && 4 * b + e < sites; e++) {
      if (u[e] >= rate_q32) continue;
      if (out && total >= first && total - first < cap) {
        long p = (4 * b + e) / s.c;
        out[total - first] = ActSite{layer, (int)(p / s.w), (int)(p % s.w), (int)((4 * b + e) % s.c), s.levels == 3 ? 1 + (int)(u[e] & 1) : 1};
      }
      total++;
    }
  }
  return total;
}

}  // namespace bnn
