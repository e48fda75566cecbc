// mem_org.cpp -- see mem_org.h (host only).
#include "mem_org.h"

#include <cstring>

#include "act_faults.h"
#include "mem_faults.h"

namespace bnn {

int mem_element_bits(const LayerSpec &L, int target) {
  if (target == 0) return L.fold.simd * L.wbits;
  return L.nthr == 0 ? 0 : (L.thr24 ? 24 : 16);
}

int hardening_scheme_of(const char *name) {
  const char *dash = name ? std::strchr(name, '-') : nullptr;
  if (!dash) return HS_NONE;
  if (!std::strcmp(dash, "-TMR")) return HS_TMR;
  if (!std::strcmp(dash, "-interleaved")) return HS_INTERLEAVED;
  if (!std::strcmp(dash, "-resilient-interleaved")) return HS_RESILIENT;
  return HS_NONE;
}

std::string hardening_layout(const NetSpec &net, int scheme, int layer, MemOrg &out) {
  if (scheme < HS_NONE || scheme > HS_RESILIENT) return "scheme must be 0 (none), 1 (TMR), 2 (interleaved) or 3 (resilient-interleaved)";
  if (layer < 0 || layer >= net.nlayers) return "layer must be 0 ... " + std::to_string(net.nlayers - 1);
  out = MemOrg{1, 1, 0};
  if (scheme == HS_NONE) return "";
  if (!net.is_cnv)
    return std::string(net.name) + ": no hardened memory organisation is modelled for the LFC networks (the one LFC overlay interleaves "
           "24-bit elements into 16-bit words; what its hardware makes of that is not in the reference)";
  if (net.id == NET_CNVW2A2 && scheme == HS_INTERLEAVED)
    return "cnvW2A2 with scheme 2 (interleaved): the reference interleaves its 64-bit weight elements with a 64-bit pattern for 128 "
           "positions and reads past the second element: no defined layout to model";
  const bool thr = net.L[layer].nthr > 0;
  if (scheme == HS_TMR) {
    if (layer == 0) out.w_modules = 3;
    if (layer <= 4 && thr) out.t_modules = 3;
  } else if (thr) {
    out.t_interleave = scheme;
  }
  return "";
}

void phys_load(const NetSpec &net, int scheme, const RawParams &raw, int l0, int l1, PhysParams &out) {
  out.l0 = l0;
  out.l1 = l1;
  for (int l = l0; l < l1; l++) {
    const LayerSpec &L = net.L[l];
    MemOrg org{1, 1, 0};
    hardening_layout(net, scheme, l, org);
    for (int m = 0; m < 3; m++) {
      out.mod[m].w[l].clear();
      out.mod[m].t[l].clear();
    }
    for (int m = 0; m < org.w_modules; m++) out.mod[m].w[l] = raw.w[l];
    std::vector<std::vector<uint64_t>> t = raw.t[l];
    if (org.t_interleave) {
      const int T = mem_element_bits(L, 1), lines = L.fold.tmem;
      const uint64_t emask = (1ull << T) - 1;
      for (size_t pe = 0; pe < t.size(); pe++)
        for (int ind = 0; ind + 1 < lines; ind += 2)  // (an odd last line stays as the file has it)
          for (int i = 0; i < L.nthr; i++) {
            uint64_t w[2] = {0, 0};
            for (int half = 0; half < 2; half++)
              for (int bit = 0; bit < T; bit++) {
                int pi, pb;
                interleave_site(org.t_interleave, T, lines, ind + half, bit, &pi, &pb);
                w[pi - ind] |= ((raw.t[l][pe][(size_t)(ind + half) * L.nthr + i] >> bit) & 1) << pb;
              }
            t[pe][(size_t)ind * L.nthr + i] = w[0] & emask;
            t[pe][(size_t)(ind + 1) * L.nthr + i] = w[1] & emask;
          }
    }
    for (int m = 0; m < org.t_modules; m++) out.mod[m].t[l] = t;
  }
}

int phys_apply(const NetSpec &net, int scheme, PhysParams &p, const PhysFault &pf) {
  const Fault &f = pf.f;
  if (f.layer < p.l0 || f.layer >= p.l1 || (f.target != 0 && f.target != 1)) return -1;
  MemOrg org{1, 1, 0};
  if (!hardening_layout(net, scheme, f.layer, org).empty()) return -1;
  if (pf.module < 0 || pf.module >= (f.target == 0 ? org.w_modules : org.t_modules)) return -1;
  return apply_fault(net, p.mod[pf.module], f);
}

namespace {
// module 0, or the bitwise majority of the three modules' low ebits
void vote(const RawParams *mod, bool thresholds, int l, int modules, int ebits, std::vector<std::vector<uint64_t>> &out) {
  auto mem = [&](int m) -> const std::vector<std::vector<uint64_t>> & { return thresholds ? mod[m].t[l] : mod[m].w[l]; };
  out = mem(0);
  if (modules != 3) return;
  const uint64_t emask = ebits >= 64 ? ~0ull : (1ull << ebits) - 1;
  for (size_t pe = 0; pe < out.size(); pe++)
    for (size_t i = 0; i < out[pe].size(); i++) {
      const uint64_t a = mem(0)[pe][i], b = mem(1)[pe][i], c = mem(2)[pe][i];
      out[pe][i] = ((a & b) | (a & c) | (b & c)) & emask;
    }
}
}  // namespace

void phys_logical(const NetSpec &net, int scheme, const PhysParams &p, RawParams &out) {
  for (int l = p.l0; l < p.l1; l++) {
    const LayerSpec &L = net.L[l];
    MemOrg org{1, 1, 0};
    hardening_layout(net, scheme, l, org);
    vote(p.mod, false, l, org.w_modules, mem_element_bits(L, 0), out.w[l]);
    if (L.nthr == 0) {
      out.t[l] = p.mod[0].t[l];
      continue;
    }
    std::vector<std::vector<uint64_t>> v;
    vote(p.mod, true, l, org.t_modules, mem_element_bits(L, 1), v);
    out.t[l] = v;
    if (!org.t_interleave) continue;
    const int T = mem_element_bits(L, 1), lines = L.fold.tmem;
    for (size_t pe = 0; pe < v.size(); pe++)
      for (int ind = 0; ind + 1 < lines; ind += 2)
        for (int i = 0; i < L.nthr; i++) {
          uint64_t e[2] = {0, 0};
          for (int half = 0; half < 2; half++)
            for (int pb = 0; pb < T; pb++) {
              int li, lb;
              interleave_source(org.t_interleave, T, lines, ind + half, pb, &li, &lb);
              e[li - ind] |= ((v[pe][(size_t)(ind + half) * L.nthr + i] >> pb) & 1) << lb;
            }
          out.t[l][pe][(size_t)ind * L.nthr + i] = e[0];
          out.t[l][pe][(size_t)(ind + 1) * L.nthr + i] = e[1];
        }
  }
}

long hardened_mem_noise_mask(const NetSpec &net, int scheme, int burst, uint64_t run_seed, int layer, int target, int module,
                             uint32_t rate_q32, long first, PhysFault *out, long cap, int epoch) {
  if (burst < 1 || burst > kMaxBurst || epoch < 0 || epoch >= kMaxEpochs) return -1;
  MemOrg org{1, 1, 0};
  if (!hardening_layout(net, scheme, layer, org).empty()) return -1;
  const long events = enumerate_faults(net, layer, target, burst, 0, nullptr, 0);
  if (events < 0 || module < 0 || module >= (target == 0 ? org.w_modules : org.t_modules)) return -1;
  long total = 0;
  if (rate_q32 == 0) return 0;
  const uint32_t word = hardened_draw_word(target, module, burst);
  for (long b = 0; 4 * b < events; b++) {
    uint32_t u[4];
    act_noise_block((uint32_t)run_seed, (uint32_t)(run_seed >> 32), (uint32_t)layer, word, (uint32_t)b, u, exposure_tag((uint32_t)epoch));
    for (int e = 0; e < 4 && 4 * b + e < events; e++) {
      if (u[e] >= rate_q32) continue;
      if (out && total >= first && total - first < cap) {
        PhysFault &pf = out[total - first];
        enumerate_faults(net, layer, target, burst, 4 * b + e, &pf.f, 1);
        pf.module = module;
        pf.f.image = epoch;
      }
      total++;
    }
  }
  return total;
}

}  // namespace bnn
