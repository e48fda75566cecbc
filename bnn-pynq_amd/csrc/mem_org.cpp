// mem_org.cpp -- see mem_org.h (host only).
#include "mem_org.h"

#include <algorithm>
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

std::string ecc_layout(const NetSpec &net, int scheme, int code, int layer, EccOrg &out) {
  out.check_bits = 0;
  const std::string e = hardening_layout(net, scheme, layer, out.org);
  if (!e.empty()) return e;
  if (code < EC_NONE || code > EC_SECDED) return "code must be 0 (none) or 1 (SEC-DED)";
  if (code == EC_NONE) return "";
  if (scheme == HS_TMR) return "code 1 with scheme 1 (TMR): TMR plus a code is not modelled";
  if (scheme == HS_RESILIENT)
    return "code 1 with scheme 3 (resilient-interleaved): the resilient patterns are defined for 32 and 48 positions only, not for the 12 of a "
           "pair of check words";
  const LayerSpec &L = net.L[layer];
  if (L.nthr > 0 && !L.thr24) {  // (the 24-bit thresholds of CNV layer 0 are not coded: ecc.h)
    out.check_bits = kEccCheckBits;
    out.org.t_modules = 2;
  }
  return "";
}

std::string wecc_check(int weight_code) {
  if (weight_code < WC_NONE || weight_code > WC_SECDED) return "weight_code must be 0 (none) or 1 (SEC-DED (72,64) over the weights of layers >= 1)";
  return "";
}

int wecc_words_per_pe(const NetSpec &net, int weight_code, int layer) {
  if (weight_code != WC_SECDED || layer < 0 || layer >= net.nlayers) return 0;
  const LayerSpec &L = net.L[layer];
  const int ebits = mem_element_bits(L, 0);
  // (CNV layer 0: int8 taps, 3 or 6 bits per element -- not coded: wecc.h)
  if (L.arith == AR_INT8 || ebits < 1 || 64 % ebits || ((long)L.fold.wmem * ebits) % 64) return 0;
  return (int)((long)L.fold.wmem * ebits / 64);
}

std::string iwecc_check(int weight_code, int weight_interleave) {
  const std::string e = wecc_check(weight_code);
  if (!e.empty()) return e;
  if (weight_interleave < WI_NONE || weight_interleave > WI_COLUMNS) return "weight_interleave must be 0 (none) or 1 (column-interleaved code words)";
  if (weight_interleave == WI_COLUMNS && weight_code != WC_SECDED) return "weight_interleave 1 needs weight_code 1";
  return "";
}

int wecc_depth(const NetSpec &net, int weight_code, int weight_interleave, int layer) {
  const int cwpp = wecc_words_per_pe(net, weight_code, layer);
  if (!cwpp) return 0;
  if (weight_interleave != WI_COLUMNS) return 1;
  int d = kMaxBurst;
  while (cwpp % d) d >>= 1;  // (kMaxBurst is a power of two: the gcd is the largest power of two <= 16 that divides)
  return d;
}

bool iwecc_site(const NetSpec &net, int weight_code, int weight_interleave, int layer, int module, long index, long *word, int *bit) {
  const int D = wecc_depth(net, weight_code, weight_interleave, layer);
  if (!D || (module != 0 && module != 1) || index < 0) return false;
  const long per = module == 0 ? kWeccDataBits : kWeccCheckBits;  // bits of a code word in this memory
  const long words = (long)net.L[layer].fold.pe * wecc_words_per_pe(net, weight_code, layer);
  if (index >= words * per) return false;
  const long G = index / (per * D);
  int w, b;
  iwecc_member(D, (int)(index - G * per * D), &w, &b);
  *word = G * D + w;
  *bit = b;
  return true;
}

long iwecc_site_of(const NetSpec &net, int weight_code, int weight_interleave, int layer, int module, long word, int bit) {
  const int D = wecc_depth(net, weight_code, weight_interleave, layer);
  if (!D || (module != 0 && module != 1) || word < 0) return -1;
  const long per = module == 0 ? kWeccDataBits : kWeccCheckBits;
  if (word >= (long)net.L[layer].fold.pe * wecc_words_per_pe(net, weight_code, layer) || bit < 0 || bit >= per) return -1;
  return word / D * (per * D) + iwecc_offset(D, (int)(word % D), bit);
}

namespace {
// code word cw of one PE's weight memory: its 64 data bits gathered from / scattered to the 64 / ebits elements it covers
uint64_t wecc_gather(const std::vector<uint64_t> &pe, int ebits, int cw) {
  const int n = 64 / ebits;
  const uint64_t emask = ebits >= 64 ? ~0ull : (1ull << ebits) - 1;
  uint64_t d = 0;
  for (int i = 0; i < n; i++) d |= (pe[(size_t)cw * n + i] & emask) << (i * ebits);
  return d;
}
void wecc_scatter(std::vector<uint64_t> &pe, int ebits, int cw, uint64_t d) {
  const int n = 64 / ebits;
  const uint64_t emask = ebits >= 64 ? ~0ull : (1ull << ebits) - 1;
  for (int i = 0; i < n; i++) pe[(size_t)cw * n + i] = (d >> (i * ebits)) & emask;
}

// the same at interleave depth D ("column-interleaved code words", mem_org.h), bit by bit: `width` bits of code word cw of
// one PE's memory of ebits-wide elements -- the data memory (width 64) or the check memory (width 8, ebits 8).  Depth 1 is
// wecc_gather / wecc_scatter and the check element itself
uint64_t iwecc_gather(const std::vector<uint64_t> &pe, int ebits, int width, int D, int cw) {
  const long base = (long)(cw / D) * width * D;
  uint64_t d = 0;
  for (int b = 0; b < width; b++) {
    const long site = base + iwecc_offset(D, cw % D, b);
    d |= ((pe[(size_t)(site / ebits)] >> (site % ebits)) & 1) << b;
  }
  return d;
}
void iwecc_scatter(std::vector<uint64_t> &pe, int ebits, int width, int D, int cw, uint64_t d) {
  const long base = (long)(cw / D) * width * D;
  for (int b = 0; b < width; b++) {
    const long site = base + iwecc_offset(D, cw % D, b);
    uint64_t &w = pe[(size_t)(site / ebits)];
    w = (w & ~(1ull << (site % ebits))) | ((d >> b) & 1) << (site % ebits);
  }
}
// code word cw of one PE at depth D: its data bits in the weight memory `pe`, its check bits in the check memory `pe`
// (D <= 1: the whole-element route that was there before the interleave)
uint64_t code_data(const std::vector<uint64_t> &pe, int ebits, int D, int cw) {
  return D <= 1 ? wecc_gather(pe, ebits, cw) : iwecc_gather(pe, ebits, kWeccDataBits, D, cw);
}
uint32_t code_check(const std::vector<uint64_t> &pe, int D, int cw) {
  return D <= 1 ? (uint32_t)pe[(size_t)cw] : (uint32_t)iwecc_gather(pe, kWeccCheckBits, kWeccCheckBits, D, cw);
}
void store_data(std::vector<uint64_t> &pe, int ebits, int D, int cw, uint64_t d) {
  if (D <= 1) wecc_scatter(pe, ebits, cw, d);
  else iwecc_scatter(pe, ebits, kWeccDataBits, D, cw, d);
}
void store_check(std::vector<uint64_t> &pe, int D, int cw, uint32_t c) {
  if (D <= 1) pe[(size_t)cw] = c;
  else iwecc_scatter(pe, kWeccCheckBits, kWeccCheckBits, D, cw, c);
}
}  // namespace

namespace {
// the threshold words of one layer with the pairs of lines (ind, ind + 1) of every PE interleaved (forward) or
// de-interleaved at element width T; an odd last line stays as it is
void permute_pairs(const LayerSpec &L, int il, int T, bool forward, std::vector<std::vector<uint64_t>> &t) {
  const int lines = L.fold.tmem;
  const uint64_t emask = (1ull << T) - 1;
  for (size_t pe = 0; pe < t.size(); pe++)
    for (int ind = 0; ind + 1 < lines; ind += 2)
      for (int i = 0; i < L.nthr; i++) {
        uint64_t *const at[2] = {&t[pe][(size_t)ind * L.nthr + i], &t[pe][(size_t)(ind + 1) * L.nthr + i]};
        uint64_t w[2] = {0, 0};
        for (int half = 0; half < 2; half++)
          for (int bit = 0; bit < T; bit++) {
            int oi, ob;
            if (forward) interleave_site(il, T, lines, ind + half, bit, &oi, &ob);
            else interleave_source(il, T, lines, ind + half, bit, &oi, &ob);
            w[oi - ind] |= ((*at[half] >> bit) & 1) << ob;
          }
        *at[0] = w[0] & emask;
        *at[1] = w[1] & emask;
      }
}
}  // namespace

void phys_load(const NetSpec &net, int scheme, const RawParams &raw, int l0, int l1, PhysParams &out, int code, int weight_code,
               int weight_interleave) {
  out.l0 = l0;
  out.l1 = l1;
  for (int l = l0; l < l1; l++) {
    const LayerSpec &L = net.L[l];
    EccOrg eo{MemOrg{1, 1, 0}, 0};
    ecc_layout(net, scheme, code, l, eo);
    const MemOrg &org = eo.org;
    for (int m = 0; m < 3; m++) {
      out.mod[m].w[l].clear();
      out.mod[m].t[l].clear();
    }
    for (int m = 0; m < org.w_modules; m++) out.mod[m].w[l] = raw.w[l];
    if (const int cwpp = wecc_words_per_pe(net, weight_code, l)) {  // the check words of the loaded code words in module 1
      const int ebits = mem_element_bits(L, 0);
      out.mod[1].w[l].assign(raw.w[l].size(), std::vector<uint64_t>((size_t)cwpp));
      const int D = wecc_depth(net, weight_code, weight_interleave, l);
      for (size_t pe = 0; pe < raw.w[l].size(); pe++)
        for (int cw = 0; cw < cwpp; cw++) store_check(out.mod[1].w[l][pe], D, cw, wecc_encode(code_data(raw.w[l][pe], ebits, D, cw)));
    }
    std::vector<std::vector<uint64_t>> t = raw.t[l];
    if (org.t_interleave) permute_pairs(L, org.t_interleave, mem_element_bits(L, 1), true, t);
    if (eo.check_bits) {  // data in module 0, the check words of the LOGICAL elements in module 1
      std::vector<std::vector<uint64_t>> c = raw.t[l];
      for (auto &pe : c)
        for (uint64_t &w : pe) w = ecc_encode((uint32_t)w);
      if (org.t_interleave) permute_pairs(L, org.t_interleave, kEccCheckBits, true, c);
      out.mod[0].t[l] = t;
      out.mod[1].t[l] = c;
      continue;
    }
    for (int m = 0; m < org.t_modules; m++) out.mod[m].t[l] = t;
  }
}

int phys_apply(const NetSpec &net, int scheme, PhysParams &p, const PhysFault &pf, int code, int weight_code) {
  const Fault &f = pf.f;
  if (f.layer < p.l0 || f.layer >= p.l1 || (f.target != 0 && f.target != 1)) return -1;
  EccOrg eo{MemOrg{1, 1, 0}, 0};
  if (!ecc_layout(net, scheme, code, f.layer, eo).empty()) return -1;
  const int cwpp = f.target == 0 ? wecc_words_per_pe(net, weight_code, f.layer) : 0;
  if (cwpp && pf.module == 1) {  // the weight check memory
    const LayerSpec &L = net.L[f.layer];
    if (f.word_size < 1 || f.word_size > 64 || f.mem < 0 || f.mem >= L.fold.pe || f.ind < 0 || f.ind >= cwpp || f.bit < 0 || f.bit >= kWeccCheckBits)
      return -1;
    const int at = (f.bit / f.word_size) * f.word_size;  // (apply_fault's alignment)
    const uint64_t flip = ((1ull << event_width(kWeccCheckBits, f.word_size, at)) - 1) << at;
    p.mod[1].w[f.layer][(size_t)f.mem][(size_t)f.ind] ^= flip;
    return (int)(((long)f.ind * 64 / mem_element_bits(L, 0)) / (L.fold.wmem / L.fold.tmem)) * L.fold.pe + f.mem;
  }
  if (pf.module < 0 || pf.module >= (f.target == 0 ? eo.org.w_modules : eo.org.t_modules)) return -1;
  if (f.target == 1 && eo.check_bits && pf.module == 1) {
    const LayerSpec &L = net.L[f.layer];
    if (f.word_size < 1 || f.word_size > 64 || f.mem < 0 || f.mem >= L.fold.pe || f.ind < 0 || f.ind >= L.fold.tmem || f.thresh < 0 ||
        f.thresh >= L.nthr || f.bit < 0 || f.bit >= kEccCheckBits)
      return -1;
    const int at = (f.bit / f.word_size) * f.word_size;  // (apply_fault's alignment)
    const uint64_t flip = ((1ull << event_width(kEccCheckBits, f.word_size, at)) - 1) << at;
    p.mod[1].t[f.layer][(size_t)f.mem][(size_t)f.ind * L.nthr + f.thresh] ^= flip;
    return f.ind * L.fold.pe + f.mem;
  }
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

void phys_logical(const NetSpec &net, int scheme, const PhysParams &p, RawParams &out, int code, long (*status)[2], int weight_code,
                  long (*wstatus)[2], int weight_interleave) {
  for (int l = p.l0; l < p.l1; l++) {
    const LayerSpec &L = net.L[l];
    EccOrg eo{MemOrg{1, 1, 0}, 0};
    ecc_layout(net, scheme, code, l, eo);
    const MemOrg &org = eo.org;
    if (status) status[l][0] = status[l][1] = 0;
    vote(p.mod, false, l, org.w_modules, mem_element_bits(L, 0), out.w[l]);
    if (wstatus) wstatus[l][0] = wstatus[l][1] = 0;
    if (const int cwpp = wecc_words_per_pe(net, weight_code, l)) {
      const int ebits = mem_element_bits(L, 0);
      const int D = wecc_depth(net, weight_code, weight_interleave, l);
      for (size_t pe = 0; pe < out.w[l].size(); pe++)
        for (int cw = 0; cw < cwpp; cw++) {
          // (a correction changes bits of this code word alone, so the code words of a group do not depend on the order)
          uint64_t d;
          const int st = wecc_decode(code_data(out.w[l][pe], ebits, D, cw), code_check(p.mod[1].w[l][pe], D, cw), &d);
          if (st == 1) store_data(out.w[l][pe], ebits, D, cw, d);
          if (wstatus && st) wstatus[l][st - 1]++;
        }
    }
    if (L.nthr == 0) {
      out.t[l] = p.mod[0].t[l];
      continue;
    }
    std::vector<std::vector<uint64_t>> v;
    vote(p.mod, true, l, eo.check_bits ? 1 : org.t_modules, mem_element_bits(L, 1), v);
    if (org.t_interleave) permute_pairs(L, org.t_interleave, mem_element_bits(L, 1), false, v);
    if (eo.check_bits) {
      std::vector<std::vector<uint64_t>> c = p.mod[1].t[l];
      if (org.t_interleave) permute_pairs(L, org.t_interleave, kEccCheckBits, false, c);
      for (size_t pe = 0; pe < v.size(); pe++)
        for (size_t i = 0; i < v[pe].size(); i++) {
          uint32_t d;
          const int st = ecc_decode((uint32_t)v[pe][i], (uint32_t)c[pe][i], &d);
          v[pe][i] = d;
          if (status && st) status[l][st - 1]++;
        }
    }
    out.t[l] = v;
  }
}

namespace {
// the TMR repair of one memory: the low ebits of the three modules' words become their bitwise majority
void repair_voted(RawParams *mod, const RawParams *loaded, bool thresholds, int l, int ebits, long *counts) {
  auto mem = [&](RawParams &r) -> std::vector<std::vector<uint64_t>> & { return thresholds ? r.t[l] : r.w[l]; };
  const uint64_t emask = ebits >= 64 ? ~0ull : (1ull << ebits) - 1;
  for (size_t pe = 0; pe < mem(mod[0]).size(); pe++)
    for (size_t i = 0; i < mem(mod[0])[pe].size(); i++) {
      uint64_t *const w[3] = {&mem(mod[0])[pe][i], &mem(mod[1])[pe][i], &mem(mod[2])[pe][i]};
      const uint64_t v = ((*w[0] & *w[1]) | (*w[0] & *w[2]) | (*w[1] & *w[2])) & emask;
      bool wrote = false;
      for (int m = 0; m < 3; m++) {
        wrote = wrote || (*w[m] & emask) != v;
        *w[m] = (*w[m] & ~emask) | v;
      }
      if (counts && wrote) counts[0]++;
      if (counts && loaded && v != ((thresholds ? loaded[0].t[l] : loaded[0].w[l])[pe][i] & emask)) counts[1]++;
    }
}

// the bits of the logical element (line ind, threshold i) of one PE, gathered from / scattered to its physical sites
uint32_t gather(const LayerSpec &L, int il, int width, const std::vector<uint64_t> &pe, int ind, int i) {
  uint32_t v = 0;
  for (int k = 0; k < width; k++) {
    int pi, pb;
    interleave_site(il, width, L.fold.tmem, ind, k, &pi, &pb);
    v |= (uint32_t)((pe[(size_t)pi * L.nthr + i] >> pb) & 1) << k;
  }
  return v;
}
void scatter(const LayerSpec &L, int il, int width, std::vector<uint64_t> &pe, int ind, int i, uint32_t v) {
  for (int k = 0; k < width; k++) {
    int pi, pb;
    interleave_site(il, width, L.fold.tmem, ind, k, &pi, &pb);
    uint64_t &w = pe[(size_t)pi * L.nthr + i];
    w = (w & ~(1ull << pb)) | (uint64_t)((v >> k) & 1) << pb;
  }
}
}  // namespace

void phys_repair(const NetSpec &net, int scheme, int code, PhysParams &p, int l0, int l1, long (*counts)[2], const PhysParams *loaded,
                 int weight_code, long (*wcounts)[2], int weight_interleave) {
  for (int l = std::max(l0, p.l0); l < l1 && l < p.l1; l++) {
    const LayerSpec &L = net.L[l];
    EccOrg eo{MemOrg{1, 1, 0}, 0};
    if (counts) counts[l][0] = counts[l][1] = 0;
    if (wcounts) wcounts[l][0] = wcounts[l][1] = 0;
    if (!ecc_layout(net, scheme, code, l, eo).empty()) continue;
    if (const int cwpp = wecc_words_per_pe(net, weight_code, l)) {  // a coded weight memory, code word by code word
      const int ebits = mem_element_bits(L, 0);
      const int D = wecc_depth(net, weight_code, weight_interleave, l);
      for (size_t pe = 0; pe < p.mod[0].w[l].size(); pe++)
        for (int cw = 0; cw < cwpp; cw++) {
          uint64_t rd;
          uint32_t rc;
          const int st = wecc_repair(code_data(p.mod[0].w[l][pe], ebits, D, cw), code_check(p.mod[1].w[l][pe], D, cw), &rd, &rc);
          if (st == 1) {
            store_data(p.mod[0].w[l][pe], ebits, D, cw, rd);
            store_check(p.mod[1].w[l][pe], D, cw, rc);
            if (wcounts) wcounts[l][0]++;
          }
          if (wcounts && loaded && (rd != code_data(loaded->mod[0].w[l][pe], ebits, D, cw) || rc != code_check(loaded->mod[1].w[l][pe], D, cw)))
            wcounts[l][1]++;
        }
    }
    if (eo.org.w_modules == 3) repair_voted(p.mod, loaded ? loaded->mod : nullptr, false, l, mem_element_bits(L, 0), counts ? counts[l] : nullptr);
    if (L.nthr == 0) continue;
    if (!eo.check_bits) {
      if (eo.org.t_modules == 3) repair_voted(p.mod, loaded ? loaded->mod : nullptr, true, l, mem_element_bits(L, 1), counts ? counts[l] : nullptr);
      continue;
    }
    // a coded memory, element by element: its 16 data and 6 check bits lie where interleave_site puts them, and no other
    // element's do, so the order of the elements does not matter
    const int il = eo.org.t_interleave;
    for (size_t pe = 0; pe < p.mod[0].t[l].size(); pe++)
      for (int ind = 0; ind < L.fold.tmem; ind++)
        for (int i = 0; i < L.nthr; i++) {
          const uint32_t d = gather(L, il, kEccDataBits, p.mod[0].t[l][pe], ind, i), c = gather(L, il, kEccCheckBits, p.mod[1].t[l][pe], ind, i);
          uint32_t rd, rc;
          const int st = ecc_repair(d, c, &rd, &rc);
          if (st == 1) {
            scatter(L, il, kEccDataBits, p.mod[0].t[l][pe], ind, i, rd);
            scatter(L, il, kEccCheckBits, p.mod[1].t[l][pe], ind, i, rc);
            if (counts) counts[l][0]++;
          }
          if (counts && loaded &&
              (rd != gather(L, il, kEccDataBits, loaded->mod[0].t[l][pe], ind, i) || rc != gather(L, il, kEccCheckBits, loaded->mod[1].t[l][pe], ind, i)))
            counts[l][1]++;
        }
  }
}

std::string phys_replay(const NetSpec &net, int scheme, int code, const PhysParams &loaded, PhysParams &p, const int *records, int n,
                        int weight_code, int weight_interleave) {
  for (int i = 0; i < n; i++) {
    const int layer = records[(size_t)i * 9 + 2];
    if (layer < 0 && layer != kMarkRepair && layer != kMarkRewrite)
      return "record " + std::to_string(i) + ": layer " + std::to_string(layer) +
             " is no marker (-1: repair all memories now, -2: rewrite all memories from the loaded parameters now)";
  }
  for (int i = 0; i < n; i++) {
    const int *v = records + (size_t)i * 9;
    if (v[2] == kMarkRepair) {
      phys_repair(net, scheme, code, p, p.l0, p.l1, nullptr, nullptr, weight_code, nullptr, weight_interleave);
    } else if (v[2] == kMarkRewrite) {
      p = loaded;
    } else {
      const PhysFault pf{Fault{v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7]}, v[8]};
      if (phys_apply(net, scheme, p, pf, code, weight_code) < 0)
        return "record " + std::to_string(i) + ": fault record out of range (or a module the memory does not have)";
    }
  }
  return "";
}

long hardened_mem_noise_mask(const NetSpec &net, int scheme, int burst, uint64_t run_seed, int layer, int target, int module,
                             uint32_t rate_q32, long first, PhysFault *out, long cap, int epoch, int code, int weight_code,
                             int weight_interleave) {
  if (burst < 1 || burst > kMaxBurst || epoch < 0 || epoch >= kMaxEpochs) return -1;
  if (weight_interleave != WI_NONE && !iwecc_check(weight_code, weight_interleave).empty()) return -1;
  EccOrg eo{MemOrg{1, 1, 0}, 0};
  if (!ecc_layout(net, scheme, code, layer, eo).empty()) return -1;
  const MemOrg &org = eo.org;
  const bool check = target == 1 && module == 1 && eo.check_bits;  // the check memory: the same shape, 6 bits wide
  const int cwpp = target == 0 ? wecc_words_per_pe(net, weight_code, layer) : 0;
  const bool wcheck = cwpp && module == 1;  // the weight check memory: (PE, code word) shaped, 8 bits wide
  const long per_c = wcheck ? (long)wecc_check_groups(burst) : (long)ecc_check_groups(burst);
  const long events = wcheck  ? (long)net.L[layer].fold.pe * cwpp * per_c
                      : check ? (long)net.L[layer].fold.pe * net.L[layer].fold.tmem * net.L[layer].nthr * per_c
                              : enumerate_faults(net, layer, target, burst, 0, nullptr, 0);
  if (events < 0 || module < 0 || (!wcheck && module >= (target == 0 ? org.w_modules : org.t_modules))) return -1;
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
        if (wcheck) {
          const long el = (4 * b + e) / per_c;
          pf.f = Fault{};
          pf.f.bit = (int)((4 * b + e - el * per_c) * burst);
          pf.f.ind = (int)(el % cwpp);
          pf.f.mem = (int)(el / cwpp);
          pf.f.layer = layer;
          pf.f.target = 0;
          pf.f.word_size = burst;
        } else if (check) {
          const LayerSpec &L = net.L[layer];
          long el = (4 * b + e) / per_c;
          pf.f = Fault{};
          pf.f.bit = (int)((4 * b + e - el * per_c) * burst);
          pf.f.thresh = (int)(el % L.nthr);
          el /= L.nthr;
          pf.f.ind = (int)(el % L.fold.tmem);
          pf.f.mem = (int)(el / L.fold.tmem);
          pf.f.layer = layer;
          pf.f.target = 1;
          pf.f.word_size = burst;
        } else {
          enumerate_faults(net, layer, target, burst, 4 * b + e, &pf.f, 1);
        }
        pf.module = module;
        pf.f.image = epoch;
      }
      total++;
    }
  }
  return total;
}

}  // namespace bnn
