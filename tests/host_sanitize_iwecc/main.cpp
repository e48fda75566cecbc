// Stand-alone driver for tests/test_host_sanitize_iwecc.py: the column-interleaved coded weight memories' host code
// (csrc/mem_org.cpp: wecc_depth, iwecc_site / iwecc_site_of, phys_load, phys_logical, phys_repair and phys_replay with
// weight_interleave 1 -- the route of bnn_mi355x_pack_params_iwecc, down to pack_blob) and the kernels' bit exchange
// (csrc/iwecc.h: unzip, zip, the butterfly's stages, the check offsets) under AddressSanitizer + UBSan.
// argv[1]: the params root.
//   The exchange, with an array of 64 lanes where the device has __shfl_xor: at every depth 1 ... 16 the unzip and the
//   stages give code word c of a group bit i * (64 / D) + j = lane i's bit j * D + c -- the membership of mem_org.h --, the
//   way back restores the lanes, and the check offsets are each other's inverse and the membership's.
//   Every net, every coded layer: depth = gcd(16, code words per PE); the site map and its inverse over both memories (whole
//   for the small layers, strided for the large ones), no group across PEs; the loaded image decodes clean; two epochs of
//   events (bursts 1, 2, 16, both memories) with a repair between and after them: the delivered weights are the same before
//   and after a repair, a second repair rewrites nothing, the counts stay inside the memories; a single event of width <= D
//   is corrected; the marker stream through phys_replay against the steps by hand and on through pack_blob; weight_interleave
//   0 is weight_code 1's route, word for word.
#include <cstdio>
#include <string>
#include <vector>

#include "iwecc.h"
#include "mem_org.h"

using namespace bnn;

#define CHECK(x) do { if (!(x)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

static uint64_t rnd(uint64_t &s) {
  s ^= s << 13; s ^= s >> 7; s ^= s << 17;
  return s;
}

static std::vector<int> records_of(const std::vector<PhysFault> &ev) {
  std::vector<int> out;
  for (const PhysFault &pf : ev) {
    const Fault &f = pf.f;
    for (int v : {f.image, f.target, f.layer, f.mem, f.ind, f.thresh, f.bit, f.word_size, pf.module}) out.push_back(v);
  }
  return out;
}

// one butterfly stage over all 64 lanes
template <int LOGD, int S>
static void stage_all(uint64_t *x) {
  uint64_t y[64];
  for (unsigned l = 0; l < 64; l++) y[l] = iwecc_stage<LOGD, S>(x[l], x[l ^ (1u << S)], (l >> S) & 1u);
  for (unsigned l = 0; l < 64; l++) x[l] = y[l];
}
template <int LOGD>
static void transpose_all(uint64_t *x) {
  if constexpr (LOGD > 0) stage_all<LOGD, 0>(x);
  if constexpr (LOGD > 1) stage_all<LOGD, 1>(x);
  if constexpr (LOGD > 2) stage_all<LOGD, 2>(x);
  if constexpr (LOGD > 3) stage_all<LOGD, 3>(x);
}

template <int LOGD>
static int check_exchange(uint64_t seed) {
  constexpr int D = 1 << LOGD;
  uint64_t phys[64], x[64];
  uint32_t cphys[64], cw[64], back[64];
  for (int trial = 0; trial < 8; trial++) {
    for (int l = 0; l < 64; l++) {
      phys[l] = trial == 0 ? 1ull << l : rnd(seed);
      cphys[l] = (uint32_t)(rnd(seed) & 0xFF);
      x[l] = iwecc_unzip<LOGD>(phys[l]);
      CHECK(iwecc_zip<LOGD>(x[l]) == phys[l]);
    }
    transpose_all<LOGD>(x);
    for (int l = 0; l < 64; l++) {  // lane l now holds code word l % D of group l / D
      const int base = l & ~(D - 1), c = l & (D - 1);
      uint64_t want = 0;
      for (int p = 0; p < 64 * D; p++) {  // the membership, from the model's text
        int w, b;
        iwecc_member(D, p, &w, &b);
        CHECK(iwecc_offset(D, w, b) == p);
        if (w == c) want |= ((phys[base + p / 64] >> (p % 64)) & 1) << b;
      }
      CHECK(x[l] == want);
      uint32_t cwant = 0;
      for (int r = 0; r < 8 * D; r++) {
        int w, b;
        iwecc_member(D, r, &w, &b);
        if (w == c) cwant |= ((cphys[base + r / 8] >> (r % 8)) & 1u) << b;
      }
      cw[l] = 0;
      for (unsigned k = 0; k < 8; k++) {
        unsigned el, b, w2, k2;
        iwecc_check_source((unsigned)D, (unsigned)c, k, &el, &b);
        CHECK(el < (unsigned)D && b < 8);
        iwecc_check_target((unsigned)D, el, b, &w2, &k2);
        CHECK(w2 == (unsigned)c && k2 == k);
        cw[l] |= ((cphys[base + el] >> b) & 1u) << k;
      }
      CHECK(cw[l] == cwant);
    }
    for (int l = 0; l < 64; l++) {
      const int base = l & ~(D - 1);
      back[l] = 0;
      for (unsigned b = 0; b < 8; b++) {
        unsigned c, k;
        iwecc_check_target((unsigned)D, (unsigned)(l & (D - 1)), b, &c, &k);
        CHECK(c < (unsigned)D && k < 8);
        back[l] |= ((cw[base + c] >> k) & 1u) << b;
      }
      CHECK(back[l] == cphys[l]);
    }
    transpose_all<LOGD>(x);
    for (int l = 0; l < 64; l++) CHECK(iwecc_zip<LOGD>(x[l]) == phys[l]);
  }
  return 0;
}

static int gcd(int a, int b) { return b ? gcd(b, a % b) : a; }

int main(int argc, char **argv) {
  CHECK(argc == 2);
  const std::string root = argv[1];
  CHECK(check_exchange<0>(11) == 0 && check_exchange<1>(12) == 0 && check_exchange<2>(13) == 0 && check_exchange<3>(14) == 0 &&
        check_exchange<4>(15) == 0);
  CHECK(iwecc_check(0, 0).empty() && iwecc_check(1, 0).empty() && iwecc_check(1, 1).empty());
  CHECK(iwecc_check(0, 1) == "weight_interleave 1 needs weight_code 1" && iwecc_check(2, 0) == wecc_check(2) && iwecc_check(2, 1) == wecc_check(2));
  CHECK(iwecc_check(1, 2) == "weight_interleave must be 0 (none) or 1 (column-interleaved code words)" && iwecc_check(1, -1) == iwecc_check(1, 2));
  const int wc = WC_SECDED, wi = WI_COLUMNS;
  for (NetId id : {NET_CNVW1A1, NET_CNVW1A2, NET_CNVW2A2, NET_LFCW1A1, NET_LFCW1A2}) {
    const NetSpec &net = net_spec(id);
    RawParams raw;
    CHECK(read_raw_params(net, root + (net.is_cnv ? "/cifar10/" : "/mnist/") + net.name, raw).empty());
    long words[9] = {};
    int depth[9] = {};
    for (int l = 0; l < net.nlayers; l++) {
      const int cwpp = wecc_words_per_pe(net, wc, l);
      depth[l] = wecc_depth(net, wc, wi, l);
      words[l] = (long)cwpp * net.L[l].fold.pe;
      CHECK(wecc_depth(net, WC_NONE, WI_NONE, l) == 0 && wecc_depth(net, wc, WI_NONE, l) == (cwpp ? 1 : 0));
      CHECK(depth[l] == (cwpp ? gcd(kMaxBurst, cwpp) : 0));
      long w;
      int b;
      if (!cwpp) {
        CHECK(!iwecc_site(net, wc, wi, l, 0, 0, &w, &b) && iwecc_site_of(net, wc, wi, l, 0, 0, 0) == -1);
        continue;
      }
      CHECK(cwpp % depth[l] == 0 && depth[l] >= 2);  // (in the five nets: never 1)
      for (int module = 0; module < 2; module++) {
        const long per = module ? kWeccCheckBits : kWeccDataBits, n = words[l] * per;
        const long step = n <= (1 << 16) ? 1 : 61;  // (whole for the small memories)
        for (long s = 0; s < n; s += step) {
          CHECK(iwecc_site(net, wc, wi, l, module, s, &w, &b) && w >= 0 && w < words[l] && b >= 0 && b < per);
          CHECK(iwecc_site_of(net, wc, wi, l, module, w, b) == s);
          CHECK(w / cwpp == s / (per * cwpp));  // the code word lies in the site's own PE
          long w0;
          int b0;
          CHECK(iwecc_site(net, wc, WI_NONE, l, module, s, &w0, &b0) && w0 == s / per && b0 == s % per);
        }
        CHECK(!iwecc_site(net, wc, wi, l, module, n, &w, &b) && !iwecc_site(net, wc, wi, l, module, -1, &w, &b) &&
              !iwecc_site(net, wc, wi, l, 2, 0, &w, &b));
        CHECK(iwecc_site_of(net, wc, wi, l, module, words[l], 0) == -1 && iwecc_site_of(net, wc, wi, l, module, 0, (int)per) == -1);
      }
    }
    for (int scheme = 0; scheme <= 3; scheme++)
      for (int code = 0; code <= 1; code++) {
        EccOrg eo;
        if (!ecc_layout(net, scheme, code, 0, eo).empty()) continue;
        // (the interleave is orthogonal to scheme and code, which tests/host_sanitize_wecc walks in full: none, TMR, and an
        // interleaved coded threshold memory next to it are enough here)
        if (!((scheme == 0 && code == 0) || (scheme == 1 && code == 0) || (scheme == 2 && code == 1))) continue;
        PhysParams loaded, plain, phys;
        phys_load(net, scheme, raw, 0, net.nlayers, loaded, code, wc, wi);
        phys_load(net, scheme, raw, 0, net.nlayers, plain, code, wc, WI_NONE);
        long counts[9][2], wcounts[9][2], wst[9][2];
        RawParams clean = raw;
        phys_logical(net, scheme, loaded, clean, code, nullptr, wc, wst, wi);
        for (int l = 0; l < net.nlayers; l++) {
          CHECK(loaded.mod[0].w[l] == plain.mod[0].w[l] && wst[l][0] == 0 && wst[l][1] == 0);  // the weights stay where they were
          CHECK(loaded.mod[1].w[l].size() == plain.mod[1].w[l].size());
          for (size_t pe = 0; words[l] && pe < loaded.mod[1].w[l].size(); pe++)
            for (uint64_t v : loaded.mod[1].w[l][pe]) CHECK(v < 256);
        }
        phys = loaded;
        phys_repair(net, scheme, code, phys, 0, net.nlayers, counts, &loaded, wc, wcounts, wi);  // nothing to repair yet
        for (int l = 0; l < net.nlayers; l++) CHECK(wcounts[l][0] == 0 && wcounts[l][1] == 0);
        std::vector<int> stream;
        long rewritten = 0, left = 0;
        for (int epoch : {0, 1})
          for (int burst : {1, 2, 16}) {
            std::vector<PhysFault> all;
            for (int l = 0; l < net.nlayers; l++) {
              if (!words[l]) continue;  // (the other memories: tests/host_sanitize_wecc)
              for (int m = 0; m < 2; m++) {
                const uint32_t rate = 1u << 24;
                const long k = hardened_mem_noise_mask(net, scheme, burst, 93, l, 0, m, rate, 0, nullptr, 0, epoch, code, wc, wi);
                CHECK(k >= 0 && k == hardened_mem_noise_mask(net, scheme, burst, 93, l, 0, m, rate, 0, nullptr, 0, epoch, code, wc));
                std::vector<PhysFault> ev((size_t)k);
                CHECK(hardened_mem_noise_mask(net, scheme, burst, 93, l, 0, m, rate, 0, ev.data(), k, epoch, code, wc, wi) == k);
                all.insert(all.end(), ev.begin(), ev.end());
              }
              CHECK(hardened_mem_noise_mask(net, scheme, burst, 93, l, 0, 0, 1u << 24, 0, nullptr, 0, epoch, code, WC_NONE, wi) == -1);
              CHECK(hardened_mem_noise_mask(net, scheme, burst, 93, l, 0, 0, 1u << 24, 0, nullptr, 0, epoch, code, wc, 2) == -1);
            }
            for (const PhysFault &pf : all) CHECK(phys_apply(net, scheme, phys, pf, code, wc) >= 0);
            const std::vector<int> recs = records_of(all);
            stream.insert(stream.end(), recs.begin(), recs.end());
            RawParams before = raw, after = raw;
            phys_logical(net, scheme, phys, before, code, nullptr, wc, wst, wi);
            phys_repair(net, scheme, code, phys, 0, net.nlayers, counts, &loaded, wc, wcounts, wi);
            stream.insert(stream.end(), {0, 0, kMarkRepair, 0, 0, 0, 0, 0, 0});
            phys_logical(net, scheme, phys, after, code, nullptr, wc, nullptr, wi);
            for (int l = 0; l < net.nlayers; l++) {
              CHECK(before.w[l] == after.w[l] && before.t[l] == after.t[l]);  // the delivered parameters do not change
              CHECK(wst[l][0] >= 0 && wst[l][1] >= 0 && wst[l][0] + wst[l][1] <= words[l]);
              CHECK(wcounts[l][0] == wst[l][0] && wcounts[l][1] >= wst[l][1] && wcounts[l][1] <= words[l]);
              rewritten += wcounts[l][0];
              left += wcounts[l][1];
            }
            long again[9][2], wagain[9][2];
            PhysParams twice = phys;
            phys_repair(net, scheme, code, twice, 0, net.nlayers, again, &loaded, wc, wagain, wi);
            for (int l = 0; l < net.nlayers; l++) {
              CHECK(wagain[l][0] == 0 && wagain[l][1] == wcounts[l][1]);
              for (int m = 0; m < 3; m++) CHECK(twice.mod[m].w[l] == phys.mod[m].w[l] && twice.mod[m].t[l] == phys.mod[m].t[l]);
            }
          }
        CHECK(rewritten > 0 && left > 0);
        // the same steps as a marker stream, and on to the blob: the route of bnn_mi355x_pack_params_iwecc
        PhysParams replayed = loaded;
        CHECK(phys_replay(net, scheme, code, loaded, replayed, stream.data(), (int)(stream.size() / 9), wc, wi).empty());
        for (int l = 0; l < net.nlayers; l++)
          for (int m = 0; m < 3; m++) CHECK(replayed.mod[m].w[l] == phys.mod[m].w[l] && replayed.mod[m].t[l] == phys.mod[m].t[l]);
        RawParams logical = raw;
        phys_logical(net, scheme, replayed, logical, code, nullptr, wc, nullptr, wi);
        std::vector<uint8_t> blob, cleanb;
        pack_blob(net, logical, blob);
        pack_blob(net, raw, cleanb);
        CHECK(blob.size() == cleanb.size() && blob != cleanb);
        stream.insert(stream.end(), {7, 7, kMarkRewrite, 7, 7, 7, 7, 7, 7});
        CHECK(phys_replay(net, scheme, code, loaded, replayed, stream.data(), (int)(stream.size() / 9), wc, wi).empty());
        for (int l = 0; l < net.nlayers; l++)
          for (int m = 0; m < 3; m++) CHECK(replayed.mod[m].w[l] == loaded.mod[m].w[l] && replayed.mod[m].t[l] == loaded.mod[m].t[l]);
        // one event of width 1, 2 and D, first and last group of the layer, both memories: corrected, and repaired to the loaded state
        for (int l = 0; l < net.nlayers; l++) {
          if (!words[l]) continue;
          const LayerSpec &L = net.L[l];
          const int ebits = mem_element_bits(L, 0), cwpp = wecc_words_per_pe(net, wc, l);
          PhysParams lone;  // (this layer's memories alone)
          phys_load(net, scheme, raw, l, l + 1, lone, code, wc, wi);
          for (int b = 1; b <= depth[l] && b <= kMaxBurst; b = b < 2 ? b + 1 : b < depth[l] ? depth[l] : b + 1)
            for (int m = 0; m < 2; m++)
              for (int last = 0; last < 2; last++) {
                const int eb = m ? kWeccCheckBits : ebits;
                if (b > eb) continue;
                PhysFault pf{Fault{}, m};
                pf.f.layer = l;
                pf.f.mem = last ? L.fold.pe - 1 : 0;
                pf.f.ind = last ? (m ? cwpp : L.fold.wmem) - 1 : 0;
                pf.f.bit = (eb - 1) / b * b;  // the last group of the element (clipped where b does not divide it)
                pf.f.word_size = b;
                PhysParams one = lone;
                CHECK(phys_apply(net, scheme, one, pf, code, wc) >= 0);
                RawParams got = raw;
                phys_logical(net, scheme, one, got, code, nullptr, wc, wst, wi);
                CHECK(got.w[l] == clean.w[l] && wst[l][1] == 0 && wst[l][0] >= 1 && wst[l][0] <= b);
                phys_repair(net, scheme, code, one, l, l + 1, nullptr, &lone, wc, wcounts, wi);
                CHECK(wcounts[l][0] == wst[l][0] && wcounts[l][1] == 0 && one.mod[0].w[l] == loaded.mod[0].w[l] && one.mod[1].w[l] == loaded.mod[1].w[l]);
              }
        }
        // weight_interleave 0 is weight_code 1's route
        PhysParams a = plain, bb = plain;
        CHECK(phys_replay(net, scheme, code, plain, a, stream.data(), (int)(stream.size() / 9) - 1, wc).empty());
        CHECK(phys_replay(net, scheme, code, plain, bb, stream.data(), (int)(stream.size() / 9) - 1, wc, WI_NONE).empty());
        for (int l = 0; l < net.nlayers; l++)
          for (int m = 0; m < 3; m++) CHECK(a.mod[m].w[l] == bb.mod[m].w[l] && a.mod[m].t[l] == bb.mod[m].t[l]);
      }
  }
  std::printf("iwecc sanitize run ok\n");
  return 0;
}
