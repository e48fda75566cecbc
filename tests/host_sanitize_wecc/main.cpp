// Stand-alone driver for tests/test_host_sanitize_wecc.py: the coded weight memories' host code (csrc/mem_org.cpp: phys_load,
// phys_apply, phys_logical, phys_repair and phys_replay with the weight check memory -- the route of
// bnn_mi355x_pack_params_wecc, down to pack_blob; csrc/wecc.h) under AddressSanitizer + UBSan.
// argv[1]: the params root.  wecc_repair over every error pattern of weight <= 2 and a stride of triples; every supported
// (network, scheme, code) with weight_code 1: two epochs of events (bursts 1, 3, 16, every module, both kinds of check
// memories included) with a repair between and after them -- the delivered parameters are the same before and after a
// repair, a second repair rewrites nothing, the counts stay inside the memories -- then the marker stream through
// phys_replay against the same steps by hand and through pack_blob; records outside the check memory; weight_code 0
// leaves no check memory and refuses its records.
#include <cstdio>
#include <string>
#include <vector>

#include "mem_org.h"

using namespace bnn;

#define CHECK(x) do { if (!(x)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

static std::vector<int> records_of(const std::vector<PhysFault> &ev) {
  std::vector<int> out;
  for (const PhysFault &pf : ev) {
    const Fault &f = pf.f;
    for (int v : {f.image, f.target, f.layer, f.mem, f.ind, f.thresh, f.bit, f.word_size, pf.module}) out.push_back(v);
  }
  return out;
}

static int check_pattern(uint64_t d, uint64_t dm, uint32_t cm, int weight) {
  uint64_t out = ~0ull, rd = ~0ull, again_d;
  uint32_t rc = ~0u, again_c;
  const uint64_t sd = d ^ dm;
  const uint32_t sc = wecc_encode(d) ^ cm;
  const int st = wecc_repair(sd, sc, &rd, &rc);
  CHECK(st == wecc_decode(sd, sc, &out) && rc < 256);
  if (weight == 0) CHECK(st == 0 && out == d);
  if (weight == 1) CHECK(st == 1 && out == d && rd == d && rc == wecc_encode(d));
  if (weight == 2) CHECK(st == 2 && out == sd && rd == sd && rc == sc);
  if (st == 1) CHECK(rd == out && rc == wecc_encode(out));
  else CHECK(rd == sd && rc == sc);
  CHECK(wecc_repair(rd, rc, &again_d, &again_c) == (st == 2 ? 2 : 0) && again_d == rd && again_c == rc);
  return 0;
}

int main(int argc, char **argv) {
  CHECK(argc == 2);
  const std::string root = argv[1];
  for (uint64_t d : {0ull, ~0ull, 0x0123456789ABCDEFull, 0x8000000000000001ull}) {
    CHECK(check_pattern(d, 0, 0, 0) == 0);
    for (int a = 0; a < 72; a++) {
      const uint64_t da = a < 64 ? 1ull << a : 0;
      const uint32_t ca = a < 64 ? 0 : 1u << (a - 64);
      CHECK(check_pattern(d, da, ca, 1) == 0);
      for (int b = a + 1; b < 72; b++) {
        const uint64_t db = da | (b < 64 ? 1ull << b : 0);
        const uint32_t cb = ca | (b < 64 ? 0 : 1u << (b - 64));
        CHECK(check_pattern(d, db, cb, 2) == 0);
        for (int c = b + 1; c < 72; c += 5) CHECK(check_pattern(d, db | (c < 64 ? 1ull << c : 0), cb | (c < 64 ? 0 : 1u << (c - 64)), 3) == 0);
      }
    }
  }
  for (NetId id : {NET_CNVW1A1, NET_CNVW1A2, NET_CNVW2A2, NET_LFCW1A1, NET_LFCW1A2}) {
    const NetSpec &net = net_spec(id);
    RawParams raw;
    CHECK(read_raw_params(net, root + (net.is_cnv ? "/cifar10/" : "/mnist/") + net.name, raw).empty());
    CHECK(!wecc_check(-1).empty() && !wecc_check(2).empty() && wecc_check(0).empty() && wecc_check(1).empty());
    for (int scheme = 0; scheme <= 3; scheme++)
      for (int code = 0; code <= 1; code++) {
        EccOrg eo;
        if (!ecc_layout(net, scheme, code, 0, eo).empty()) continue;
        const int wc = WC_SECDED;
        PhysParams loaded, phys;
        phys_load(net, scheme, raw, 0, net.nlayers, loaded, code, wc);
        phys = loaded;
        long counts[9][2], wcounts[9][2], words[9] = {};
        for (int l = 0; l < net.nlayers; l++) {
          const int cwpp = wecc_words_per_pe(net, wc, l);
          CHECK((cwpp == 0) == (net.is_cnv && l == 0) && wecc_words_per_pe(net, WC_NONE, l) == 0);
          words[l] = (long)cwpp * net.L[l].fold.pe;
          CHECK(cwpp == 0 || ((long)cwpp * 64 == (long)net.L[l].fold.wmem * mem_element_bits(net.L[l], 0) && loaded.mod[1].w[l].size() == (size_t)net.L[l].fold.pe));
          if (!cwpp && ecc_layout(net, scheme, code, l, eo).empty() && eo.org.w_modules == 1) CHECK(loaded.mod[1].w[l].empty());
        }
        phys_repair(net, scheme, code, phys, 0, net.nlayers, counts, &loaded, wc, wcounts);  // nothing to repair yet
        for (int l = 0; l < net.nlayers; l++) CHECK(counts[l][0] == 0 && counts[l][1] == 0 && wcounts[l][0] == 0 && wcounts[l][1] == 0);
        std::vector<int> stream;
        long rewritten = 0, left = 0;
        for (int epoch : {0, 1})
          for (int burst : {1, 3, 16}) {
            std::vector<PhysFault> all;
            for (int l = 0; l < net.nlayers; l++) {
              CHECK(ecc_layout(net, scheme, code, l, eo).empty());
              for (int target = 0; target < 2; target++) {
                const int modules = target ? eo.org.t_modules : eo.org.w_modules + (words[l] ? 1 : 0);
                for (int m = 0; m < modules; m++) {
                  const uint32_t rate = 1u << 25;
                  const long k = hardened_mem_noise_mask(net, scheme, burst, 91, l, target, m, rate, 0, nullptr, 0, epoch, code, wc);
                  CHECK(k >= 0);
                  std::vector<PhysFault> ev((size_t)k);
                  CHECK(hardened_mem_noise_mask(net, scheme, burst, 91, l, target, m, rate, 0, ev.data(), k, epoch, code, wc) == k);
                  all.insert(all.end(), ev.begin(), ev.end());
                }
                // (a module past the last one, and the check memory without the code, are refused)
                CHECK(hardened_mem_noise_mask(net, scheme, burst, 91, l, target, modules, 1u << 25, 0, nullptr, 0, epoch, code, wc) == -1);
              }
              if (words[l]) CHECK(hardened_mem_noise_mask(net, scheme, burst, 91, l, 0, 1, 1u << 25, 0, nullptr, 0, epoch, code, WC_NONE) == -1);
            }
            for (const PhysFault &pf : all) CHECK(phys_apply(net, scheme, phys, pf, code, wc) >= 0);
            const std::vector<int> recs = records_of(all);
            stream.insert(stream.end(), recs.begin(), recs.end());
            RawParams before = raw, after = raw;
            long wst[9][2];
            phys_logical(net, scheme, phys, before, code, nullptr, wc, wst);
            phys_repair(net, scheme, code, phys, 0, net.nlayers, counts, &loaded, wc, wcounts);
            stream.insert(stream.end(), {0, 0, kMarkRepair, 0, 0, 0, 0, 0, 0});
            phys_logical(net, scheme, phys, after, code, nullptr, wc);
            for (int l = 0; l < net.nlayers; l++) {
              CHECK(before.w[l] == after.w[l] && before.t[l] == after.t[l]);  // the delivered parameters do not change
              CHECK(wst[l][0] >= 0 && wst[l][1] >= 0 && wst[l][0] + wst[l][1] <= words[l]);
              CHECK(wcounts[l][0] == wst[l][0] && wcounts[l][1] >= wst[l][1] && wcounts[l][1] <= words[l]);
              rewritten += wcounts[l][0];
              left += wcounts[l][1];
            }
            long again[9][2], wagain[9][2];
            PhysParams twice = phys;
            phys_repair(net, scheme, code, twice, 0, net.nlayers, again, &loaded, wc, wagain);
            for (int l = 0; l < net.nlayers; l++) {
              CHECK(wagain[l][0] == 0 && wagain[l][1] == wcounts[l][1]);
              for (int m = 0; m < 3; m++) CHECK(twice.mod[m].w[l] == phys.mod[m].w[l] && twice.mod[m].t[l] == phys.mod[m].t[l]);
            }
          }
        CHECK(rewritten > 0 && left > 0);
        // the same steps as a marker stream, and on to the blob: the route of bnn_mi355x_pack_params_wecc
        PhysParams replayed = loaded;
        CHECK(phys_replay(net, scheme, code, loaded, replayed, stream.data(), (int)(stream.size() / 9), wc).empty());
        for (int l = 0; l < net.nlayers; l++)
          for (int m = 0; m < 3; m++) CHECK(replayed.mod[m].w[l] == phys.mod[m].w[l] && replayed.mod[m].t[l] == phys.mod[m].t[l]);
        RawParams logical = raw;
        phys_logical(net, scheme, replayed, logical, code, nullptr, wc);
        std::vector<uint8_t> blob, clean;
        pack_blob(net, logical, blob);
        pack_blob(net, raw, clean);
        CHECK(blob.size() == clean.size() && blob != clean);
        stream.insert(stream.end(), {7, 7, kMarkRewrite, 7, 7, 7, 7, 7, 7});
        CHECK(phys_replay(net, scheme, code, loaded, replayed, stream.data(), (int)(stream.size() / 9), wc).empty());
        for (int l = 0; l < net.nlayers; l++)
          for (int m = 0; m < 3; m++) CHECK(replayed.mod[m].w[l] == loaded.mod[m].w[l] && replayed.mod[m].t[l] == loaded.mod[m].t[l]);
        // the stream holds check-memory records: without the weight code they are refused, by record number
        CHECK(phys_replay(net, scheme, code, loaded, replayed, stream.data(), (int)(stream.size() / 9), WC_NONE).rfind("record ", 0) == 0);
        // records outside the check memory
        const int last = net.nlayers - 1, cwpp = wecc_words_per_pe(net, wc, last);
        for (const PhysFault &pf : {PhysFault{Fault{0, 0, last, net.L[last].fold.pe, 0, 0, 0, 1}, 1}, PhysFault{Fault{0, 0, last, 0, cwpp, 0, 0, 1}, 1},
                                    PhysFault{Fault{0, 0, last, 0, 0, 0, 8, 1}, 1}, PhysFault{Fault{0, 0, last, 0, -1, 0, 0, 1}, 1},
                                    PhysFault{Fault{0, 0, last, 0, 0, 0, 0, 0}, 1}, PhysFault{Fault{0, 0, last, 0, 0, 0, 0, 1}, 2}})
          CHECK(phys_apply(net, scheme, replayed, pf, code, wc) == -1);
        CHECK(phys_apply(net, scheme, replayed, PhysFault{Fault{0, 0, last, 0, cwpp - 1, 0, 7, 16}, 1}, code, wc) >= 0);  // (clipped to the 8 bits)
        CHECK(replayed.mod[1].w[last][0][(size_t)cwpp - 1] < 256);
        // a part of the layers, a range past the state, no counts
        PhysParams part;
        phys_load(net, scheme, raw, 0, 1, part, code, wc);
        phys_repair(net, scheme, code, part, 0, net.nlayers, nullptr, nullptr, wc);
        phys_repair(net, scheme, code, part, 0, 1, counts, nullptr, wc, wcounts);
        phys_repair(net, scheme, code, phys, net.nlayers - 1, net.nlayers, nullptr, &loaded, wc, wcounts);
        phys_repair(net, scheme, code, phys, 2, 1, counts, nullptr, wc);
      }
  }
  std::printf("wecc sanitize run ok\n");
  return 0;
}
