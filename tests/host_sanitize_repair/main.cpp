// Stand-alone driver for tests/test_host_sanitize_repair.py: the repair scrub's host code (csrc/mem_org.cpp: phys_repair,
// phys_replay -- the marker route of bnn_mi355x_pack_params_repair; csrc/ecc.h: ecc_repair) under AddressSanitizer + UBSan.
// argv[1]: the params root.  ecc_repair over every stored pair of one data word and a stride of them on three more; every supported (network, scheme,
// code): two epochs of events (bursts 1, 3, 16, every module, the check memories included) with a repair between and after
// them -- the delivered parameters are the same before and after a repair, a second repair rewrites nothing, the counts
// stay inside the memories -- then the marker stream through phys_replay against the same steps by hand, bad markers,
// bad records and layer ranges.
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

int main(int argc, char **argv) {
  CHECK(argc == 2);
  const std::string root = argv[1];
  for (uint32_t d : {0x0000u, 0xFFFFu, 0x1234u, 0x8001u})
    for (uint32_t s = 0; s < 64 * 65536; s += d == 0x1234u ? 1 : 13) {  // (one word under every error pattern, the others under a stride)
      uint32_t rd = ~0u, rc = ~0u, out = ~0u, again_d, again_c;
      const uint32_t sd = (d ^ s) & 0xFFFF, sc = ecc_encode(d) ^ (s >> 16);
      const int st = ecc_repair(sd, sc, &rd, &rc);
      CHECK(st == ecc_decode(sd, sc, &out) && rd < 65536 && rc < 64);
      if (st == 1) CHECK(rd == out && rc == ecc_encode(out));
      else CHECK(rd == sd && rc == sc);
      CHECK(ecc_repair(rd, rc, &again_d, &again_c) == (st == 2 ? 2 : 0) && again_d == rd && again_c == rc);
    }
  for (NetId id : {NET_CNVW1A1, NET_CNVW1A2, NET_CNVW2A2, NET_LFCW1A1, NET_LFCW1A2}) {
    const NetSpec &net = net_spec(id);
    RawParams raw;
    CHECK(read_raw_params(net, root + (net.is_cnv ? "/cifar10/" : "/mnist/") + net.name, raw).empty());
    for (int scheme = 0; scheme <= 3; scheme++)
      for (int code = 0; code <= 1; code++) {
        EccOrg eo;
        if (!ecc_layout(net, scheme, code, 0, eo).empty()) continue;
        PhysParams loaded, phys;
        phys_load(net, scheme, raw, 0, net.nlayers, loaded, code);
        phys = loaded;
        long counts[9][2], words[9] = {};
        bool redundancy = false;
        for (int l = 0; l < net.nlayers; l++) {
          CHECK(ecc_layout(net, scheme, code, l, eo).empty());
          const long t_words = (long)net.L[l].fold.pe * net.L[l].fold.tmem * net.L[l].nthr;
          if (eo.org.w_modules == 3) words[l] += (long)net.L[l].fold.pe * net.L[l].fold.wmem;
          if (eo.org.t_modules == 3 || eo.check_bits) words[l] += t_words;
          redundancy = redundancy || words[l] > 0;
        }
        phys_repair(net, scheme, code, phys, 0, net.nlayers, counts, &loaded);  // nothing to repair yet
        for (int l = 0; l < net.nlayers; l++) CHECK(counts[l][0] == 0 && counts[l][1] == 0);
        std::vector<int> stream;
        long rewritten = 0, left = 0;
        for (int epoch : {0, 1})
          for (int burst : {1, 3, 16}) {
            std::vector<PhysFault> all;
            for (int l = 0; l < net.nlayers; l++) {
              CHECK(ecc_layout(net, scheme, code, l, eo).empty());
              for (int target = 0; target < 2; target++)
                for (int m = 0; m < (target ? eo.org.t_modules : eo.org.w_modules); m++) {
                  const uint32_t rate = target == 0 && eo.org.w_modules == 1 ? 1u << 20 : 1u << 28;
                  const long k = hardened_mem_noise_mask(net, scheme, burst, 91, l, target, m, rate, 0, nullptr, 0, epoch, code);
                  CHECK(k >= 0);
                  std::vector<PhysFault> ev((size_t)k);
                  CHECK(hardened_mem_noise_mask(net, scheme, burst, 91, l, target, m, rate, 0, ev.data(), k, epoch, code) == k);
                  all.insert(all.end(), ev.begin(), ev.end());
                }
            }
            for (const PhysFault &pf : all) CHECK(phys_apply(net, scheme, phys, pf, code) >= 0);
            const std::vector<int> recs = records_of(all);
            stream.insert(stream.end(), recs.begin(), recs.end());
            RawParams before = raw, after = raw;
            phys_logical(net, scheme, phys, before, code);
            phys_repair(net, scheme, code, phys, 0, net.nlayers, counts, &loaded);
            stream.insert(stream.end(), {0, 0, kMarkRepair, 0, 0, 0, 0, 0, 0});
            phys_logical(net, scheme, phys, after, code);
            for (int l = 0; l < net.nlayers; l++) {
              CHECK(before.w[l] == after.w[l] && before.t[l] == after.t[l]);  // the delivered parameters do not change
              CHECK(counts[l][0] >= 0 && counts[l][0] <= words[l] && counts[l][1] >= 0 && counts[l][1] <= words[l]);
              rewritten += counts[l][0];
              left += counts[l][1];
            }
            long again[9][2];
            PhysParams twice = phys;
            phys_repair(net, scheme, code, twice, 0, net.nlayers, again, &loaded);
            for (int l = 0; l < net.nlayers; l++) {
              CHECK(again[l][0] == 0 && again[l][1] == counts[l][1]);
              for (int m = 0; m < 3; m++) CHECK(twice.mod[m].w[l] == phys.mod[m].w[l] && twice.mod[m].t[l] == phys.mod[m].t[l]);
            }
          }
        CHECK(redundancy ? rewritten > 0 && left > 0 : rewritten == 0 && left == 0);
        // the same steps as a marker stream
        PhysParams replayed = loaded;
        CHECK(phys_replay(net, scheme, code, loaded, replayed, stream.data(), (int)(stream.size() / 9)).empty());
        for (int l = 0; l < net.nlayers; l++)
          for (int m = 0; m < 3; m++) CHECK(replayed.mod[m].w[l] == phys.mod[m].w[l] && replayed.mod[m].t[l] == phys.mod[m].t[l]);
        stream.insert(stream.end(), {7, 7, kMarkRewrite, 7, 7, 7, 7, 7, 7});
        CHECK(phys_replay(net, scheme, code, loaded, replayed, stream.data(), (int)(stream.size() / 9)).empty());
        for (int l = 0; l < net.nlayers; l++)
          for (int m = 0; m < 3; m++) CHECK(replayed.mod[m].w[l] == loaded.mod[m].w[l] && replayed.mod[m].t[l] == loaded.mod[m].t[l]);
        CHECK(phys_replay(net, scheme, code, loaded, replayed, nullptr, 0).empty());
        for (int bad : {-3, -1000, (int)0x80000000}) {
          const int recs[18] = {0, 0, kMarkRepair, 0, 0, 0, 0, 0, 0, 0, 0, bad, 0, 0, 0, 0, 0, 0};
          CHECK(phys_replay(net, scheme, code, loaded, replayed, recs, 2).rfind("record 1: layer ", 0) == 0);
        }
        const int outside[18] = {0, 0, kMarkRewrite, 0, 0, 0, 0, 0, 0, 0, 1, net.nlayers, 0, 0, 0, 0, 1, 0};
        CHECK(phys_replay(net, scheme, code, loaded, replayed, outside, 2).rfind("record 1: fault record out of range", 0) == 0);
        // a part of the layers, a range past the state, no counts
        PhysParams part;
        phys_load(net, scheme, raw, 0, 1, part, code);
        phys_repair(net, scheme, code, part, 0, net.nlayers, nullptr);
        phys_repair(net, scheme, code, part, 0, 1, counts, nullptr);
        phys_repair(net, scheme, code, phys, net.nlayers - 1, net.nlayers, nullptr, &loaded);
        phys_repair(net, scheme, code, phys, 2, 1, counts);
      }
  }
  std::printf("repair sanitize run ok\n");
  return 0;
}
