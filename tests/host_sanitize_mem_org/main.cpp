// Stand-alone driver for tests/test_host_sanitize_mem_org.py: the memory-organisation model (csrc/mem_org.cpp) under
// AddressSanitizer + UBSan.  argv[1]: the params root.  Every supported (network, scheme): the loader's physical state
// gives back the files' blob; a run's events (bursts 3, 4 and 16, every module) applied and voted / de-interleaved;
// the mapping function and its inverse over an odd line count; the refusals.
#include <cstdio>
#include <string>
#include <vector>

#include "mem_org.h"

using namespace bnn;

#define CHECK(x) do { if (!(x)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

int main(int argc, char **argv) {
  CHECK(argc == 2);
  const std::string root = argv[1];
  for (NetId id : {NET_CNVW1A1, NET_CNVW1A2, NET_CNVW2A2, NET_LFCW1A1, NET_LFCW1A2}) {
    const NetSpec &net = net_spec(id);
    RawParams raw;
    CHECK(read_raw_params(net, root + (net.is_cnv ? "/cifar10/" : "/mnist/") + net.name, raw).empty());
    std::vector<uint8_t> clean;
    pack_blob(net, raw, clean);
    for (int scheme = 0; scheme <= 3; scheme++) {
      MemOrg org;
      if (!hardening_layout(net, scheme, 0, org).empty()) {
        CHECK(hardened_mem_noise_mask(net, scheme, 1, 5, 0, 0, 0, 1u << 28, 0, nullptr, 0) == -1);
        continue;
      }
      PhysParams phys;
      phys_load(net, scheme, raw, 0, net.nlayers, phys);
      RawParams logical = raw;
      phys_logical(net, scheme, phys, logical);
      std::vector<uint8_t> blob;
      pack_blob(net, logical, blob);
      CHECK(blob == clean);
      long applied = 0;
      for (int burst : {3, 4, 16})
        for (int l = 0; l < net.nlayers; l++) {
          CHECK(hardening_layout(net, scheme, l, org).empty());
          for (int target = 0; target < 2; target++)
            for (int m = 0; m < (target ? org.t_modules : org.w_modules); m++) {
              const long k = hardened_mem_noise_mask(net, scheme, burst, 77, l, target, m, 1u << 25, 0, nullptr, 0);
              CHECK(k >= 0);
              std::vector<PhysFault> ev((size_t)k);
              CHECK(hardened_mem_noise_mask(net, scheme, burst, 77, l, target, m, 1u << 25, 0, ev.data(), k) == k);
              for (const PhysFault &pf : ev) CHECK(phys_apply(net, scheme, phys, pf) >= 0);
              applied += k;
              CHECK(hardened_mem_noise_mask(net, scheme, burst, 77, l, target, 3, 1u << 25, 0, nullptr, 0) == -1);
            }
        }
      CHECK(applied > 1000);
      phys_logical(net, scheme, phys, logical);
      pack_blob(net, logical, blob);
      CHECK(blob != clean);
      PhysFault out{Fault{0, 1, net.nlayers, 0, 0, 0, 0, 1}, 0};
      CHECK(phys_apply(net, scheme, phys, out) == -1);
    }
  }
  for (int il : {0, 2, 3})
    for (int T : {16, 24})
      for (int lines : {1, 2, 5})
        for (int ind = 0; ind < lines; ind++)
          for (int bit = 0; bit < T; bit++) {
            int a, b, c, d;
            interleave_site(il, T, lines, ind, bit, &a, &b);
            interleave_source(il, T, lines, a, b, &c, &d);
            CHECK(a >= 0 && a < lines && b >= 0 && b < T && c == ind && d == bit);
          }
  CHECK(hardening_scheme_of("cnvW1A1-TMR") == 1 && hardening_scheme_of("lfcW1A2-interleaved") == 2 &&
        hardening_scheme_of("cnvW2A2-resilient-interleaved") == 3 && hardening_scheme_of("cnvW1A1") == 0 && hardening_scheme_of(nullptr) == 0);
  std::printf("mem_org sanitize run ok\n");
  return 0;
}
