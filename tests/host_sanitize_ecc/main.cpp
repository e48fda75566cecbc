// Stand-alone driver for tests/test_host_sanitize_ecc.py: the coded threshold memories (csrc/ecc.h, csrc/mem_org.cpp) under
// AddressSanitizer + UBSan.  argv[1]: the params root.  The code over every data word (encode, the 22 single errors, a
// stride of the doubles); every supported (network, scheme, code): the loader's physical state gives back the files'
// blob; a run's events (bursts 1, 3, 4 and 16, every module, the check memories included) over two epochs applied, then
// de-interleaved and decoded; the check words' mapping over an odd line count; bad records and the refusals.
#include <cstdio>
#include <string>
#include <vector>

#include "mem_org.h"

using namespace bnn;

#define CHECK(x) do { if (!(x)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

int main(int argc, char **argv) {
  CHECK(argc == 2);
  const std::string root = argv[1];
  CHECK(ecc_encode(0x0001) == 0x23 && ecc_encode(0x8000) == 0x15 && ecc_encode(0xFFFF) == 0x1E && ecc_encode(0x1234) == 0x19);
  for (uint32_t d = 0; d < 65536; d++) {
    const uint32_t c = ecc_encode(d);
    uint32_t out = ~0u;
    CHECK(c < 64 && ecc_decode(d, c, &out) == 0 && out == d);
    for (int p = 0; p < 22; p++) {
      const uint32_t dm = p < 16 ? 1u << p : 0, cm = p < 16 ? 0 : 1u << (p - 16);
      CHECK(ecc_decode(d ^ dm, c ^ cm, &out) == 1 && out == d);
      const int q = (p + 1 + (int)(d % 21)) % 22;  // (one double per single: all 231 pairs come by over the words)
      const uint32_t dm2 = dm ^ (q < 16 ? 1u << q : 0), cm2 = cm ^ (q < 16 ? 0 : 1u << (q - 16));
      CHECK(ecc_decode(d ^ dm2, c ^ cm2, &out) == 2 && out == (d ^ dm2));
    }
  }
  for (uint32_t s = 0; s < 64 * 65536; s += 37) {  // any stored pair decodes to something, in range
    uint32_t out = ~0u;
    const int st = ecc_decode(s & 0xFFFF, s >> 16, &out);
    CHECK(st >= 0 && st <= 2 && out < 65536);
  }
  for (NetId id : {NET_CNVW1A1, NET_CNVW1A2, NET_CNVW2A2, NET_LFCW1A1, NET_LFCW1A2}) {
    const NetSpec &net = net_spec(id);
    RawParams raw;
    CHECK(read_raw_params(net, root + (net.is_cnv ? "/cifar10/" : "/mnist/") + net.name, raw).empty());
    std::vector<uint8_t> clean;
    pack_blob(net, raw, clean);
    for (int scheme = 0; scheme <= 3; scheme++)
      for (int code = 0; code <= 1; code++) {
        EccOrg eo;
        if (!ecc_layout(net, scheme, code, 0, eo).empty()) {
          CHECK(hardened_mem_noise_mask(net, scheme, 1, 5, 1, 1, 0, 1u << 28, 0, nullptr, 0, 0, code) == -1);
          CHECK(code == 1 ? (scheme == 1 || scheme == 3 || !hardening_layout(net, scheme, 0, eo.org).empty())
                          : !hardening_layout(net, scheme, 0, eo.org).empty());
          continue;
        }
        PhysParams phys;
        phys_load(net, scheme, raw, 0, net.nlayers, phys, code);
        RawParams logical = raw;
        long status[9][2];
        phys_logical(net, scheme, phys, logical, code, status);
        std::vector<uint8_t> blob;
        pack_blob(net, logical, blob);
        CHECK(blob == clean);
        for (int l = 0; l < net.nlayers; l++) CHECK(status[l][0] == 0 && status[l][1] == 0);
        long applied = 0, check_events = 0, coded = 0;
        for (int burst : {1, 3, 4, 16})
          for (int epoch : {0, 3})
            for (int l = 0; l < net.nlayers; l++) {
              CHECK(ecc_layout(net, scheme, code, l, eo).empty());
              CHECK(eo.check_bits == (code == 1 && net.L[l].nthr > 0 && !net.L[l].thr24 ? 6 : 0));
              coded += eo.check_bits != 0;
              for (int target = 0; target < 2; target++)
                for (int m = 0; m < (target ? eo.org.t_modules : eo.org.w_modules); m++) {
                  const long k = hardened_mem_noise_mask(net, scheme, burst, 77, l, target, m, 1u << 25, 0, nullptr, 0, epoch, code);
                  CHECK(k >= 0);
                  std::vector<PhysFault> ev((size_t)k);
                  CHECK(hardened_mem_noise_mask(net, scheme, burst, 77, l, target, m, 1u << 25, 0, ev.data(), k, epoch, code) == k);
                  for (const PhysFault &pf : ev) {
                    CHECK(phys_apply(net, scheme, phys, pf, code) >= 0);
                    if (target == 1 && m == 1 && eo.check_bits) CHECK(pf.f.bit < 6 && pf.f.bit % burst == 0 && pf.f.word_size == burst && pf.module == 1);
                  }
                  applied += k;
                  if (target == 1 && m == 1 && eo.check_bits) check_events += k;
                  CHECK(hardened_mem_noise_mask(net, scheme, burst, 77, l, target, 3, 1u << 25, 0, nullptr, 0, epoch, code) == -1);
                }
              if (eo.check_bits) {  // records outside the check memory
                for (const Fault &f : {Fault{0, 1, l, 0, 0, 0, 6, 1}, Fault{0, 1, l, net.L[l].fold.pe, 0, 0, 0, 1}, Fault{0, 1, l, 0, net.L[l].fold.tmem, 0, 0, 1},
                                       Fault{0, 1, l, 0, 0, net.L[l].nthr, 0, 1}, Fault{0, 1, l, 0, 0, 0, 0, 0}, Fault{0, 1, l, -1, 0, 0, 0, 1}})
                  CHECK(phys_apply(net, scheme, phys, PhysFault{f, 1}, code) == -1);
                CHECK(phys_apply(net, scheme, phys, PhysFault{Fault{0, 1, l, 0, 0, 0, 0, 1}, 2}, code) == -1);
              }
            }
        CHECK(applied > 1000 && (code == 0 ? check_events == 0 && coded == 0 : check_events > 100 && coded > 0));
        phys_logical(net, scheme, phys, logical, code, status);
        pack_blob(net, logical, blob);
        CHECK(blob != clean);
        long fixed = 0, seen = 0;
        for (int l = 0; l < net.nlayers; l++) {
          fixed += status[l][0];
          seen += status[l][1];
        }
        CHECK(code == 0 ? fixed == 0 && seen == 0 : fixed > 0 && seen > 0);
        PhysFault out{Fault{0, 1, net.nlayers, 0, 0, 0, 0, 1}, 0};
        CHECK(phys_apply(net, scheme, phys, out, code) == -1);
      }
  }
  for (int il : {0, 2})
    for (int lines : {1, 2, 5})
      for (int ind = 0; ind < lines; ind++)
        for (int bit = 0; bit < 6; bit++) {
          int a, b, c, d;
          interleave_site(il, 6, lines, ind, bit, &a, &b);
          interleave_source(il, 6, lines, a, b, &c, &d);
          CHECK(a >= 0 && a < lines && b >= 0 && b < 6 && c == ind && d == bit);
          if (il == 0 || (ind & ~1) + 1 >= lines) CHECK(a == ind && b == bit);
          else CHECK(a == ((ind & ~1) + (2 * bit + (ind & 1) >= 6 ? 0 : 1)) && b == (2 * bit + (ind & 1)) % 6);
        }
  CHECK(ecc_check_groups(1) == 6 && ecc_check_groups(2) == 3 && ecc_check_groups(4) == 2 && ecc_check_groups(16) == 1);
  std::printf("ecc sanitize run ok\n");
  return 0;
}
