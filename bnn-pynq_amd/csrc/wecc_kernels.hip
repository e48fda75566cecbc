// wecc_kernels.hip -- the upset and the repair kernel of the coded (SEC-DED (72,64)) weight memories in the exposure
// campaigns (bnn_mi355x_wecc_exposure_campaigns; the code: wecc.h, the storage and the draw: mem_org.h, "coded weight
// memories"; declared in kernels.h).
// A translation unit of its own for the reason ecc_kernels.hip and repair_kernels.hip are ones: built apart, kernels.o,
// ecc_kernels.o and repair_kernels.o stay what they were.
#include <hip/hip_runtime.h>
#include <stdint.h>

#define BNN_HD __host__ __device__  // (the shared headers' routines compile for the device here, as in kernels.hip)
#include "act_faults.h"
#include "kernels.h"
#include "mem_org.h"
#include "packed_params.h"

namespace bnn {
namespace {

constexpr int kBlock = 256;  // (kernels.hip's block)

// bits 0, 2, 4, ... 62 of x, packed into 32 bits
__device__ inline uint64_t even_bits(uint64_t x) {
  x &= 0x5555555555555555ull;
  x = (x | x >> 1) & 0x3333333333333333ull;
  x = (x | x >> 2) & 0x0F0F0F0F0F0F0F0Full;
  x = (x | x >> 4) & 0x00FF00FF00FF00FFull;
  x = (x | x >> 8) & 0x0000FFFF0000FFFFull;
  return (x | x >> 16) & 0xFFFFFFFFull;
}

// k_wmem_noise_w: the weights of a CODED layer, in k_xmem_noise_w's (kernels.hip) place and geometry: a lane per
// 64-column word k of one (run, row n), no LDS.  The lane owns sites site0 ... site0 + kSites - 1 of the weight memory,
// site0 a multiple of 64: exactly code word site0 / 64 (1-bit weights) or code words site0 / 64 and site0 / 64 + 1
// (2-bit weights: 32 columns each).  Per code word the lane's state is a pair of longs: the accumulated hit mask of the
// 64 data sites (bit j: site 64 q + j) and of the 8 check bits -- so no lane depends on another's state.  The lane draws
// its data sites exactly as k_xmem_noise_w does (module 0), then the 8 check bits of each code word (module 1, element
// q of the check memory, per_c = ceil(8 / burst) groups), XORs both into the state (stored only when something was
// hit) and decodes the PATTERN (the code is linear: wecc.h): what wecc_decode leaves of (data mask, check mask) is the
// error in the delivered word.  delivered = loaded ^ that error; the row word(s) are stored only where they differ from
// what the run's copy holds.  2-bit weights: site 2j is the low and 2j + 1 the high bit of column j's field; the planes
// (neg, nz, two) are rebuilt from the delivered (high, low) the way fill_row derives them, and a word that holds a -2
// sets the row's flag dword (k_mem_noise_flags, launched behind, clears it where a correction or a flip removed the
// last one).  counts as for k_xmem_noise_w: [0] += the data and check bits flipped, [1] += the delivered data bits that
// differ from the loaded ones.  wst: this epoch's [layer][4] of run 0, run q's wst_stride longs behind: [0] / [1] += the
// code words at decode status 1 / 2, over ALL lanes.
template <bool TWO_BIT>
__global__ __launch_bounds__(kBlock) void k_wmem_noise_w(uint8_t *__restrict__ copies, unsigned long long stride, MemNoiseLayer L, unsigned ebits,
                                                         unsigned burst, const unsigned long long *__restrict__ seeds, unsigned rate,
                                                         unsigned epoch, const uint8_t *__restrict__ loaded, ulonglong2 *__restrict__ state,
                                                         unsigned long long *__restrict__ counts, unsigned long long run_stride,
                                                         unsigned long long *__restrict__ wst, unsigned long long wst_stride) {
  constexpr unsigned CW = TWO_BIT ? 2 : 1;
  const unsigned run = blockIdx.y, t = blockIdx.x * kBlock + threadIdx.x;
  unsigned c = 0, d = 0, fixed = 0, seen = 0;
  if (t < L.rows * L.kw) {
    const unsigned n = t / L.kw, k = t - n * L.kw;
    const unsigned long long seed = seeds[run];
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32), tag = exposure_tag(epoch);
    const unsigned per = (ebits + burst - 1) / burst, per_c = wecc_check_groups((int)burst);
    const unsigned site0 = (((n % L.pe) * L.tmem + n / L.pe) * L.kw + k) * (64 * CW);
    unsigned element = site0 / ebits, bit = site0 - element * ebits, e = element * per + bit / burst, in_group = bit % burst;
    uint32_t u[4], have = ~0u;
    uint64_t dm[CW], rem[CW];
    uint32_t cm[CW];
    {
      const uint32_t word = hardened_draw_word(0, 0, (int)burst);
#pragma unroll
      for (unsigned w = 0; w < CW; w++) {
        uint64_t m = 0;
        for (unsigned j = 0; j < 64; j++) {
          if ((e >> 2) != have) {
            have = e >> 2;
            act_noise_block(k0, k1, L.layer, word, have, u, tag);
          }
          const uint32_t ue = (e & 2) ? ((e & 1) ? u[3] : u[2]) : ((e & 1) ? u[1] : u[0]);
          m |= (ue < rate ? 1ull : 0ull) << j;
          if (++bit == ebits) {
            bit = 0; in_group = 0;
            e = ++element * per;
          } else if (++in_group == burst) {
            in_group = 0;
            e++;
          }
        }
        dm[w] = m;
      }
    }
    {
      const uint32_t word = hardened_draw_word(0, 1, (int)burst);
      have = ~0u;
#pragma unroll
      for (unsigned w = 0; w < CW; w++) {
        const unsigned q = site0 / 64 + w;
        uint32_t m = 0;
#pragma unroll
        for (unsigned b = 0; b < (unsigned)kWeccCheckBits; b++) {
          const uint32_t ec = q * per_c + b / burst;
          if ((ec >> 2) != have) {
            have = ec >> 2;
            act_noise_block(k0, k1, L.layer, word, have, u, tag);
          }
          const uint32_t ue = (ec & 2) ? ((ec & 1) ? u[3] : u[2]) : ((ec & 1) ? u[1] : u[0]);
          m |= (ue < rate ? 1u : 0u) << b;
        }
        cm[w] = m;
      }
    }
    ulonglong2 *const st = state + ((size_t)run * L.rows * L.kw + t) * CW;
#pragma unroll
    for (unsigned w = 0; w < CW; w++) {
      ulonglong2 s = st[w];
      if (dm[w] | cm[w]) {
        s.x ^= dm[w];
        s.y ^= cm[w];
        st[w] = s;
      }
      const int status = wecc_decode(s.x, (uint32_t)s.y, &rem[w]);
      fixed += status == 1;
      seen += status == 2;
      c += __popcll(dm[w]) + __popc(cm[w]);
      d += __popcll(rem[w]);
    }
    const size_t at = (size_t)L.offset + (size_t)n * L.row_dwords * 4 + 8;  // (the row's planes, behind its two threshold dwords)
    uint32_t *const row = reinterpret_cast<uint32_t *>(copies + (size_t)run * stride + L.offset) + (size_t)n * L.row_dwords;
    const uint64_t *const was = reinterpret_cast<const uint64_t *>(loaded + at);
    if constexpr (!TWO_BIT) {
      uint64_t *const w = reinterpret_cast<uint64_t *>(row + 2) + k;
      const uint64_t now = was[k] ^ rem[0];
      if (*w != now) *w = now;
    } else {
      uint64_t *const wq = reinterpret_cast<uint64_t *>(row + 2);
      const uint64_t elo = even_bits(rem[0]) | even_bits(rem[1]) << 32, ehi = even_bits(rem[0] >> 1) | even_bits(rem[1] >> 1) << 32;
      const uint64_t hi = was[2 * k] ^ ehi, lo = (was[2 * k + 1] & ~was[2 * L.kw + k]) ^ elo, two2 = hi & ~lo;
      bool changed = false;
      if (wq[2 * k] != hi) { wq[2 * k] = hi; changed = true; }
      if (wq[2 * k + 1] != (hi | lo)) { wq[2 * k + 1] = hi | lo; changed = true; }
      if (wq[2 * L.kw + k] != two2) { wq[2 * L.kw + k] = two2; changed = true; }
      if (changed && two2) atomicOr(row + 2 + 6 * L.kw, 1u);
    }
  }
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) {
    c += __shfl_xor(c, s, 64);
    d += __shfl_xor(d, s, 64);
    fixed += __shfl_xor(fixed, s, 64);
    seen += __shfl_xor(seen, s, 64);
  }
  if ((threadIdx.x & 63) == 0 && (c | d | fixed | seen)) {
    unsigned long long *const at = counts + (size_t)run * run_stride + (size_t)L.layer * 4;
    unsigned long long *const ws = wst + (size_t)run * wst_stride + (size_t)L.layer * 4;
    if (c) atomicAdd(at, (unsigned long long)c);
    if (d) atomicAdd(at + 1, (unsigned long long)d);
    if (fixed) atomicAdd(ws, (unsigned long long)fixed);
    if (seen) atomicAdd(ws + 1, (unsigned long long)seen);
  }
}

// k_wrepair_state: a lane per (coded layer blockIdx.z, run blockIdx.y, code word).  The state pairs of k_wmem_noise_w
// are per code word, so the repair is lane-local: the pair becomes wecc_repair's (status 1: the remaining error and its
// check bits; else as it was), stored only where it changed.  The blocks past a layer's code words exit as a whole.  No
// LDS, no row rebuild: the delivered weights are the same before and after.  wst[2] += the code words rewritten, [3] +=
// those whose state still differs from the loaded one.
__global__ __launch_bounds__(kBlock) void k_wrepair_state(uint8_t *__restrict__ camp, RepairTable tab, unsigned long long *__restrict__ wst,
                                                          unsigned long long wst_stride) {
  const RepairEntry E = tab.e[blockIdx.z];
  if (E.kind != RK_CODED || blockIdx.x * kBlock >= E.lanes) return;
  const unsigned run = blockIdx.y, t = blockIdx.x * kBlock + threadIdx.x;
  unsigned wrote = 0, left = 0;
  if (t < E.lanes) {
    ulonglong2 *const st = reinterpret_cast<ulonglong2 *>(camp + E.state_off) + (size_t)run * E.lanes + t;
    const ulonglong2 before = *st;
    uint64_t dd;
    uint32_t cc;
    wrote = wecc_repair(before.x, (uint32_t)before.y, &dd, &cc) == 1;
    left = (dd | cc) != 0;
    if (dd != before.x || cc != before.y) *st = make_ulonglong2(dd, cc);
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    wrote += __shfl_xor(wrote, d, 64);
    left += __shfl_xor(left, d, 64);
  }
  if ((threadIdx.x & 63) == 0 && (wrote | left)) {
    unsigned long long *const at = wst + (size_t)run * wst_stride + (size_t)E.layer * 4 + 2;
    if (wrote) atomicAdd(at, (unsigned long long)wrote);
    if (left) atomicAdd(at + 1, (unsigned long long)left);
  }
}

}  // namespace

hipError_t wmem_noise_w(uint8_t *copies, size_t stride, int runs, const unsigned long long *seeds, const MemNoiseLayer &L, bool two_bit,
                        int ebits, int burst, uint32_t rate_q32, int epoch, const uint8_t *loaded, unsigned long long *state,
                        unsigned long long *counts, size_t run_stride, unsigned long long *wst, size_t wst_stride, hipStream_t s) {
  if (runs <= 0 || rate_q32 == 0) return hipSuccess;
  if (runs > 65535 || L.kw == 0 || L.rows == 0 || stride % 256 || L.offset % 8 || L.row_dwords % 2 ||
      L.row_dwords < (two_bit ? 4 + 6 * L.kw : 2 + 2 * L.kw) || ebits < 1 || ebits > 64 || 64 % ebits || burst < 1 || burst > kMaxBurst ||
      epoch < 0 || epoch >= kMaxEpochs || !loaded || (uintptr_t)loaded % 8 || !counts || !state || (uintptr_t)state % 16 || !wst || L.pe == 0 ||
      L.rows != L.pe * L.tmem)
    return hipErrorInvalidValue;
  const dim3 g((L.rows * L.kw + kBlock - 1) / kBlock, (unsigned)runs);
  ulonglong2 *const st = reinterpret_cast<ulonglong2 *>(state);
  if (two_bit)
    hipLaunchKernelGGL(k_wmem_noise_w<true>, g, dim3(kBlock), 0, s, copies, (unsigned long long)stride, L, (unsigned)ebits, (unsigned)burst, seeds,
                       rate_q32, (unsigned)epoch, loaded, st, counts, (unsigned long long)run_stride, wst, (unsigned long long)wst_stride);
  else
    hipLaunchKernelGGL(k_wmem_noise_w<false>, g, dim3(kBlock), 0, s, copies, (unsigned long long)stride, L, (unsigned)ebits, (unsigned)burst, seeds,
                       rate_q32, (unsigned)epoch, loaded, st, counts, (unsigned long long)run_stride, wst, (unsigned long long)wst_stride);
  return hipGetLastError();
}

hipError_t wrepair_state(uint8_t *camp, const RepairTable &tab, int entries, int runs, unsigned long long *wst, size_t wst_stride, hipStream_t s) {
  if (runs <= 0 || entries <= 0) return hipSuccess;
  if (runs > 65535 || entries > kRepairEntries || !camp || !wst) return hipErrorInvalidValue;
  uint32_t most = 0;
  for (int k = 0; k < entries; k++) {
    const RepairEntry &e = tab.e[k];
    if (e.kind != RK_CODED || e.state_off % 16 || e.lanes == 0) return hipErrorInvalidValue;
    if (e.lanes > most) most = e.lanes;
  }
  const dim3 g((most + kBlock - 1) / kBlock, (unsigned)runs, (unsigned)entries);
  hipLaunchKernelGGL(k_wrepair_state, g, dim3(kBlock), 0, s, camp, tab, wst, (unsigned long long)wst_stride);
  return hipGetLastError();
}

}  // namespace bnn
