// iwecc_kernels.hip -- the upset and the repair kernel of the COLUMN-INTERLEAVED coded weight memories in the exposure
// campaigns (bnn_mi355x_iwecc_exposure_campaigns; the model: mem_org.h, "column-interleaved code words"; the exchange:
// iwecc.h; the code: wecc.h; declared in kernels.h).
// A translation unit of its own for the reason wecc_kernels.hip is one: built apart, kernels.o, ecc_kernels.o,
// repair_kernels.o and wecc_kernels.o stay what they were.
#include <hip/hip_runtime.h>
#include <stdint.h>

#define BNN_HD __host__ __device__  // (the shared headers' routines compile for the device here, as in kernels.hip)
#include "act_faults.h"
#include "iwecc.h"
#include "kernels.h"
#include "mem_org.h"
#include "packed_params.h"

namespace bnn {
namespace {

constexpr int kBlock = 256;  // (kernels.hip's block; a multiple of every depth, so a group never straddles blocks)

// bits 0, 2, 4, ... 62 of x, packed into 32 bits
__device__ inline uint32_t even_bits(uint64_t x) {
  x &= 0x5555555555555555ull;
  x = (x | x >> 1) & 0x3333333333333333ull;
  x = (x | x >> 2) & 0x0F0F0F0F0F0F0F0Full;
  x = (x | x >> 4) & 0x00FF00FF00FF00FFull;
  x = (x | x >> 8) & 0x0000FFFF0000FFFFull;
  return (uint32_t)(x | x >> 16);
}

// The D x D transpose of sub-words across the D = 2^LOGD adjacent lanes of a group: a butterfly of LOGD __shfl_xor stages
// (distances 1, 2, 4, 8: inside a 16-lane row) with a masked half-swap each (iwecc.h).  EVERY lane of the wave must call.
template <int LOGD>
__device__ inline uint64_t transpose(uint64_t x, unsigned lane) {
  if constexpr (LOGD > 0) x = iwecc_stage<LOGD, 0>(x, __shfl_xor((unsigned long long)x, 1, 64), lane & 1u);
  if constexpr (LOGD > 1) x = iwecc_stage<LOGD, 1>(x, __shfl_xor((unsigned long long)x, 2, 64), (lane >> 1) & 1u);
  if constexpr (LOGD > 2) x = iwecc_stage<LOGD, 2>(x, __shfl_xor((unsigned long long)x, 4, 64), (lane >> 2) & 1u);
  if constexpr (LOGD > 3) x = iwecc_stage<LOGD, 3>(x, __shfl_xor((unsigned long long)x, 8, 64), (lane >> 3) & 1u);
  return x;
}

// physical hit masks (a lane: its 64 sites) -> code word patterns (a lane: one code word of its group), and back.  logd is
// the layer's, the same for the whole grid, so the switch is a scalar branch and all lanes of a wave take one case.
__device__ inline uint64_t to_words(unsigned logd, uint64_t x, unsigned lane) {
  switch (logd) {
    case 1: return transpose<1>(iwecc_unzip<1>(x), lane);
    case 2: return transpose<2>(iwecc_unzip<2>(x), lane);
    case 3: return transpose<3>(iwecc_unzip<3>(x), lane);
    case 4: return transpose<4>(iwecc_unzip<4>(x), lane);
    default: return x;
  }
}
__device__ inline uint64_t from_words(unsigned logd, uint64_t x, unsigned lane) {
  switch (logd) {
    case 1: return iwecc_zip<1>(transpose<1>(x, lane));
    case 2: return iwecc_zip<2>(transpose<2>(x, lane));
    case 3: return iwecc_zip<3>(transpose<3>(x, lane));
    case 4: return iwecc_zip<4>(transpose<4>(x, lane));
    default: return x;
  }
}

// The check masks, by offsets (depth 16 gives a code word half a bit of every element: iwecc.h): a lane reads check bit k
// of its code word from the element that holds it -- 8 reads of another lane's dword -- and, on the way back, every bit of
// its element from the code word that owns it.  EVERY lane of the wave must call.
__device__ inline uint32_t check_to_words(unsigned logd, uint32_t cm, unsigned lane) {
  const unsigned D = 1u << logd, base = lane & ~(D - 1), c = lane & (D - 1);
  uint32_t out = 0;
#pragma unroll
  for (unsigned k = 0; k < (unsigned)kWeccCheckBits; k++) {
    unsigned el, b;
    iwecc_check_source(D, c, k, &el, &b);
    out |= ((__shfl(cm, (int)(base + el), 64) >> b) & 1u) << k;
  }
  return out;
}
__device__ inline uint32_t check_from_words(unsigned logd, uint32_t cw, unsigned lane) {
  const unsigned D = 1u << logd, base = lane & ~(D - 1), i = lane & (D - 1);
  uint32_t out = 0;
#pragma unroll
  for (unsigned b = 0; b < (unsigned)kWeccCheckBits; b++) {
    unsigned c, k;
    iwecc_check_target(D, i, b, &c, &k);
    out |= ((__shfl(cw, (int)(base + c), 64) >> k) & 1u) << b;
  }
  return out;
}

// k_iwmem_noise_w: the weights of a coded layer of interleave depth 2^logd, in k_wmem_noise_w's (wecc_kernels.hip) place.
// A lane per code word's worth of storage, numbered in SITE order: lane q owns sites [64 q, 64 q + 64) of the weight memory
// and element q of the check memory, so that the D words of a group sit on D adjacent lanes of one wave (k_wmem_noise_w
// numbers its lanes in row order, where a PE's consecutive words are pe * kw lanes apart).  q -> PE q / (tmem kw CW), line
// (q / (kw CW)) % tmem, 64-column word k = (q / CW) % kw of row n = line * pe + PE; 2-bit weights (CW = 2): half h = q % CW
// of that word, columns 32 h ... 32 h + 31, stored as 32-bit halves of the 64-bit plane words.
// The lane draws its sites and its check element with k_wmem_noise_w's loops (the same Philox blocks) and XORs them into
// its state pair -- the accumulated PHYSICAL hit masks of its 64 sites and its check element.  Then the group turns its D
// physical masks into the D code word patterns (to_words, check_to_words), every lane decodes its pattern (the code is
// linear: wecc.h) and the remaining-error words go back (from_words): delivered = loaded ^ remaining for the lane's own 64
// sites, stored only where that differs from the copy's.  The exchanges stand OUTSIDE the `mine` guard: every lane of a
// wave executes them (the launcher refuses a layer whose code words per run are no multiple of 64, so a wave is whole or
// absent, and an absent one contributes zeros).  A wave whose state is all zero after the XOR has nothing to decode and
// skips them as a whole (the ballot is wave-uniform).  The 2-bit plane rebuild, the -2 row flag and k_mem_noise_flags
// behind it are k_wmem_noise_w's.  counts and wst as there; [0] / [1] of wst count code words after gathering.
template <bool TWO_BIT>
__global__ __launch_bounds__(kBlock) void k_iwmem_noise_w(uint8_t *__restrict__ copies, unsigned long long stride, MemNoiseLayer L, unsigned ebits,
                                                          unsigned burst, unsigned logd, const unsigned long long *__restrict__ seeds,
                                                          unsigned rate, unsigned epoch, const uint8_t *__restrict__ loaded,
                                                          ulonglong2 *__restrict__ state, unsigned long long *__restrict__ counts,
                                                          unsigned long long run_stride, unsigned long long *__restrict__ wst,
                                                          unsigned long long wst_stride) {
  constexpr unsigned CW = TWO_BIT ? 2 : 1;
  const unsigned run = blockIdx.y, q = blockIdx.x * kBlock + threadIdx.x, lane = threadIdx.x & 63u;
  const unsigned words = L.rows * L.kw * CW;
  const bool mine = q < words;
  unsigned c = 0, d = 0, fixed = 0, seen = 0;
  uint64_t px = 0, rem = 0;
  uint32_t py = 0;
  if (mine) {
    const unsigned long long seed = seeds[run];
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32), tag = exposure_tag(epoch);
    const unsigned per = (ebits + burst - 1) / burst, per_c = wecc_check_groups((int)burst);
    const unsigned site0 = q * 64;
    unsigned element = site0 / ebits, bit = site0 - element * ebits, e = element * per + bit / burst, in_group = bit % burst;
    uint32_t u[4], have = ~0u;
    uint64_t dm = 0;
    uint32_t cm = 0;
    {
      const uint32_t word = hardened_draw_word(0, 0, (int)burst);
      for (unsigned j = 0; j < 64; j++) {
        if ((e >> 2) != have) {
          have = e >> 2;
          act_noise_block(k0, k1, L.layer, word, have, u, tag);
        }
        const uint32_t ue = (e & 2) ? ((e & 1) ? u[3] : u[2]) : ((e & 1) ? u[1] : u[0]);
        dm |= (ue < rate ? 1ull : 0ull) << j;
        if (++bit == ebits) {
          bit = 0; in_group = 0;
          e = ++element * per;
        } else if (++in_group == burst) {
          in_group = 0;
          e++;
        }
      }
    }
    {
      const uint32_t word = hardened_draw_word(0, 1, (int)burst);
      have = ~0u;
#pragma unroll
      for (unsigned b = 0; b < (unsigned)kWeccCheckBits; b++) {
        const uint32_t ec = q * per_c + b / burst;
        if ((ec >> 2) != have) {
          have = ec >> 2;
          act_noise_block(k0, k1, L.layer, word, have, u, tag);
        }
        const uint32_t ue = (ec & 2) ? ((ec & 1) ? u[3] : u[2]) : ((ec & 1) ? u[1] : u[0]);
        cm |= (ue < rate ? 1u : 0u) << b;
      }
    }
    ulonglong2 *const st = state + (size_t)run * words + q;
    ulonglong2 s = *st;
    if (dm | cm) {
      s.x ^= dm;
      s.y ^= cm;
      *st = s;
    }
    px = s.x;
    py = (uint32_t)s.y;
    c = __popcll(dm) + __popc(cm);
  }
  if (__any((px | py) != 0)) {  // (wave-uniform: all lanes exchange, or none)
    uint64_t left;
    const int status = wecc_decode(to_words(logd, px, lane), check_to_words(logd, py, lane), &left);
    fixed = status == 1;
    seen = status == 2;
    rem = from_words(logd, left, lane);
    d = __popcll(rem);
  }
  if (mine) {
    const unsigned w = q / CW, k = w % L.kw, line = (w / L.kw) % L.tmem, n = line * L.pe + w / (L.kw * L.tmem);
    const size_t at = (size_t)L.offset + (size_t)n * L.row_dwords * 4 + 8;  // (the row's planes, behind its two threshold dwords)
    uint32_t *const row = reinterpret_cast<uint32_t *>(copies + (size_t)run * stride + L.offset) + (size_t)n * L.row_dwords;
    if constexpr (!TWO_BIT) {
      uint64_t *const wd = reinterpret_cast<uint64_t *>(row + 2) + k;
      const uint64_t now = reinterpret_cast<const uint64_t *>(loaded + at)[k] ^ rem;
      if (*wd != now) *wd = now;
    } else {
      // dword 2 i + h of the planes is half h of plane word i: words 2 k (neg), 2 k + 1 (nz), 2 kw + k (two)
      const unsigned h = q & 1u, ineg = 2 * (2 * k) + h, inz = 2 * (2 * k + 1) + h, itwo = 2 * (2 * L.kw + k) + h;
      uint32_t *const wq = row + 2;
      const uint32_t *const was = reinterpret_cast<const uint32_t *>(loaded + at);
      const uint32_t hi = was[ineg] ^ even_bits(rem >> 1), lo = (was[inz] & ~was[itwo]) ^ even_bits(rem), two2 = hi & ~lo;
      bool changed = false;
      if (wq[ineg] != hi) { wq[ineg] = hi; changed = true; }
      if (wq[inz] != (hi | lo)) { wq[inz] = hi | lo; changed = true; }
      if (wq[itwo] != two2) { wq[itwo] = two2; changed = true; }
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
  if (lane == 0 && (c | d | fixed | seen)) {
    unsigned long long *const at = counts + (size_t)run * run_stride + (size_t)L.layer * 4;
    unsigned long long *const ws = wst + (size_t)run * wst_stride + (size_t)L.layer * 4;
    if (c) atomicAdd(at, (unsigned long long)c);
    if (d) atomicAdd(at + 1, (unsigned long long)d);
    if (fixed) atomicAdd(ws, (unsigned long long)fixed);
    if (seen) atomicAdd(ws + 1, (unsigned long long)seen);
  }
}

// k_iwrepair_state: a lane per (coded layer blockIdx.z, run blockIdx.y, state pair) in k_wrepair_state's place.  The pairs
// are physical, so the group exchanges them into code word patterns, every lane applies wecc_repair to its code word, and
// the new patterns go back; a pair is stored only where it changed.  The blocks past a layer's pairs exit as a whole, and
// inside a block a wave is whole or absent (the launcher checks lanes % 64), so every lane of a wave that exchanges is
// there.  wst[2] += the code words rewritten, [3] += those whose state still differs from the loaded one: per code word.
__global__ __launch_bounds__(kBlock) void k_iwrepair_state(uint8_t *__restrict__ camp, RepairTable tab, unsigned long long *__restrict__ wst,
                                                           unsigned long long wst_stride) {
  const RepairEntry E = tab.e[blockIdx.z];
  if (E.kind != RK_CODED || blockIdx.x * kBlock >= E.lanes) return;
  const unsigned run = blockIdx.y, t = blockIdx.x * kBlock + threadIdx.x, lane = threadIdx.x & 63u;
  const unsigned logd = 31u - (unsigned)__clz((int)E.depth);
  const bool mine = t < E.lanes;
  ulonglong2 *const st = reinterpret_cast<ulonglong2 *>(camp + E.state_off) + (size_t)run * E.lanes + t;
  ulonglong2 before = make_ulonglong2(0, 0);
  if (mine) before = *st;
  unsigned wrote = 0, left = 0;
  if (__any((before.x | before.y) != 0)) {
    uint64_t dd;
    uint32_t cc;
    wrote = wecc_repair(to_words(logd, before.x, lane), check_to_words(logd, (uint32_t)before.y, lane), &dd, &cc) == 1;
    left = (dd | cc) != 0;
    const uint64_t nx = from_words(logd, dd, lane);
    const uint32_t ny = check_from_words(logd, cc, lane);
    if (mine && (nx != before.x || ny != before.y)) *st = make_ulonglong2(nx, ny);
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    wrote += __shfl_xor(wrote, d, 64);
    left += __shfl_xor(left, d, 64);
  }
  if (lane == 0 && (wrote | left)) {
    unsigned long long *const at = wst + (size_t)run * wst_stride + (size_t)E.layer * 4 + 2;
    if (wrote) atomicAdd(at, (unsigned long long)wrote);
    if (left) atomicAdd(at + 1, (unsigned long long)left);
  }
}

bool depth_ok(int depth) { return depth >= 1 && depth <= kMaxBurst && (depth & (depth - 1)) == 0; }

}  // namespace

hipError_t iwmem_noise_w(uint8_t *copies, size_t stride, int runs, const unsigned long long *seeds, const MemNoiseLayer &L, bool two_bit,
                         int ebits, int burst, int depth, uint32_t rate_q32, int epoch, const uint8_t *loaded, unsigned long long *state,
                         unsigned long long *counts, size_t run_stride, unsigned long long *wst, size_t wst_stride, hipStream_t s) {
  if (runs <= 0 || rate_q32 == 0) return hipSuccess;
  if (runs > 65535 || L.kw == 0 || L.rows == 0 || stride % 256 || L.offset % 8 || L.row_dwords % 2 ||
      L.row_dwords < (two_bit ? 4 + 6 * L.kw : 2 + 2 * L.kw) || ebits < 1 || ebits > 64 || 64 % ebits || burst < 1 || burst > kMaxBurst ||
      epoch < 0 || epoch >= kMaxEpochs || !loaded || (uintptr_t)loaded % 8 || !counts || !state || (uintptr_t)state % 16 || !wst || L.pe == 0 ||
      L.rows != L.pe * L.tmem || !depth_ok(depth))
    return hipErrorInvalidValue;
  const unsigned words = L.rows * L.kw * (two_bit ? 2u : 1u);
  // a wave is whole or absent (the exchanges need every lane), a group lies inside one PE's words, and 64 q fits a dword
  if (words % 64 || (L.tmem * L.kw * (two_bit ? 2u : 1u)) % (unsigned)depth || words > (1u << 26)) return hipErrorInvalidValue;
  unsigned logd = 0;
  while ((1 << logd) < depth) logd++;
  const dim3 g((words + kBlock - 1) / kBlock, (unsigned)runs);
  ulonglong2 *const st = reinterpret_cast<ulonglong2 *>(state);
  if (two_bit)
    hipLaunchKernelGGL(k_iwmem_noise_w<true>, g, dim3(kBlock), 0, s, copies, (unsigned long long)stride, L, (unsigned)ebits, (unsigned)burst, logd,
                       seeds, rate_q32, (unsigned)epoch, loaded, st, counts, (unsigned long long)run_stride, wst, (unsigned long long)wst_stride);
  else
    hipLaunchKernelGGL(k_iwmem_noise_w<false>, g, dim3(kBlock), 0, s, copies, (unsigned long long)stride, L, (unsigned)ebits, (unsigned)burst, logd,
                       seeds, rate_q32, (unsigned)epoch, loaded, st, counts, (unsigned long long)run_stride, wst, (unsigned long long)wst_stride);
  return hipGetLastError();
}

hipError_t iwrepair_state(uint8_t *camp, const RepairTable &tab, int entries, int runs, unsigned long long *wst, size_t wst_stride, hipStream_t s) {
  if (runs <= 0 || entries <= 0) return hipSuccess;
  if (runs > 65535 || entries > kRepairEntries || !camp || !wst) return hipErrorInvalidValue;
  uint32_t most = 0;
  for (int k = 0; k < entries; k++) {
    const RepairEntry &e = tab.e[k];
    if (e.kind != RK_CODED || e.state_off % 16 || e.lanes == 0 || e.lanes % 64 || !depth_ok((int)e.depth) || e.lanes % e.depth) return hipErrorInvalidValue;
    if (e.lanes > most) most = e.lanes;
  }
  const dim3 g((most + kBlock - 1) / kBlock, (unsigned)runs, (unsigned)entries);
  hipLaunchKernelGGL(k_iwrepair_state, g, dim3(kBlock), 0, s, camp, tab, wst, (unsigned long long)wst_stride);
  return hipGetLastError();
}

}  // namespace bnn
