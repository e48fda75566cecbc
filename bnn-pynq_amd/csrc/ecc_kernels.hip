// ecc_kernels.hip -- the upset kernel of the coded (SEC-DED) threshold memories in the exposure campaigns
// (bnn_mi355x_ecc_exposure_campaigns; the code: ecc.h, the storage and the draw: mem_org.h; declared in kernels.h).
// A translation unit of its own, for one reason: interleave_site is called here at widths 16 AND 6, and in kernels.hip
// -- where every caller passes 16 -- that would change what the compiler makes of k_xmem_noise_t (measured: DESIGN.md
// 9).  Kept apart, every kernel body of kernels.hip is what it was.
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

// k_emem_noise_t: the thresholds of a CODED layer (SEC-DED, ecc.h; the storage and the draw: mem_org.h, "coded threshold
// memories"), in k_xmem_noise_t's (kernels.hip) place and geometry: a lane per (run, neuron n, threshold i), no LDS.  The lane's state
// word holds, in logical-image order, the accumulated hit mask of its 16 data bits (bits 0 ... 15; module 0) and of its
// 6 check bits (bits 16 ... 21; the check memory, module 1): bit k is the physical bit interleave_site gives for logical
// bit k at width 16 or 6 -- so no lane depends on another's state.  The code is linear, so the lane decodes the error
// pattern itself: what ecc_decode leaves of (data mask, check mask) is the error in the delivered word.  Where that
// differs from the one before the epoch the row dword(s) are rebuilt from the pristine raw table.  ecc: this epoch's
// [layer][2: words decoded with status 1, with status 2] of run 0, run q's ecc_stride longs behind, over ALL lanes.
__global__ __launch_bounds__(kBlock) void k_emem_noise_t(uint8_t *__restrict__ copies, unsigned long long stride, MemNoiseLayer L, unsigned nthr,
                                                         Arith arith, bool signed_bb, const uint16_t *__restrict__ raw, unsigned interleave,
                                                         unsigned burst, const unsigned long long *__restrict__ seeds, unsigned rate,
                                                         unsigned epoch, unsigned long long *__restrict__ state,
                                                         unsigned long long *__restrict__ counts, unsigned long long run_stride,
                                                         unsigned long long *__restrict__ ecc, unsigned long long ecc_stride) {
  const unsigned run = blockIdx.y, t = blockIdx.x * kBlock + threadIdx.x;
  uint32_t m = 0;
  unsigned phys = 0, fixed = 0, seen = 0;
  if (t < L.rows * nthr) {
    const unsigned n = t / nthr, i = t - n * nthr, mem = n % L.pe, ind = n / L.pe;
    const unsigned long long seed = seeds[run];
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32), tag = exposure_tag(epoch);
    uint32_t hits = 0, u[4];
#pragma unroll
    for (int md = 0; md < 2; md++) {  // the data memory, then the check memory: the same construction at width 16 and 6
      const int width = md ? kEccCheckBits : kEccDataBits;
      const unsigned per = ((unsigned)width + burst - 1) / burst;
      const uint32_t word = hardened_draw_word(1, md, (int)burst);
      uint32_t have = ~0u;  // (the last Philox block: bits of one line share it)
      for (int k = 0; k < width; k++) {
        int p_ind, p_bit;
        interleave_site((int)interleave, width, (int)L.tmem, (int)ind, k, &p_ind, &p_bit);
        const uint32_t e = ((mem * L.tmem + (unsigned)p_ind) * nthr + i) * per + (unsigned)p_bit / burst;
        if ((e >> 2) != have) {
          have = e >> 2;
          act_noise_block(k0, k1, L.layer, word, have, u, tag);
        }
        const uint32_t ue = (e & 2) ? ((e & 1) ? u[3] : u[2]) : ((e & 1) ? u[1] : u[0]);
        hits |= (ue < rate ? 1u : 0u) << (md ? kEccDataBits + k : k);
      }
    }
    phys = __popc(hits);
    unsigned long long *const st = state + (size_t)run * L.rows * nthr + t;
    const uint32_t before = (uint32_t)*st, after = before ^ hits;
    if (hits) *st = (unsigned long long)after;
    uint32_t m_before;
    ecc_decode(before & 0xFFFFu, before >> kEccDataBits, &m_before);
    const int status = ecc_decode(after & 0xFFFFu, after >> kEccDataBits, &m);
    fixed = status == 1;
    seen = status == 2;
    if (m != m_before) {
      uint32_t *const row = reinterpret_cast<uint32_t *>(copies + (size_t)run * stride + L.offset) + (size_t)n * L.row_dwords;
      const int32_t T = (int16_t)(uint16_t)(raw[t] ^ m);
      const uint32_t v = (uint32_t)packed_threshold(arith, signed_bb, 64 * (int)L.kw, T);
      row[i] = v;
      if (nthr == 1) row[1] = v;
    }
  }
  unsigned c = __popc(m);
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    c += __shfl_xor(c, d, 64);
    phys += __shfl_xor(phys, d, 64);
    fixed += __shfl_xor(fixed, d, 64);
    seen += __shfl_xor(seen, d, 64);
  }
  if ((threadIdx.x & 63) == 0 && (phys | c | fixed | seen)) {
    unsigned long long *const at = counts + (size_t)run * run_stride + (size_t)L.layer * 4 + 2;
    unsigned long long *const ec = ecc + (size_t)run * ecc_stride + (size_t)L.layer * 2;
    if (phys) atomicAdd(at, (unsigned long long)phys);
    if (c) atomicAdd(at + 1, (unsigned long long)c);
    if (fixed) atomicAdd(ec, (unsigned long long)fixed);
    if (seen) atomicAdd(ec + 1, (unsigned long long)seen);
  }
}

}  // namespace

hipError_t emem_noise_t(uint8_t *copies, size_t stride, int runs, const unsigned long long *seeds, const MemNoiseLayer &L, int nthr, Arith arith,
                        bool signed_bb, const uint16_t *raw, int interleave, int burst, uint32_t rate_q32, int epoch, unsigned long long *state,
                        unsigned long long *counts, size_t run_stride, unsigned long long *ecc, size_t ecc_stride, hipStream_t s) {
  if (runs <= 0 || rate_q32 == 0) return hipSuccess;
  if (runs > 65535 || L.rows == 0 || stride % 256 || L.offset % 4 || nthr < 1 || nthr > 2 || L.row_dwords < 2 || arith == AR_INT8 || !raw ||
      (interleave != 0 && interleave != HS_INTERLEAVED) || burst < 1 || burst > kMaxBurst || L.pe == 0 || L.rows != L.pe * L.tmem || epoch < 0 ||
      epoch >= kMaxEpochs || !state || (uintptr_t)state % 8 || !counts || !ecc)
    return hipErrorInvalidValue;
  const dim3 g((L.rows * (unsigned)nthr + kBlock - 1) / kBlock, (unsigned)runs);
  hipLaunchKernelGGL(k_emem_noise_t, g, dim3(kBlock), 0, s, copies, (unsigned long long)stride, L, (unsigned)nthr, arith, signed_bb, raw,
                     (unsigned)interleave, (unsigned)burst, seeds, rate_q32, (unsigned)epoch, state, counts, (unsigned long long)run_stride, ecc,
                     (unsigned long long)ecc_stride);
  return hipGetLastError();
}

}  // namespace bnn
