// repair_kernels.hip -- the repair scrub of the exposure campaigns (bnn_mi355x_repair_exposure_campaigns; the model:
// mem_org.h, "repair scrubs"; the code: ecc.h; declared in kernels.h).
// A translation unit of its own for the reason ecc_kernels.hip is one: built apart, kernels.o and ecc_kernels.o stay
// byte for byte what they were.
#include <hip/hip_runtime.h>
#include <stdint.h>

#define BNN_HD __host__ __device__  // (the shared headers' routines compile for the device here, as in kernels.hip)
#include "ecc.h"
#include "kernels.h"

namespace bnn {
namespace {

constexpr int kBlock = 256;  // (kernels.hip's block)

// k_repair_state: a lane per (layer-with-redundancy blockIdx.z, run blockIdx.y, state word).  The state words of
// k_xmem_noise_t and k_emem_noise_t are per lane, in logical-image order, so voting and decoding are lane-local: the lane
// loads its word, applies the error-pattern rule (TMR: the three masks become their majority; coded: ecc_repair of the
// data and check masks) and stores it only where it changed.  The grid's x covers the largest layer; the blocks past a
// layer's lanes exit as a whole, so a wave never straddles layers.  No LDS, no row rebuild, no copy: the delivered
// parameters are the same before and after.
__global__ __launch_bounds__(kBlock) void k_repair_state(uint8_t *__restrict__ camp, RepairTable tab, unsigned long long *__restrict__ rep,
                                                         unsigned long long rep_stride) {
  const RepairEntry E = tab.e[blockIdx.z];
  if (E.kind == RK_SKIP || blockIdx.x * kBlock >= E.lanes) return;
  const unsigned run = blockIdx.y, t = blockIdx.x * kBlock + threadIdx.x;
  unsigned wrote = 0, left = 0;
  if (t < E.lanes) {
    unsigned long long *const st = reinterpret_cast<unsigned long long *>(camp + E.state_off) + (size_t)run * E.lanes + t;
    const unsigned long long before = *st;
    unsigned long long after;
    if (E.kind == RK_TMR) {
      const uint32_t m0 = (uint32_t)before & 0xFFFFu, m1 = (uint32_t)(before >> 16) & 0xFFFFu, m2 = (uint32_t)(before >> 32) & 0xFFFFu;
      const uint32_t v = (m0 & m1) | (m0 & m2) | (m1 & m2);
      after = (unsigned long long)v | (unsigned long long)v << 16 | (unsigned long long)v << 32;
      wrote = after != before;
    } else {
      uint32_t d, c;
      wrote = ecc_repair((uint32_t)before & 0xFFFFu, (uint32_t)before >> kEccDataBits, &d, &c) == 1;
      after = (unsigned long long)(d | c << kEccDataBits);
    }
    left = after != 0;
    if (after != before) *st = after;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    wrote += __shfl_xor(wrote, d, 64);
    left += __shfl_xor(left, d, 64);
  }
  if ((threadIdx.x & 63) == 0 && (wrote | left)) {
    unsigned long long *const at = rep + (size_t)run * rep_stride + (size_t)E.layer * 2;
    if (wrote) atomicAdd(at, (unsigned long long)wrote);
    if (left) atomicAdd(at + 1, (unsigned long long)left);
  }
}

}  // namespace

hipError_t repair_state(uint8_t *camp, const RepairTable &tab, int entries, int runs, unsigned long long *rep, size_t rep_stride, hipStream_t s) {
  if (runs <= 0 || entries <= 0) return hipSuccess;
  if (runs > 65535 || entries > kRepairEntries || !camp || !rep) return hipErrorInvalidValue;
  uint32_t most = 0;
  for (int k = 0; k < entries; k++) {
    const RepairEntry &e = tab.e[k];
    if (e.kind > RK_CODED || e.state_off % 8 || (e.kind != RK_SKIP && e.lanes == 0)) return hipErrorInvalidValue;
    if (e.kind != RK_SKIP && e.lanes > most) most = e.lanes;
  }
  if (most == 0) return hipSuccess;
  const dim3 g((most + kBlock - 1) / kBlock, (unsigned)runs, (unsigned)entries);
  hipLaunchKernelGGL(k_repair_state, g, dim3(kBlock), 0, s, camp, tab, rep, (unsigned long long)rep_stride);
  return hipGetLastError();
}

}  // namespace bnn
