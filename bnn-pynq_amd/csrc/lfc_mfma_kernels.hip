// lfc_mfma_kernels.hip -- the four layers of lfcW1A1 and lfcW1A2 on the matrix cores (lfc_mfma_kernels.h; DESIGN.md 5 "The
// matrix pipe", "LFC").
//
// The arithmetic is k_tail_mfma's (kernels.hip): activations and weights as FP4 E2M1, one
// v_mfma_scale_f32_32x32x64_f8f6f4 with unit scales per 64 synapses (32 neurons x 32 images), f32 accumulators seeded from
// the layer's operand table, the decision read off the sign bit.
//   * 1-bit activations (lfcW1A1, and layer 0 of lfcW1A2): bit 1 -> +1 (0x2), bit 0 -> -1 (0xA), eight at a time through a
//     256-entry LDS table (fp4_pm1).  Layer 0's 13 words include the reference's 48 padding inputs (bit 0 = -1): its
//     thresholds count them against the weight memories' own bits, so they are synapses like the others here.
//   * 2-bit activations (lfcW1A2 layers 1-3): (sign, non-zero) planes -> +1 / -1 / 0 (0x2 / 0xA / 0x0) through two tables
//     (fp4_planes), as cnvW1A2's.
//   * One threshold (!OUT2): seed -(theta + 1) (XNOR rows, d - theta even) or -(t0 + 1/2) (lfcW1A2's last layer), sign bit
//     = !fire.  Two thresholds (OUT2): one v_sub_f32 with the second table gives the second decision's value; the planes are
//     sign = ~(f0 | f1), non-zero = ~(f0 ^ f1), as finish_bits forms them.
//   * Exactness: |d| <= K = 832 or 1024 for 1-bit activations, <= 1024 for 2-bit ones against +-1 weights (the bound used
//     is the looser 3 * 1024); the table kernels clamp the thresholds to the range d can reach, which changes no decision.
//     Seeds, every partial sum and the second threshold's distance are multiples of 1/2 below 2^14: f32 represents them all
//     and every addition is exact, in whatever order the matrix core sums.  A decision value is an odd integer or an odd
//     multiple of 1/2, never zero: the sign bit read is never a zero's.
// What is this kernel's own is the work split.  A hidden layer is 32 neuron tiles x 16 k steps: 2 048 VGPRs of weights, so
// no wave can own a neuron tile's share of them the way k_tail_mfma's do (NT / WAVES x KS x 4 = 256 VGPRs at 8 waves).
//   * A BLOCK (512 threads, eight waves) owns a GROUP of G = 128 images and HALF of the neuron tiles: blockIdx & 1 picks
//     the half, blockIdx >> 1 the first group; groups are dealt round-robin over the grid's block pairs.  The two blocks of
//     a pair read the same source words (the second from L2).
//   * A WAVE owns 2 neuron tiles for the whole kernel: 2 x KS x 4 = 104 / 128 VGPRs of weights.  It walks the group's four
//     item tiles (32 images each); one ds_read_b128 per k step feeds both tiles' MFMAs.  Eight waves are two a SIMD, up to
//     256 VGPRs each: one block a CU.
//   * LAST layer (2 neuron tiles): every wave holds both, and the waves split the group's item tiles among themselves (wave
//     w takes tile w: four of the eight have MFMAs to issue; all eight expand).  One block per group.
//   * The group's source words are expanded once per block into LDS planes [32-synapse block q = 2 ks + h][image] x 16
//     bytes, rows padded by one entry (consecutive threads write consecutive q: the pad spreads them over the banks); lane
//     (c, h) reads entry c of row 2 ks + h -- consecutive lanes, consecutive 16 bytes.  The NEXT group's words are requested
//     into registers before this group's MFMAs are issued.
//   * Seeds (and the second table) are read from LDS at the head of every item tile: kept in VGPRs they would cost 32 (64).
//   * Items past the last image repeat the last valid one and store nothing.
//   * Epilogue: a wave's two tiles are the two halves of one output u64: one 8-byte store per image from lane half 0
//     (1-bit out), or plane h from lane half h (2-bit out).  Vector stores only.
// Built for gfx950 (-O3, amdgpu-mfma-vgpr-form; -Rpass-analysis=kernel-resource-usage), <IN2, OUT2, KS, NT>: VGPRs / SGPRs /
// static LDS bytes / scratch, two waves a SIMD everywhere, no spills --
//   lfcW1A1  L0 <0,0,13,32> 234 / 26 / 56 768 / 0   L1-2 <0,0,16,32> 244 / 26 / 69 120 / 0   L3 <0,0,16,2> 230 / 30 / 67 328 / 0
//   lfcW1A2  L0 <0,1,13,32> 232 / 26 / 58 816 / 0   L1-2 <1,1,16,32> 256 / 26 / 72 192 / 0   L3 <1,0,16,2> 228 / 31 / 68 352 / 0
// (<1,1,16,32> sits at the register limit: forming the second decision's 16 differences before reading their signs spilled
// 12 VGPRs; sign_nibbles_sub reads them one at a time.)
// Measured (profiles/r38_lfc_mfma_rate.txt, stage events at 131 072 images, us, this kernel vs k_vec_x / k_vec): lfcW1A1 L0
// 50.2 vs 155.6, L1 58.7 vs 186.8, L2 58.2 vs 185.8, L3 22.7 vs 19.5; lfcW1A2 59.1 vs 160.9, 76.8 vs 207.1, 75.6 vs 206.7,
// 31.1 vs 23.0.  The last layer loses: 128 blocks of four working waves; a twentieth of the pass either way.
#include "lfc_mfma_kernels.h"

#include <type_traits>

namespace bnn {
namespace {

typedef int v8i __attribute__((ext_vector_type(8)));
typedef float v16f __attribute__((ext_vector_type(16)));

// ---- the helpers of kernels.hip this kernel is written with (copies: that file's are in its anonymous namespace) ----
// bits = (bits << 1) | (v < 0)
__device__ __forceinline__ uint32_t shift_in_sign(uint32_t bits, int v) {
  asm("" : "+v"(v));
  return __builtin_amdgcn_alignbit(bits, (uint32_t)v, 31);
}
// sign bits of the 16 accumulators of one lane -> bits 8g + 4h + q of a dword (other bits 0)
__device__ __forceinline__ uint32_t sign_nibbles(const v16f &a, int h) {
  uint32_t x = 0;
#pragma unroll
  for (int g = 3; g >= 0; g--) {
#pragma unroll
    for (int q = 3; q >= 0; q--) x = shift_in_sign(x, __float_as_int(a[4 * g + q]));
    if (g) x <<= 4;
  }
  return x << (4 * h);
}
// the same of a - d, one difference at a time (the second decision: 16 VGPRs less than forming the differences first)
__device__ __forceinline__ uint32_t sign_nibbles_sub(const v16f &a, const v16f &d, int h) {
  uint32_t x = 0;
#pragma unroll
  for (int g = 3; g >= 0; g--) {
#pragma unroll
    for (int q = 3; q >= 0; q--) x = shift_in_sign(x, __float_as_int(a[4 * g + q] - d[4 * g + q]));
    if (g) x <<= 4;
  }
  return x << (4 * h);
}
// OR with the partner lane l ^ 32
__device__ __forceinline__ uint32_t or_halves(uint32_t x) {
  const auto sw = __builtin_amdgcn_permlane32_swap(x, x, false, false);
  return sw[0] | sw[1];
}
// 8 bits -> 8 FP4 nibbles, bit i -> nibble i: 1 -> 0x2 (+1.0), 0 -> 0xA (-1.0)
__device__ __forceinline__ uint32_t fp4_pm1(uint32_t byte) {
  uint32_t t = ~byte & 0xFFu;
  t = (t | (t << 12)) & 0x000F000Fu;
  t = (t | (t << 6)) & 0x03030303u;
  t = (t | (t << 3)) & 0x11111111u;
  return (t << 3) + 0x22222222u;
}
// bit i of a byte -> 0x1 in nibble i
__device__ __forceinline__ uint32_t nibble_spread(uint32_t byte) {
  uint32_t t = byte & 0xFFu;
  t = (t | (t << 12)) & 0x000F000Fu;
  t = (t | (t << 6)) & 0x03030303u;
  return (t | (t << 3)) & 0x11111111u;
}
// 32 synapses (non-zero bits nz, sign bits sg) -> 32 FP4 nibbles through the two tables: 2 * [nz] + 8 * [nz & sign]
__device__ __forceinline__ uint4 fp4_planes(const uint32_t *lutz, const uint32_t *luts, uint32_t sg, uint32_t nz) {
  const uint32_t m = sg & nz;
  return make_uint4(lutz[nz & 255] | luts[m & 255], lutz[(nz >> 8) & 255] | luts[(m >> 8) & 255],
                    lutz[(nz >> 16) & 255] | luts[(m >> 16) & 255], lutz[nz >> 24] | luts[m >> 24]);
}

constexpr int kWaves = kLfcMfmaWaves, kG = kLfcMfmaGroup, kTPW = kLfcMfmaTilesPerWave, kT = 64 * kWaves;
static_assert(kLfcMfmaItemTile == 32 && kG % 32 == 0 && kTPW == 2, "the MFMA's item tile; a wave's two tiles make one output u64");

// IN2: 2-bit source words ([image][KS][plane] u64), else 1-bit ([image][KS] u64); OUT2: two thresholds, 2-bit words out;
// KS: k steps; NT: the layer's neuron tiles (2: the last layer's split)
template <bool IN2, bool OUT2, int KS, int NT>
__global__ __launch_bounds__(kT, 1) void k_lfc_mfma(const std::conditional_t<IN2, uint4, uint32_t> *__restrict__ in, uint2 *__restrict__ out,
                                                     const uint8_t *__restrict__ tab, int n_images) {
  using U = std::conditional_t<IN2, uint4, uint32_t>;  // source unit: 64 synapses in two planes, or 32 synapses
  constexpr bool LAST = NT == kTPW;
  constexpr int NB = LAST ? kTPW : kTPW * kWaves, PARTS = NT / NB;  // neuron tiles per block; blocks that share a group
  constexpr int UPI = IN2 ? KS : 2 * KS, GP = kG + 1, NPF = (kG * UPI + kT - 1) / kT, NC = (OUT2 ? 2 : 1) * NB * 2;
  static_assert(NT % NB == 0 && (LAST || kG / 32 <= kWaves), "work split");
  static_assert(sizeof(uint4) * 2 * KS * GP + 4 * (IN2 ? 512 : 256) + 64 * NC <= 160 * 1024, "LDS of one block");
  __shared__ uint4 plane[2 * KS * GP];        // [32-synapse block q][image], rows GP apart
  __shared__ uint32_t lut[IN2 ? 512 : 256];   // IN2: lutz, then luts (fp4_planes)
  __shared__ v16f cst[NC];                    // the block's seeds [tile][h], then (OUT2) the second table [tile][h]
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), c = lane & 31, h = lane >> 5;
  const int part = blockIdx.x % PARTS, stride = gridDim.x / PARTS;
  const int lt0 = LAST ? 0 : wave * kTPW, mt0 = part * NB + lt0;  // the wave's first tile: in the block, in the layer (even)
  for (int k = tid; k < 256; k += kT) {
    if constexpr (IN2) {
      lut[k] = nibble_spread((uint32_t)k) << 1;
      lut[256 + k] = nibble_spread((uint32_t)k) << 3;
    } else {
      lut[k] = fp4_pm1((uint32_t)k);
    }
  }
  {
    const float *__restrict__ src = reinterpret_cast<const float *>(tab + (size_t)KS * NT * 64 * 16);
    for (int k = tid; k < NB * 32; k += kT) {
      reinterpret_cast<float *>(cst)[k] = src[part * NB * 32 + k];
      if constexpr (OUT2) reinterpret_cast<float *>(cst)[NB * 32 + k] = src[NT * 32 + part * NB * 32 + k];
    }
  }
  // weights [k step][neuron tile][lane] x 16 bytes
  const uint4 *__restrict__ wt = reinterpret_cast<const uint4 *>(tab);
  v8i wreg[kTPW][KS];
#pragma unroll
  for (int j = 0; j < kTPW; j++)
#pragma unroll
    for (int ks = 0; ks < KS; ks++) {
      const uint4 v = wt[(ks * NT + mt0 + j) * 64 + lane];
      wreg[j][ks] = v8i{(int)v.x, (int)v.y, (int)v.z, (int)v.w, 0, 0, 0, 0};
    }
  const int ngroups = (n_images + kG - 1) / kG;
  U pre[NPF];
  auto fetch = [&](int grp) {
    const int img0 = grp * kG, lim = min(kG, n_images - img0) * UPI;
#pragma unroll
    for (int j = 0; j < NPF; j++) {
      const int d = tid + kT * j;
      pre[j] = d < lim ? in[(size_t)img0 * UPI + d] : U{};
    }
  };
  const int grp0 = blockIdx.x / PARTS;
  if (grp0 < ngroups) fetch(grp0);
  for (int grp = grp0; grp < ngroups; grp += stride) {
    const int img0 = grp * kG, nimg = min(kG, n_images - img0);
    __syncthreads();  // the previous group's planes are no longer read (first pass: lut and cst are written)
#pragma unroll
    for (int j = 0; j < NPF; j++) {
      const int d = tid + kT * j;
      if (d < nimg * UPI) {
        const int i = d / UPI, e = d - i * UPI;
        if constexpr (IN2) {  // one source uint4: sign lo, hi, non-zero lo, hi of 64 synapses
          const uint4 v = pre[j];
          plane[2 * e * GP + i] = fp4_planes(lut, lut + 256, v.x, v.z);
          plane[(2 * e + 1) * GP + i] = fp4_planes(lut, lut + 256, v.y, v.w);
        } else {  // one source dword: 32 synapses
          const uint32_t bits = pre[j];
          plane[e * GP + i] = make_uint4(lut[bits & 255], lut[(bits >> 8) & 255], lut[(bits >> 16) & 255], lut[bits >> 24]);
        }
      }
    }
    if (grp + stride < ngroups) fetch(grp + stride);
    __syncthreads();
#pragma clang loop unroll(disable) interleave(disable) vectorize(disable)
    for (int t0 = LAST ? wave * 32 : 0; t0 < nimg; t0 += LAST ? kWaves * 32 : 32) {
      const int item = min(t0 + c, nimg - 1);
      v16f acc[kTPW];
#pragma unroll
      for (int j = 0; j < kTPW; j++) acc[j] = cst[(lt0 + j) * 2 + h];
#pragma unroll
      for (int ks = 0; ks < KS; ks++) {
        const uint4 v = plane[(2 * ks + h) * GP + item];
        const v8i b = v8i{(int)v.x, (int)v.y, (int)v.z, (int)v.w, 0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < kTPW; j++)
          acc[j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(wreg[j][ks], b, acc[j], 4, 4, 0, 0x7F7F7F7F, 0, 0x7F7F7F7F);
      }
      // the image's words: NT / 2 u64 (1-bit out), NT / 2 pairs of planes (2-bit out); this wave's tiles are u64 mt0 / 2
      const bool valid = t0 + c < nimg;
      const size_t w64 = (size_t)(img0 + item) * (NT / 2) + mt0 / 2;
      if constexpr (OUT2) {
        uint32_t w[kTPW];
#pragma unroll
        for (int j = 0; j < kTPW; j++) {
          const uint32_t n0 = or_halves(sign_nibbles(acc[j], h));                                       // !fire0
          const uint32_t n1 = or_halves(sign_nibbles_sub(acc[j], cst[NB * 2 + (lt0 + j) * 2 + h], h));  // !fire1
          w[j] = h ? ~(n0 ^ n1) : (n0 & n1);  // lane half h stores plane h
        }
        if (valid) out[w64 * 2 + h] = make_uint2(w[0], w[1]);
      } else {
        const uint32_t lo = ~or_halves(sign_nibbles(acc[0], h)), hi = ~or_halves(sign_nibbles(acc[1], h));
        if (valid && h == 0) out[w64] = make_uint2(lo, hi);
      }
    }
  }
}

// one layer: `cap` groups in flight, PARTS blocks each
template <bool IN2, bool OUT2, int KS, int NT>
void launch(const void *in, void *out, const uint8_t *tab, int n, hipStream_t s) {
  constexpr int parts = NT == kTPW ? 1 : NT / (kTPW * kWaves);
  const long long groups = ((long long)n + kG - 1) / kG, per = (groups + kLfcMfmaGrid - 1) / kLfcMfmaGrid;
  const unsigned pairs = (unsigned)((groups + per - 1) / per);  // the groups dealt evenly: at most kLfcMfmaGrid block sets
  hipLaunchKernelGGL((k_lfc_mfma<IN2, OUT2, KS, NT>), dim3(pairs * parts), dim3(kT), 0, s,
                     static_cast<const std::conditional_t<IN2, uint4, uint32_t> *>(in), static_cast<uint2 *>(out), tab, n);
}

}  // namespace

hipError_t launch_lfc_mfma(NetId net, int layer, const void *in, void *out, const uint8_t *tab, int n, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  if ((net != NET_LFCW1A1 && net != NET_LFCW1A2) || layer < 0 || layer > 3) return hipErrorInvalidValue;
  const bool two = net == NET_LFCW1A2;
  const uint8_t *t = tab + lfc_mfma_offset(layer, two);
  if (!two) {
    if (layer == 0) launch<false, false, 13, 32>(in, out, t, n, s);
    else if (layer < 3) launch<false, false, 16, 32>(in, out, t, n, s);
    else launch<false, false, 16, 2>(in, out, t, n, s);
  } else {
    if (layer == 0) launch<false, true, 13, 32>(in, out, t, n, s);
    else if (layer < 3) launch<true, true, 16, 32>(in, out, t, n, s);
    else launch<true, false, 16, 2>(in, out, t, n, s);
  }
  return hipGetLastError();
}

}  // namespace bnn
