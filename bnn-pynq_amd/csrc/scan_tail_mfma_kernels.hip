// scan_tail_mfma_kernels.hip -- stages 4 and 5 of the clip scan on the matrix cores (scan_tail_mfma_kernels.h; DESIGN.md 9
// "Clip scan").
//
// The arithmetic is k_tail_mfma's and k_clip_conv_mfma's: +-1 activations and weights as FP4 E2M1 (0x2 / 0xA), one
// v_mfma_scale_f32_32x32x64_f8f6f4 with unit scales per tap and 64 channels (32 neurons x 32 pixels), f32 accumulators
// seeded with -(theta + 1) from the layer's operand table (kernels.h: kTailMfmaL4Off, kTailMfmaL5Off; k step = tap * KH +
// 64-channel block, KH = 2 / 4: 18 / 36 steps, eight neuron tiles), sign bit = !fire.  Sums of at most 2 304 terms of +-1
// plus the seed are exact in f32.  What is this kernel's own is the geometry: 256 neurons, no pool, and maps that are
// small and ragged (75 x 55, 46 x 33, down to 1 x 1), many of them in one launch.
//   * A BLOCK (512 threads, eight waves) owns a band of one map: up to kClipTailRowPairs (4) pairs of output rows x up to
//     kClipTailCols (64) columns, equal shares of the map (scan_clip.h).  It finds the band (ClipTailBand) and the map's
//     descriptor (ClipTailMap) through scalar loads.
//   * A WAVE owns one of the eight neuron tiles for the whole band: all 18 / 36 k steps of its FP4 weights stay in 72 /
//     144 VGPRs.  Eight waves are two a SIMD, 256 VGPRs each: one block a CU.
//   * The band's input patch, (2 row pairs + 2) rows x (columns + 2) columns x CD dwords, is read once from HBM, a row
//     per wave and a dword per lane, and expanded bit -> FP4 through a 256-entry LDS table into planes
//     [32-channel block q][row][column] x 16 bytes, rows 66 slots apart.
//   * A TILE is 32 consecutive PIXEL PAIRS of the band in row-pair-major order: pair p is column p % cols of row pair
//     p / cols and stands for the output pixels (2 rp, x) and (2 rp + 1, x).  A tile may therefore straddle row pairs, and
//     a band of nrp x cols pairs is ceil(nrp cols / 32) tiles: only the band's last tile has idle lanes, whatever the width
//     (tiles of 32 columns of ONE row pair would idle 21 of 96 lanes on a 75-wide map and 18 of 64 on a 46-wide one).
//     Every lane computes its own LDS address (one integer division per tile).  The vertical pairing is kept because it
//     is what makes the LDS port suffice: per 64-channel step and tap column, four ds_read_b128 (input rows 2rp .. 2rp + 3)
//     feed six MFMAs (output rows 2rp, 2rp + 1 x ky), against one read per MFMA for single pixels.  All eight waves read
//     the same patch, so a CU issues 16 reads (8 LDS cycles each) per 24 MFMAs of a SIMD (32 cycles each): 128 of 192
//     cycles.  The reads of a step are issued behind the MFMAs of the step before, into a second register set.
//   * LDS bank conflicts: the 16 lanes of a ds_read_b128 group read 16 consecutive 16-byte slots (every bank once) unless
//     the tile's row-pair break falls inside the group; then the group's two runs lie (132 - cols) slots apart and overlap
//     in the banks unless that is a multiple of 16: at most one of a read's four groups, in tiles that straddle, takes a
//     second pass.  Lanes past the band's last pair repeat its address (a broadcast).
//   * An odd map height leaves the last row pair with one row.  Its second row's MFMAs run on a patch row that was not
//     loaded (LDS only: every FP4 pattern is a finite number) and its store is dropped; the patch load stops at the
//     map's last input row.
//   * Epilogue: sign bits -> one dword per 32 neurons; lane half h stores row 2rp + h.  No pool.
// No scratch, no spills; outputs are k_clip_vec's bit-packed HWC words, [oh][ow][8] dwords, at the same offsets.
#include "scan_tail_mfma_kernels.h"

namespace bnn {
namespace {

typedef int v8i __attribute__((ext_vector_type(8)));
typedef float v16f __attribute__((ext_vector_type(16)));
typedef const ClipTailMap __attribute__((address_space(4))) *kptr_tmap;
typedef const ClipTailBand __attribute__((address_space(4))) *kptr_tband;

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
// 8 bits -> 8 FP4 nibbles, bit i -> nibble i: 1 -> 0x2 (+1.0), 0 -> 0xA (-1.0)
__device__ __forceinline__ uint32_t fp4_pm1(uint32_t byte) {
  uint32_t t = ~byte & 0xFFu;
  t = (t | (t << 12)) & 0x000F000Fu;
  t = (t | (t << 6)) & 0x03030303u;
  t = (t | (t << 3)) & 0x11111111u;
  return (t << 3) + 0x22222222u;
}

constexpr int kWaves = 8, kNT = 8;  // one neuron tile per wave: 256 neurons

// CD: input dwords per pixel (4: layer 4's 128 channels, 8: layer 5's 256)
template <int CD>
__global__ __launch_bounds__(64 * kWaves, 1) void k_clip_tail_mfma(const uint8_t *__restrict__ in, uint8_t *__restrict__ out, const uint8_t *__restrict__ tab,
                                                                    const ClipTailMap *__restrict__ maps, const ClipTailBand *__restrict__ bands) {
  constexpr int KH = CD / 2, KS = 9 * KH, NS = 3 * KH;
  constexpr int ROWS = 2 * kClipTailRowPairs + 2, WS = kClipTailCols + 2, PIXS = ROWS * WS;
  static_assert(CD == 4 || CD == 8, "layers 4 and 5");
  static_assert(sizeof(uint4) * CD * PIXS + 1024 == clip_tail_lds_bytes(CD) && clip_tail_lds_bytes(CD) <= 160 * 1024, "the header states the LDS");
  __shared__ uint4 plane[CD * PIXS];  // [32-channel block q][row][column], strides PIXS, WS, 1
  __shared__ uint32_t lut[256];
  const int tid = threadIdx.x, lane = tid & 63, mt = __builtin_amdgcn_readfirstlane(tid >> 6), c = lane & 31, h = lane >> 5;
  if (tid < 256) lut[tid] = fp4_pm1((uint32_t)tid);
  // the block's band and its map (wave-uniform: scalar loads)
  const kptr_tband bq = (kptr_tband)(uintptr_t)bands + blockIdx.x;
  const int rp0 = bq->rp0, x0 = bq->x0;
  const kptr_tmap mq = (kptr_tmap)(uintptr_t)maps + bq->map;
  const long long in_off = mq->in_off, out_off = mq->out_off;
  const int ow = mq->ow, oh = mq->oh, iw = ow + 2;
  const int cols = min(mq->band_cols, ow - x0), nrp = min(mq->band_rps, ((oh + 1) >> 1) - rp0);
  // weights [k step = tap * KH + kh][neuron tile][lane] x 16 bytes, then the seeds [tile][h][16] floats
  const uint4 *__restrict__ wt = reinterpret_cast<const uint4 *>(tab);
  v8i wreg[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ks++) {
    const uint4 v = wt[(ks * kNT + mt) * 64 + lane];
    wreg[ks] = v8i{(int)v.x, (int)v.y, (int)v.z, (int)v.w, 0, 0, 0, 0};
  }
  const v16f seed = reinterpret_cast<const v16f *>(tab + (size_t)KS * kNT * 64 * 16)[mt * 2 + h];
  __syncthreads();  // the expansion table
  // the patch: input rows 2 rp0 .. 2 rp0 + 2 nrp + 1, less the one past the map's (oh + 2)-th when oh is odd, columns
  // x0 .. x0 + cols + 1 <= ow + 1.  A row of the patch is one run of (cols + 2) CD dwords: a row per wave, a dword per lane.
  {
    const uint32_t *__restrict__ src = reinterpret_cast<const uint32_t *>(in + in_off) + ((size_t)(2 * rp0) * iw + x0) * CD;
    const int prows = min(2 * nrp + 2, oh + 2 - 2 * rp0), rowdw = (cols + 2) * CD;
    for (int r = mt; r < prows; r += kWaves) {
      const uint32_t *__restrict__ row = src + (size_t)r * iw * CD;
      for (int e = lane; e < rowdw; e += 64) {  // source dword e: 32-channel block e % CD of column e / CD
        const uint32_t bits = row[e];
        plane[(e % CD) * PIXS + r * WS + e / CD] = make_uint4(lut[bits & 255], lut[(bits >> 8) & 255], lut[(bits >> 16) & 255], lut[bits >> 24]);
      }
    }
  }
  __syncthreads();
  uint32_t *__restrict__ o = reinterpret_cast<uint32_t *>(out + out_off);
  const int npairs = nrp * cols;
#pragma clang loop unroll(disable)
  for (int t0 = 0; t0 < npairs; t0 += 32) {
    const bool valid = t0 + c < npairs;
    const int p = valid ? t0 + c : npairs - 1;  // (lanes past the band's last pair read that pair: inside the patch, results dropped)
    const int rpl = p / cols, xl = p - rpl * cols;
    const uint4 *__restrict__ P = &plane[h * PIXS + 2 * rpl * WS + xl];
    v16f acc[2] = {seed, seed};  // output rows 2rp, 2rp + 1
    // step s = 3 kh + kx: input rows 2rp .. 2rp + 3 at column x + kx of channel block 2 kh + h, then the 6 MFMAs of
    // output rows 2rp, 2rp + 1 x ky
    auto read = [&](v8i &b, int s, int y) {
      const uint4 v = P[(s / 3) * 2 * PIXS + y * WS + s % 3];
      b = v8i{(int)v.x, (int)v.y, (int)v.z, (int)v.w, 0, 0, 0, 0};
    };
    auto mfma = [&](const v8i (&b)[4], int s, int k) {  // k = 2 ky + dy
      acc[k & 1] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(wreg[((k >> 1) * 3 + s % 3) * KH + s / 3], b[(k >> 1) + (k & 1)], acc[k & 1], 4, 4, 0,
                                                                  0x7F7F7F7F, 0, 0x7F7F7F7F);
    };
    // the four reads of step s + 1 go out behind the first four MFMAs of step s, into the other register set; the
    // scheduling barriers keep that order
    v8i b[2][4];
#pragma unroll
    for (int y = 0; y < 4; y++) read(b[0][y], 0, y);
#pragma unroll
    for (int s = 0; s < NS; s++)
#pragma unroll
      for (int k = 0; k < 6; k++) {
        __builtin_amdgcn_sched_barrier(0);
        mfma(b[s & 1], s, k);
        if (s + 1 < NS && k < 4) read(b[(s + 1) & 1][k], s + 1, k);
      }
    __builtin_amdgcn_sched_barrier(0);
    // half h stores row 2rp + h: one swap hands half 0's row-1 bits to half 1 and half 1's row-0 bits to half 0
    const auto sw = __builtin_amdgcn_permlane32_swap(sign_nibbles(acc[0], h), sign_nibbles(acc[1], h), false, false);
    const int y = 2 * (rp0 + rpl) + h;
    if (valid && y < oh) o[((size_t)y * ow + x0 + xl) * kNT + mt] = ~(sw[0] | sw[1]);
  }
}

}  // namespace

hipError_t launch_clip_tail_mfma(int stage, const ClipTailLaunch &a) {
  if (stage < 4 || stage > 5 || a.blocks < 1 || a.blocks > INT32_MAX || !a.tab) return hipErrorInvalidValue;
  const dim3 grid((unsigned)a.blocks), block(64 * kWaves);
  const ClipTailMap *maps = reinterpret_cast<const ClipTailMap *>(a.maps);
  const ClipTailBand *bands = reinterpret_cast<const ClipTailBand *>(a.bands);
  if (stage == 4) hipLaunchKernelGGL((k_clip_tail_mfma<4>), grid, block, 0, a.stream, a.in, a.out, a.tab, maps, bands);
  else hipLaunchKernelGGL((k_clip_tail_mfma<8>), grid, block, 0, a.stream, a.in, a.out, a.tab, maps, bands);
  return hipGetLastError();
}

}  // namespace bnn
