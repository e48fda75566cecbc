// scan_mfma_kernels.hip -- stages 1-3 of the clip scan on the matrix cores (scan_mfma_kernels.h; DESIGN.md 9 "Clip scan").
//
// The arithmetic is k_conv_mfma's (kernels.hip): +-1 activations and weights as FP4 E2M1 (0x2 / 0xA), one
// v_mfma_scale_f32_32x32x64_f8f6f4 per tap and 64 channels (32 neurons x 32 pixels), f32 accumulators seeded with
// -(theta + 1) from the layer's operand table, sign bit = !fire.  What differs is the picture: a map here is one large
// picture whose width and height are known at run time, and a launch holds many maps of different sizes.
//   * A BLOCK (256 threads, four waves) owns a band of one map: up to kClipMfmaRowPairs (8) output row pairs x up to
//     kClipMfmaChunk (64) conv-output columns.  It finds its band (map, first row pair, first column) and the map's
//     descriptor in the tables of scan_clip.h (ClipMfmaBand, ClipMfmaMap) through scalar loads.
//   * The band's input patch, (2 row pairs + 2) rows x (columns + 2) columns x CD dwords, is read once from HBM, a row
//     per wave and a dword per lane, and expanded bit -> FP4 through a 256-entry LDS table into planes
//     [32-channel block q][row][column] x 16 bytes, rows 66 slots apart.  A tile is 32 consecutive columns of ONE row,
//     so the 16 lanes of a ds_read_b128 group read 16 consecutive slots (256 bytes: every bank once) whatever the row
//     stride is; lanes clamped at the band's last column repeat an address, which the LDS broadcasts.
//   * A WAVE owns one neuron tile for the whole kernel: 9 CD / 2 k steps of FP4 weights in 36 / 36 / 72 VGPRs.  With two
//     neuron tiles (layer 1) waves w and w + 2 share a tile and take alternate pixel tiles.
//   * A TILE is 32 columns of one output row pair.  Per 64-channel step and tap column: four ds_read_b128 (input rows
//     2rp .. 2rp + 3) feed six MFMAs (output rows 2rp, 2rp + 1 x ky); the reads of a column are issued behind the
//     MFMAs of the column before, into a second register set (as in k_conv_mfma).
//   * Epilogue: sign bits -> one dword per 32 neurons.  Pool: AND of the two rows' sign bits, AND with lane c ^ 1 (tiles
//     start on even columns), the even lane stores pooled pixel (rp, x / 2).  No pool: lane half h stores row 2rp + h.
//     Lanes past the band's last column store nothing.
// No scratch, no spills; outputs are k_clip_quad's bit-packed HWC words at the same offsets.
#include "scan_mfma_kernels.h"

namespace bnn {
namespace {

typedef int v8i __attribute__((ext_vector_type(8)));
typedef float v16f __attribute__((ext_vector_type(16)));
typedef const ClipMfmaMap __attribute__((address_space(4))) *kptr_mmap;
typedef const ClipMfmaBand __attribute__((address_space(4))) *kptr_band;

// ---- the helpers of kernels.hip this kernel is written with (copies: that file's are in its anonymous namespace) ----
// bits = (bits << 1) | (v < 0)
__device__ __forceinline__ uint32_t shift_in_sign(uint32_t bits, int v) {
  asm("" : "+v"(v));
  return __builtin_amdgcn_alignbit(bits, (uint32_t)v, 31);
}
// sign bits of the 16 accumulators of one lane -> bits 8g + 4h + q of a dword (other bits 0)
__device__ __forceinline__ uint32_t sign_nibbles(const int (&v)[16], int h) {
  uint32_t x = 0;
#pragma unroll
  for (int g = 3; g >= 0; g--) {
#pragma unroll
    for (int q = 3; q >= 0; q--) x = shift_in_sign(x, v[4 * g + q]);
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

// CD: input dwords per pixel (2: 64 channels, 4: 128), NT: neuron tiles (output dwords per pixel), POOL: 2 x 2 max-pool behind
template <int CD, int NT, bool POOL>
__global__ __launch_bounds__(256, 2) void k_clip_conv_mfma(const uint8_t *__restrict__ in, uint8_t *__restrict__ out, const uint8_t *__restrict__ tab,
                                                            const ClipMfmaMap *__restrict__ maps, const ClipMfmaBand *__restrict__ bands) {
  constexpr int KH = CD / 2, KS = 9 * KH, NS = 3 * KH, STREAMS = 4 / NT;
  constexpr int ROWS = 2 * kClipMfmaRowPairs + 2, WS = kClipMfmaChunk + 2, PIXS = ROWS * WS;
  static_assert((NT == 2 || NT == 4) && (CD == 2 || CD == 4) && kClipMfmaChunk % 32 == 0, "tile geometry");
  static_assert(sizeof(uint4) * CD * PIXS + 1024 == clip_mfma_lds_bytes(CD), "the header states the LDS");
  __shared__ uint4 plane[CD * PIXS];  // [32-channel block q][row][column], strides PIXS, WS, 1
  __shared__ uint32_t lut[256];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), mt = wave % NT, c = lane & 31, h = lane >> 5;
  lut[tid] = fp4_pm1((uint32_t)tid);
  // the block's band and its map (wave-uniform: scalar loads)
  const kptr_band bq = (kptr_band)(uintptr_t)bands + blockIdx.x;
  const int rp0 = bq->rp0, x0 = bq->x0;
  const kptr_mmap mq = (kptr_mmap)(uintptr_t)maps + bq->map;
  const long long in_off = mq->in_off, out_off = mq->out_off;
  const int iw = mq->iw, ow = mq->ow, row_pairs = mq->row_pairs;
  const int cols = min(kClipMfmaChunk, ow - x0), nrp = min(kClipMfmaRowPairs, row_pairs - rp0);
  // weights [k step = tap * KH + kh][neuron tile][lane] x 16 bytes, then the seeds [tile][h][16] floats
  const uint4 *__restrict__ wt = reinterpret_cast<const uint4 *>(tab);
  v8i wreg[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ks++) {
    const uint4 v = wt[(ks * NT + mt) * 64 + lane];
    wreg[ks] = v8i{(int)v.x, (int)v.y, (int)v.z, (int)v.w, 0, 0, 0, 0};
  }
  const v16f seed = reinterpret_cast<const v16f *>(tab + (size_t)KS * NT * 64 * 16)[mt * 2 + h];
  __syncthreads();  // the expansion table
  // the patch: input rows 2 rp0 .. 2 rp0 + 2 nrp + 1, columns x0 .. x0 + cols + 1, all inside the map (iw = ow + 2 columns,
  // 2 row_pairs + 2 rows).  A row of the patch is one run of (cols + 2) CD dwords: a row per wave, a dword per lane.
  {
    const uint32_t *__restrict__ src = reinterpret_cast<const uint32_t *>(in + in_off) + ((size_t)(2 * rp0) * iw + x0) * CD;
    const int prows = 2 * nrp + 2, rowdw = (cols + 2) * CD;
    for (int r = wave; r < prows; r += 4) {
      const uint32_t *__restrict__ row = src + (size_t)r * iw * CD;
      for (int e = lane; e < rowdw; e += 64) {  // source dword e: 32-channel block e % CD of column e / CD
        const uint32_t bits = row[e];
        plane[(e % CD) * PIXS + r * WS + e / CD] = make_uint4(lut[bits & 255], lut[(bits >> 8) & 255], lut[(bits >> 16) & 255], lut[bits >> 24]);
      }
    }
  }
  __syncthreads();
  uint32_t *__restrict__ o = reinterpret_cast<uint32_t *>(out + out_off);
  const int ntx = (cols + 31) >> 5, ntiles = nrp * ntx;  // tiles of the band: (row pair, 32 columns), columns inner
  for (int t = wave / NT; t < ntiles; t += STREAMS) {
    const int rpl = ntx == 2 ? t >> 1 : t, xt = ntx == 2 ? (t & 1) * 32 : 0;
    const bool valid = xt + c < cols;
    // (lanes past the band's last column read that column: inside the patch, results dropped)
    const uint4 *__restrict__ P = &plane[h * PIXS + 2 * rpl * WS + (valid ? xt + c : cols - 1)];
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
    const int rp = rp0 + rpl, x = x0 + xt + c;
    if constexpr (POOL) {
      // vertical pool: the sign bit of the AND of the two bit patterns is "both negative" (finite values: |sum| <= 1152 + 1154)
      int v[16];
#pragma unroll
      for (int k = 0; k < 16; k++) v[k] = __float_as_int(acc[0][k]) & __float_as_int(acc[1][k]);
      const uint32_t nf = or_halves(sign_nibbles(v, h));
      const uint32_t pooled = nf & (uint32_t)__builtin_amdgcn_mov_dpp((int)nf, 0xB1, 0xF, 0xF, true);  // & lane c ^ 1
      if (valid && h == 0 && !(c & 1)) o[((size_t)rp * (ow >> 1) + (x >> 1)) * NT + mt] = ~pooled;
    } else {
      uint32_t nf[2];
#pragma unroll
      for (int dy = 0; dy < 2; dy++) {
        int v[16];
#pragma unroll
        for (int k = 0; k < 16; k++) v[k] = __float_as_int(acc[dy][k]);
        nf[dy] = sign_nibbles(v, h);  // this half's 16 neurons of output row 2rp + dy
      }
      // half h stores row 2rp + h: one swap hands half 0's row-1 bits to half 1 and half 1's row-0 bits to half 0
      const auto sw = __builtin_amdgcn_permlane32_swap(nf[0], nf[1], false, false);
      if (valid) o[((size_t)(2 * rp + h) * ow + x) * NT + mt] = ~(sw[0] | sw[1]);
    }
  }
}

}  // namespace

hipError_t launch_clip_conv_mfma(int stage, const ClipMfmaLaunch &a) {
  if (stage < 1 || stage > 3 || a.blocks < 1 || a.blocks > INT32_MAX || !a.tab) return hipErrorInvalidValue;
  const dim3 grid((unsigned)a.blocks), block(256);
  const ClipMfmaMap *maps = reinterpret_cast<const ClipMfmaMap *>(a.maps);
  const ClipMfmaBand *bands = reinterpret_cast<const ClipMfmaBand *>(a.bands);
  if (stage == 1) hipLaunchKernelGGL((k_clip_conv_mfma<2, 2, true>), grid, block, 0, a.stream, a.in, a.out, a.tab, maps, bands);
  else if (stage == 2) hipLaunchKernelGGL((k_clip_conv_mfma<2, 4, false>), grid, block, 0, a.stream, a.in, a.out, a.tab, maps, bands);
  else hipLaunchKernelGGL((k_clip_conv_mfma<4, 4, true>), grid, block, 0, a.stream, a.in, a.out, a.tab, maps, bands);
  return hipGetLastError();
}

}  // namespace bnn
