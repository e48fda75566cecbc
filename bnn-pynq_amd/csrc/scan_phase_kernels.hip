// scan_phase_kernels.hip -- stages 2 and 3 of the fine clip scan on the matrix cores (scan_phase_kernels.h; DESIGN.md 9 "Fine scan").
//
// The arithmetic is k_clip_conv_mfma's (scan_mfma_kernels.hip): +-1 activations and weights as FP4 E2M1 (0x2 / 0xA), one
// v_mfma_scale_f32_32x32x64_f8f6f4 per tap and 64 channels (32 neurons x 32 pixels), f32 accumulators seeded with -(theta + 1)
// from the layer's operand table, sign bit = !fire.  The maps are not that kernel's: either side of a map can be odd, a map can
// be narrower than a tile, and layer 3 leaves FOUR pooled maps, one per pool phase, from one evaluation of its convolution.
//
//   * A pooled pixel of any phase is a 2 x 2 block of conv outputs, and every 2 x 2 block is one: the block that starts at conv
//     (r, c) is pixel (c >> 1, r >> 1) of phase (c & 1, r & 1).  So the pool is a 2 x 2 AND of !fire words at stride ONE, and
//     the phases are nothing but the parities of where a block starts.
//   * A BLOCK (256 threads, four waves) owns a band of one map (ClipPhaseBand, ClipPhaseMap: scalar loads): up to 16 conv rows
//     x up to two tiles of 32 conv columns.  Its input patch, (rows + 2) x (columns + 2) x CD dwords, is read once from HBM, a
//     row per wave and a dword per lane, and expanded bit -> FP4 through a 256-entry LDS table into planes
//     [32-channel block][row][column] x 16 bytes.  When the band has an odd number of rows the patch's last row is staged
//     twice, so that the row pair below reads defined values (its second row is never stored).
//   * A WAVE owns neuron tile `wave` (32 of the 128 or 256 neurons; 9 CD / 2 k steps of weights in registers) and walks the
//     band's column strips downwards: strip, then row pair.  A TILE is 32 columns of two conv rows: per 64-channel step and
//     tap column four ds_read_b128 (input rows 2rp .. 2rp + 3) feed six MFMAs, the reads of a step issued behind the MFMAs of
//     the step before.
//   * Epilogue.  Lane (h, c) ends with W, the !fire word of its 32 neurons at conv (row 2rp + h, column c).  Stage 2 stores ~W.
//     Stage 3: H = W & W of lane c + 1 (one ds_bpermute) pairs the columns; a swap of the wave's halves pairs row 2rp with
//     2rp + 1 (half 0 stores the block starting at row 2rp) and row 2rp with the row above, whose H half 1 CARRIES in a
//     register from the row pair before (half 1 stores the block starting at row 2rp - 1).  Nothing pooled passes through
//     LDS or HBM.  Lane 31 has no right neighbour in its tile and the first row pair no row above, so a tile owns 31 starts
//     and a band 15 start rows: tiles lie 31 columns apart and bands 15 rows (scan_fine.h), and one conv row in 16 and one
//     column in 32 are computed twice.
// No scratch, no spills; every store is a vector store of one dword.
#include "scan_phase_kernels.h"

namespace bnn {
namespace {

typedef int v8i __attribute__((ext_vector_type(8)));
typedef float v16f __attribute__((ext_vector_type(16)));
typedef const ClipPhaseMap __attribute__((address_space(4))) *kptr_pmap;
typedef const ClipPhaseBand __attribute__((address_space(4))) *kptr_pband;

// bits = (bits << 1) | (v < 0)
__device__ __forceinline__ uint32_t shift_in_sign(uint32_t bits, int v) {
  asm("" : "+v"(v));
  return __builtin_amdgcn_alignbit(bits, (uint32_t)v, 31);
}
// sign bits of the 16 accumulators of one lane -> bits 8g + 4h + q of a dword (other bits 0): the MFMA's 32 x 32 result
// holds neuron 8g + 4h + q of pixel c in accumulator 4g + q of lane (h, c)
__device__ __forceinline__ uint32_t sign_word(const v16f &acc, int h) {
  uint32_t x = 0;
#pragma unroll
  for (int g = 3; g >= 0; g--) {
#pragma unroll
    for (int q = 3; q >= 0; q--) x = shift_in_sign(x, __float_as_int(acc[4 * g + q]));
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

// CD: input dwords per pixel (2: 64 channels, 4: 128), NT: neuron tiles = waves (output dwords per pixel), PHASES: the four
// pooled phase maps instead of the conv map
template <int CD, int NT, bool PHASES>
__global__ __launch_bounds__(256, 2) void k_clip_conv_phase(const uint8_t *__restrict__ in, uint8_t *__restrict__ out, const uint8_t *__restrict__ tab,
                                                             const ClipPhaseMap *__restrict__ maps, const ClipPhaseBand *__restrict__ bands) {
  constexpr int KH = CD / 2, KS = 9 * KH, NS = 3 * KH;
  constexpr int ROWS = kPhaseRows + 2, WS = 2 * kPhaseTile + 2, PIXS = ROWS * WS, TSTEP = phase_tile_step(PHASES);
  static_assert(NT == 4 && (CD == 2 || CD == 4) && kPhaseTile == 32 && kPhaseRows % 2 == 0, "a wave per neuron tile, tiles of the MFMA's 32 pixels");
  static_assert(phase_band_span(PHASES) + 2 <= WS, "the band's patch fits the planes");
  static_assert(sizeof(uint4) * CD * PIXS + 1024 == clip_phase_lds_bytes(CD), "the header states the LDS");
  __shared__ uint4 plane[CD * PIXS];  // [32-channel block q][row][column], strides PIXS, WS, 1
  __shared__ uint32_t lut[256];
  const int tid = threadIdx.x, lane = tid & 63, mt = __builtin_amdgcn_readfirstlane(tid >> 6), c = lane & 31, h = lane >> 5;
  lut[tid] = fp4_pm1((uint32_t)tid);
  // the block's band and its map (wave-uniform: scalar loads)
  const kptr_pband bq = (kptr_pband)(uintptr_t)bands + blockIdx.x;
  const int y0 = bq->y0, x0 = bq->x0;
  const kptr_pmap mq = (kptr_pmap)(uintptr_t)maps + bq->map;
  const long long in_off = mq->in_off;
  const int iw = mq->iw, ow = mq->ow, oh = mq->oh;
  const int nrows = min(kPhaseRows, oh - y0), ncols = min(phase_band_span(PHASES), ow - x0), nrp = (nrows + 1) >> 1;
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
  // the patch: input rows y0 .. y0 + nrows + 1, columns x0 .. x0 + ncols + 1, all inside the map (ow + 2 columns, oh + 2
  // rows).  The row pairs read 2 nrp + 2 rows: with nrows odd the last one is the row above it again.
  {
    const uint32_t *__restrict__ src = reinterpret_cast<const uint32_t *>(in + in_off) + ((size_t)y0 * iw + x0) * CD;
    const int rowdw = (ncols + 2) * CD;
    for (int r = mt; r < 2 * nrp + 2; r += 4) {
      const uint32_t *__restrict__ row = src + (size_t)min(r, nrows + 1) * iw * CD;
      for (int e = lane; e < rowdw; e += 64) {  // source dword e: 32-channel block e % CD of column e / CD
        const uint32_t bits = row[e];
        plane[(e % CD) * PIXS + r * WS + e / CD] = make_uint4(lut[bits & 255], lut[(bits >> 8) & 255], lut[(bits >> 16) & 255], lut[bits >> 24]);
      }
    }
  }
  __syncthreads();
  // the strips of the band: 32 columns from xs on.  The pooled stage needs a column behind a start: ncols - 1 starts, 31 a strip
  const int strips = PHASES ? (ncols - 1 + TSTEP - 1) / TSTEP : (ncols + kPhaseTile - 1) / kPhaseTile;
  for (int xt = 0; xt < strips; xt++) {
    const int xs = xt * TSTEP, gc = x0 + xs + c;  // this lane's conv column
    const bool in_cols = xs + c < ncols;
    // (lanes past the band's last column read that column: inside the patch, results dropped)
    const uint4 *__restrict__ strip = &plane[h * PIXS + (in_cols ? xs + c : ncols - 1)];
    // where this lane stores.  Stage 2: row 2rp + h of the conv map.  Stage 3: the block starting at row 2rp - h, column gc,
    // in the phase map of the two parities (the row's is that of y0 + h for every row pair)
    uint32_t *dst = nullptr;
    int pitch = ow;
    bool col_ok = in_cols;
    if constexpr (PHASES) {
      const int px = gc & 1, py = (y0 + h) & 1;
      const long long off_even = px ? mq->out_off[1] : mq->out_off[0], off_odd = px ? mq->out_off[3] : mq->out_off[2];
      const long long off = py ? off_odd : off_even;
      pitch = (ow - px) >> 1;
      col_ok = c < TSTEP && xs + c + 1 < ncols && off >= 0;
      dst = reinterpret_cast<uint32_t *>(out + (off >= 0 ? off : 0)) + (size_t)(gc >> 1) * NT + mt;
    } else {
      dst = reinterpret_cast<uint32_t *>(out + mq->out_off[0]) + (size_t)gc * NT + mt;
    }
    uint32_t carry = 0xFFFFFFFFu;  // H of the row above (half 1's of the row pair before)
    for (int rpl = 0; rpl < nrp; rpl++) {
      const uint4 *__restrict__ P = strip + 2 * rpl * WS;
      v16f acc[2] = {seed, seed};  // conv rows 2rp, 2rp + 1
      // step s = 3 kh + kx: input rows 2rp .. 2rp + 3 at column c + kx of channel block 2 kh + h, then the 6 MFMAs of conv
      // rows 2rp, 2rp + 1 x ky
      auto read = [&](v8i &b, int s, int y) {
        const uint4 v = P[(s / 3) * 2 * PIXS + y * WS + s % 3];
        b = v8i{(int)v.x, (int)v.y, (int)v.z, (int)v.w, 0, 0, 0, 0};
      };
      auto mfma = [&](const v8i (&b)[4], int s, int k) {  // k = 2 ky + dy
        acc[k & 1] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(wreg[((k >> 1) * 3 + s % 3) * KH + s / 3], b[(k >> 1) + (k & 1)], acc[k & 1], 4, 4, 0,
                                                                    0x7F7F7F7F, 0, 0x7F7F7F7F);
      };
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
      // W: the !fire word of conv (row 2rp + h, column c).  Each half holds 16 neurons of both rows: one swap hands half 0's
      // row-1 bits to half 1 and half 1's row-0 bits to half 0
      const auto rows = __builtin_amdgcn_permlane32_swap(sign_word(acc[0], h), sign_word(acc[1], h), false, false);
      const uint32_t W = rows[0] | rows[1];
      if constexpr (!PHASES) {
        if (col_ok && 2 * rpl + h < nrows) dst[(size_t)(y0 + 2 * rpl + h) * pitch * NT] = ~W;
      } else {
        const uint32_t H = W & (uint32_t)__builtin_amdgcn_ds_bpermute(((lane + 1) & 63) << 2, (int)W);  // columns c, c + 1
        const auto halves = __builtin_amdgcn_permlane32_swap(H, H, false, false);
        const uint32_t other = h ? halves[0] : halves[1];  // H of the wave's other half: row 2rp + 1 for half 0, row 2rp for half 1
        const uint32_t pooled = (h ? carry : H) & other;
        const bool row_ok = h ? rpl > 0 : 2 * rpl + 1 < nrows;  // both of the block's rows are the band's
        if (col_ok && row_ok) dst[(size_t)((y0 + 2 * rpl - h) >> 1) * pitch * NT] = ~pooled;  // its first row is 2rp - h
        carry = H;
      }
    }
  }
}

}  // namespace

hipError_t launch_clip_conv_phase(int stage, const ClipPhaseLaunch &a) {
  if (stage < 2 || stage > 3 || a.blocks < 1 || a.blocks > INT32_MAX || !a.tab) return hipErrorInvalidValue;
  const dim3 grid((unsigned)a.blocks), block(256);
  const ClipPhaseMap *maps = reinterpret_cast<const ClipPhaseMap *>(a.maps);
  const ClipPhaseBand *bands = reinterpret_cast<const ClipPhaseBand *>(a.bands);
  if (stage == 2) hipLaunchKernelGGL((k_clip_conv_phase<2, 4, false>), grid, block, 0, a.stream, a.in, a.out, a.tab, maps, bands);
  else hipLaunchKernelGGL((k_clip_conv_phase<4, 4, true>), grid, block, 0, a.stream, a.in, a.out, a.tab, maps, bands);
  return hipGetLastError();
}

}  // namespace bnn
