// scan_l0_mfma_kernels.hip -- stage 0 of the clip scan on the matrix cores (scan_l0_mfma_kernels.h; DESIGN.md 9 "Clip scan").
//
// The arithmetic is k_conv0_tile's (kernels.hip): quantised int8 pixels against the {-1, 0, +1} weights of layer 0, nine
// 3-tap runs (c, ky) of a window as nine dwords of the K = 32 + 16 operand of v_mfma_i32_32x32x32_i8 + v_mfma_i32_32x32x16_i8,
// the threshold folded into the product by the constants 1 and 64, sign bit = !fire; the A operands are the table every
// load_parameters makes for that kernel (packed_params.h).  What differs is the picture: a map here belongs to a planar level
// of any width, whose rows and planes start at any byte address, and a launch holds many maps of different sizes.
//   * A BLOCK (256 threads, four waves) owns a band of one map: up to kClipL0Rows (16) output rows x up to kClipL0Cols (128)
//     output columns.  It finds its band (map, first row, first column) and the map's descriptor in the tables of
//     scan_clip.h (ClipMfmaBand, ClipL0Map) through scalar loads.
//   * The band's input patch, 3 planes x (rows + 2) rows x (columns + 2) bytes, is read ONCE from HBM and quantised ONCE.  A
//     wave stages one (plane, row) per pass and a lane four bytes of it: the two aligned dwords around them and a
//     v_alignbyte by the row's phase, which is wave-uniform.  Column 0 of the patch is then dword-aligned in LDS whatever the
//     source's alignment.  The passes are unrolled, all loads of a wave in flight together; passes past the patch's last
//     row repeat that row (the same bytes to the same place).  The last dword of a row can reach up to 7 bytes past the row's
//     own bytes: ClipL0Tables::planes_top states how far, and the caller reserves it.
//   * LDS rows are kClipL0Pitch (160) bytes apart and planes 18 rows (2 880): the header says why these keep the two lane
//     halves on different banks.
//   * A TILE is 32 consecutive output pixels of one output row; the band's tiles (row, 32 columns), columns inner, go round
//     the four waves.  The tile loop is k_conv0_tile's: lane (r, h) fetches its five runs as aligned dword pairs +
//     v_alignbyte, the next tile's fetches are issued behind this tile's first MFMAs, one v_permlane32_swap leaves lane
//     (r, h) with dword h of pixel r.  Lanes past the band's right edge compute on what the patch holds there and store nothing.
// No scratch, no spills; outputs are k_clip_conv0's words at the same offsets.  Only the 1-bit form (cnvW1A1) is built.
#include "scan_l0_mfma_kernels.h"

#include "packed_params.h"

namespace bnn {
namespace {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));
typedef const ClipL0Map __attribute__((address_space(4))) *kptr_lmap;
typedef const ClipMfmaBand __attribute__((address_space(4))) *kptr_band;

// ---- the helpers of kernels.hip this kernel is written with (copies: that file's are in its anonymous namespace) ----
// uint8 p -> int8 q = p - 128 + (p >= 128) - (p == 255), four bytes at a time
__device__ __forceinline__ uint32_t quantise4(uint32_t p) {
  const uint32_t t = p ^ 0x80808080u;
  const uint32_t s = (t & 0x7F7F7F7Fu) + 0x01010101u;
  const uint32_t inc = p & ~s & 0x80808080u;
  return t + (inc >> 7);
}
// bits = (bits << 1) | (v < 0)
__device__ __forceinline__ uint32_t shift_in_sign(uint32_t bits, int v) {
  asm("" : "+v"(v));
  return __builtin_amdgcn_alignbit(bits, (uint32_t)v, 31);
}
// sign bits of 16 accumulators -> bits 0..15 (register i -> bit i)
__device__ __forceinline__ uint32_t sign_bits16(const v16i &acc) {
  uint32_t x = 0;
#pragma unroll
  for (int i = 15; i >= 0; i--) x = shift_in_sign(x, acc[i]);
  return x;
}
// 16-bit words: lanes 0..31 contribute `a`, lanes 32..63 `b`; lane (r, h): (a of lane r | a of lane r + 32 << 16) for
// h = 0, the same of b for h = 1
__device__ __forceinline__ uint32_t merge_halves16(uint32_t a, uint32_t b) {
  const auto sw = __builtin_amdgcn_permlane32_swap(a, b, false, false);
  return sw[0] | (sw[1] << 16);
}

constexpr int kPitch = kClipL0Pitch, kPlane = kClipL0Plane, kPatchRows = kClipL0Rows + 2;
constexpr int kWaves = 4, kPasses = (3 * kPatchRows + kWaves - 1) / kWaves;  // 54 (plane, row) pairs: 14 passes
static_assert(kClipL0Cols % 32 == 0 && kClipL0Cols / 4 + 1 <= 64, "a wave stages a patch row in one pass; whole tiles in a full band");

__global__ __launch_bounds__(256, 2) void k_clip_conv0_mfma(const uint8_t *__restrict__ planes, uint8_t *__restrict__ out, const uint8_t *__restrict__ tab,
                                                             const ClipL0Map *__restrict__ maps, const ClipMfmaBand *__restrict__ bands) {
  __shared__ uint32_t patch[kClipL0LdsBytes / 4];  // quantised: [plane][row][byte], strides kPlane, kPitch, 1
  const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // the block's band and its map (wave-uniform: scalar loads)
  const kptr_band bq = (kptr_band)(uintptr_t)bands + blockIdx.x;
  const int y0 = bq->rp0, x0 = bq->x0;
  const kptr_lmap mq = (kptr_lmap)(uintptr_t)maps + bq->map;
  const long long in_off = mq->in_off, out_off = mq->out_off, plane_stride = mq->plane_stride;
  const int row_stride = mq->row_stride, ow = mq->ow, oh = mq->oh;
  const int cols = min(kClipL0Cols, ow - x0), nrows = min(kClipL0Rows, oh - y0);
  // the patch: level rows y0 .. y0 + nrows + 1, columns x0 .. x0 + cols + 1 of the three planes, all inside the level
  // (ow + 2 <= its width, oh + 2 <= its height).  Lane d < nd of a pass takes patch bytes 4d .. 4d + 3 of the pass's row.
  {
    const uint8_t *__restrict__ src = planes + in_off + (size_t)y0 * row_stride + x0;
    const int prows = nrows + 2, nd = (cols + 2 + 3) >> 2;
    if (lane < nd) {
      uint32_t lo[kPasses], hi[kPasses];
#pragma unroll
      for (int i = 0; i < kPasses; i++) {
        const int pr = min(wave + kWaves * i, 3 * kPatchRows - 1), plane = pr / kPatchRows, row = min(pr - plane * kPatchRows, prows - 1);
        const uint8_t *p = src + (size_t)plane * plane_stride + (size_t)row * row_stride;
        const uint32_t *__restrict__ q = reinterpret_cast<const uint32_t *>(p - ((uintptr_t)p & 3));
        lo[i] = q[lane];
        hi[i] = q[lane + 1];
      }
#pragma unroll
      for (int i = 0; i < kPasses; i++) {
        const int pr = min(wave + kWaves * i, 3 * kPatchRows - 1), plane = pr / kPatchRows, row = min(pr - plane * kPatchRows, prows - 1);
        const uint32_t phase = (uint32_t)((uintptr_t)(src + (size_t)plane * plane_stride + (size_t)row * row_stride) & 3);
        patch[(plane * kPlane + row * kPitch) / 4 + lane] = quantise4(__builtin_amdgcn_alignbyte(hi[i], lo[i], phase));
      }
    }
  }
  // A operands (loop-invariant): 16 + 8 bytes per lane and neuron tile
  v4i abig[2];
  long asm0[2];
#pragma unroll
  for (int ct = 0; ct < 2; ct++) {
    abig[ct] = *reinterpret_cast<const v4i *>(tab + ((ct * 32 + r) * 2 + h) * 16);
    asm0[ct] = *reinterpret_cast<const long *>(tab + kL0MfmaBigBytes + (((0 * 2 + ct) * 32 + r) * 2 + h) * 8);
  }
  __syncthreads();
  const uint8_t *qb = reinterpret_cast<const uint8_t *>(patch);
  const v16i zero = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  // this lane's runs: h = 0: (c,ky) = (0,0) (0,1) (0,2) (2,0) and, for the K = 16 product, (2,1);
  //                   h = 1: (1,0) (1,1) (1,2) (2,2) and the constants 1, 64
  // Their LDS addresses are two lane constants plus the tile's term oy * kPitch + 32 tx, a multiple of 4: the `& ~3` applies
  // to the lane part alone and the shift is r & 3 in every tile.
  const uint32_t lane_byte = (uint32_t)(r + h * kPlane);
  const uint32_t al_lane = lane_byte & ~3u;
  uint32_t al2_lane = al_lane + 2 * kPlane - h * (kPlane - 2 * kPitch);  // run (2,0) / (2,2): two rows apart
  uint32_t lane_out = (uint32_t)(r * 2 + h) * 4;                         // bytes into the tile's 32 output pixels
  asm("" : "+v"(al2_lane), "+v"(lane_out));
  uint32_t lo[5], hi[5];  // the two aligned dwords around each run
  const auto fetch = [&](int oy, int tx) {
    const uint32_t tile = (uint32_t)(oy * kPitch + 32 * tx);
    const uint32_t *al = reinterpret_cast<const uint32_t *>(qb + (al_lane + tile));
    const uint32_t *al2 = reinterpret_cast<const uint32_t *>(qb + (al2_lane + tile));
#pragma unroll
    for (int i = 0; i < 3; i++) lo[i] = al[(kPitch / 4) * i], hi[i] = al[(kPitch / 4) * i + 1];
#pragma unroll
    for (int i = 0; i < 2; i++) lo[3 + i] = al2[(kPitch / 4) * i], hi[3 + i] = al2[(kPitch / 4) * i + 1];
  };
  // tile T of the band is (row T / ntx, columns 32 (T % ntx) ..): a wave keeps (oy, tx) and steps them four tiles on
  const int ntx = (cols + 31) >> 5, ntiles = nrows * ntx;
  int oy = 0, tx = wave;
  while (tx >= ntx) tx -= ntx, oy++;
  uint8_t *__restrict__ o = out + out_off;
  uint32_t bs_lo = 0x00004001u;  // lane half 1 keeps this through the loop
  fetch(min(oy, nrows - 1), tx);
  for (int T = wave; T < ntiles; T += kWaves) {
    uint8_t *orow = o + ((size_t)(y0 + oy) * ow + (size_t)(x0 + 32 * tx)) * 8;
    const bool live = r < cols - 32 * tx;
    v4i bb;
#pragma unroll
    for (int i = 0; i < 4; i++) bb[i] = (int)__builtin_amdgcn_alignbyte(hi[i], lo[i], lane_byte);
    {  // run (2,1) where h = 0; lanes 32..63 are masked off and keep their constant
      uint64_t saved;
      asm volatile("s_mov_b64 %1, exec\n\ts_mov_b64 exec, 0xffffffff\n\tv_alignbyte_b32 %0, %2, %3, %4\n\ts_mov_b64 exec, %1"
                   : "+v"(bs_lo), "=&s"(saved)
                   : "v"(hi[4]), "v"(lo[4]), "v"(lane_byte));
    }
    const long bs = (long)(uint64_t)bs_lo;
    // both neuron tiles' products are issued before either is read: the second chain covers the first one's latency
    v16i big[2], d0[2];
#pragma unroll
    for (int ct = 0; ct < 2; ct++) big[ct] = __builtin_amdgcn_mfma_i32_32x32x32_i8(abig[ct], bb, zero, 0, 0, 0);
#pragma unroll
    for (int ct = 0; ct < 2; ct++) d0[ct] = __builtin_amdgcn_mfma_i32_32x32x16_i8(asm0[ct], bs, big[ct], 0, 0, 0);  // dot - t0 - 1: sign = !fire
    // the next tile's fetches (behind the wave's last tile: a staged row of the band again, unused)
    tx += kWaves;
    while (tx >= ntx) tx -= ntx, oy++;
    fetch(min(oy, nrows - 1), tx);
    const uint32_t w = ~merge_halves16(sign_bits16(d0[0]), sign_bits16(d0[1]));  // collected !fire
    if (live) *reinterpret_cast<uint32_t *>(orow + lane_out) = w;
  }
}

}  // namespace

hipError_t launch_clip_conv0_mfma(const ClipL0Launch &a) {
  if (a.blocks < 1 || a.blocks > INT32_MAX || !a.tab || ((uintptr_t)a.planes & 3)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_clip_conv0_mfma, dim3((unsigned)a.blocks), dim3(256), 0, a.stream, a.planes, a.out, a.tab + kL0MfmaTileOffset,
                     reinterpret_cast<const ClipL0Map *>(a.maps), reinterpret_cast<const ClipMfmaBand *>(a.bands));
  return hipGetLastError();
}

}  // namespace bnn
