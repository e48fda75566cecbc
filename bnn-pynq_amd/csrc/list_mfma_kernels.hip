// list_mfma_kernels.hip -- layers 1-7 of the single-fault sweeps on the matrix cores (list_mfma_kernels.h; DESIGN.md 9
// "Sweeps on the matrix cores").
//
// The arithmetic, the FP4 encodings, the seeds, the LDS planes, the read-ahead and the epilogues are those of k_conv_mfma,
// k_conv_mfma_a2 and k_tail_mfma (kernels.hip), whose comments derive them, through the device functions of mfma_device.h;
// what is stated here is what differs.
//   * A launch is a LIST of `count` alive slots, ascending: grid min(tiles, resident blocks), tile t the entries
//     [t G, t G + G).  A block loads its wave's neuron tile(s) of the loaded tables into VGPRs once and walks tiles
//     blockIdx.x, + gridDim.x, ...: weights once per block, whatever runs the slots belong to.
//   * The slots of a tile go to LDS (two sets, slots[2][G]): the next tile's between the two barriers of this tile, so that
//     the next tile's source loads, issued behind the second barrier, find them; this tile's epilogue reads its own set.
//     Entries past `count` repeat the last slot; their images are neither expanded nor stored.
//   * Image i of a tile reads in + slots[i] * (an image's input) and writes out + slots[i] * (an image's output): an
//     item's image index, carried or derived as before, goes through the tile's slots instead of being added to a base.
// Outputs are the words the MULTI instantiations of k_quad_x / k_quad / k_vec_x / k_vec leave in those slots.
#include "list_mfma_kernels.h"

#include <type_traits>

#include "kernels.h"
#include "mfma_device.h"

namespace bnn {
namespace {

// the slots of tile t into set `set` (block size >= G)
template <int G>
__device__ __forceinline__ void tile_slots(uint32_t (&slots)[2][G], int set, const uint32_t *__restrict__ list, int count, int t) {
  if ((int)threadIdx.x < G) slots[set][threadIdx.x] = list[min(t * G + (int)threadIdx.x, count - 1)];
}

// ---------------------------------------------------------------------------
// cnvW1A1 layers 1-3 of the listed slots: k_conv_mfma's tile loop, a tile's images wherever their slots lie.
// WIN: input width, CD: input dwords per pixel, NT: neuron tiles, POOL: 2x2 max-pool behind, G: images per tile.
// ---------------------------------------------------------------------------
template <int WIN, int CD, int NT, bool POOL, int G>
__global__ __launch_bounds__(256, 2) void k_list_conv_mfma(const uint32_t *__restrict__ in, uint32_t *__restrict__ out,
                                                            const uint8_t *__restrict__ tab, const uint32_t *__restrict__ list, int count) {
  constexpr int WOUT = WIN - 2, RP = WOUT / 2, IPI = RP * WOUT, KH = CD / 2, KS = 9 * KH, NS = 3 * KH, STREAMS = 4 / NT;
  constexpr int PIX = WIN * WIN, DWI = PIX * CD, NPF = (G * DWI + 255) / 256, DWO = (POOL ? RP * RP : WOUT * WOUT) * NT;
  constexpr int WS = conv_mfma_row_stride(WIN), PIXS = WIN * WS, IMGS = conv_mfma_img_stride(WIN, CD);
  static_assert(WOUT % 2 == 0 && IPI % 2 == 0 && (NT == 2 || NT == 4) && G <= 256, "tile geometry");
  const int ntiles = (count + G - 1) / G;
  if ((int)blockIdx.x >= ntiles) return;  // (the grid is min(tiles, resident): never taken by run_cnv_list_mfma's launches)
  __shared__ uint4 plane[G * IMGS];  // [image][32-channel block q][row][column], strides IMGS, PIXS, WS, 1
  __shared__ uint32_t lut[256];
  __shared__ uint32_t slots[2][G];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), mt = wave % NT, c = lane & 31, h = lane >> 5;
  lut[tid] = fp4_pm1((uint32_t)tid);
  tile_slots<G>(slots, 0, list, count, blockIdx.x);
  // the weights [k step = tap * KH + kh][neuron tile][lane] x 16 bytes, then the seeds [tile][h][16] floats
  const uint4 *__restrict__ wt = reinterpret_cast<const uint4 *>(tab);
  v8i wreg[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ks++) {
    const uint4 v = wt[(ks * NT + mt) * 64 + lane];
    wreg[ks] = v8i{(int)v.x, (int)v.y, (int)v.z, (int)v.w, 0, 0, 0, 0};
  }
  const v16f seed = reinterpret_cast<const v16f *>(tab + (size_t)KS * NT * 64 * 16)[mt * 2 + h];
  uint32_t pre[NPF];
  auto fetch = [&](int t, int set) {  // source dword d of the tile: dword e = d % DWI of the slot of its image i = d / DWI
    const int lim = min(G, count - t * G) * DWI;
    // (i, e) stepped from dword to dword, and from a start the compiler cannot see through: NPF pairs held over the tile loop
    // would cost layer 3 its registers
    int i = 0, e = tid;
    asm volatile("" : "+v"(i), "+v"(e));
    static_assert(DWI >= 256, "a thread's first dword lies in image 0; at most one image wrap per step");
#pragma unroll
    for (int j = 0; j < NPF; j++) {
      pre[j] = 0u;
      if (tid + 256 * j < lim) pre[j] = in[(size_t)slots[set][i] * DWI + e];
      e += 256;
      if (e >= DWI) e -= DWI, i += 1;
    }
  };
  // source dword d of the tile (32 channels of a pixel) -> its 16-byte slot in the planes
  auto slot = [&](int d) {
    const int i = d / DWI, e = d - i * DWI, pix = e / CD, q = e % CD;
    return i * IMGS + q * PIXS + (WS == WIN ? pix : pix / WIN * WS + pix % WIN);
  };
  // item arithmetic carried from step to step, as in k_conv_mfma, and the item's image; PS_LAST keeps ragged lanes' reads inside the planes
  constexpr int STEP = 32 * STREAMS, DR = STEP / WOUT, DX = STEP % WOUT, PS_LAST = (G - 1) * IMGS + 2 * (RP - 1) * WS + WOUT - 1;
  constexpr bool RAGGED = (G * IPI) % 32 != 0;
  static_assert(DX % 2 == 0 && DR + 1 <= RP, "a lane's column keeps its parity; one row-pair wrap and one image wrap per step");
  const int item0 = (wave / NT) * 32 + c, i0 = item0 / IPI, rem0 = item0 - i0 * IPI, rp0 = rem0 / WOUT, x0 = rem0 - rp0 * WOUT;
  const int ps0 = i0 * IMGS + 2 * rp0 * WS + x0;
  __syncthreads();  // the first tile's slots
  fetch(blockIdx.x, 0);
  int set = 0;
  for (int t = blockIdx.x; t < ntiles; t += gridDim.x, set ^= 1) {
    const int nimg = min(G, count - t * G), nitems = nimg * IPI;
    const bool more = t + (int)gridDim.x < ntiles;
    __syncthreads();  // the previous tile's planes and the other set of slots are no longer read
#pragma unroll
    for (int j = 0; j < NPF; j++) {  // one source dword (32 channels of a pixel) per iteration
      const int d = tid + 256 * j;
      if (d < nimg * DWI) {
        const uint32_t bits = pre[j];
        plane[slot(d)] = make_uint4(lut[bits & 255], lut[(bits >> 8) & 255], lut[(bits >> 16) & 255], lut[bits >> 24]);
      }
    }
    if (more) tile_slots<G>(slots, set ^ 1, list, count, t + gridDim.x);
    __syncthreads();
    if (more) fetch(t + gridDim.x, set ^ 1);
    const uint32_t *__restrict__ mine = slots[set];
    int x = x0, rp = rp0, ps = ps0, im = i0;
    for (int t0 = (wave / NT) * 32; t0 < nitems; t0 += STEP) {
      v16f acc[2] = {seed, seed};  // output rows 2rp, 2rp + 1
      const uint4 *__restrict__ P = &plane[(RAGGED ? min(ps, PS_LAST) : ps) + h * PIXS];
      auto read = [&](v8i &b, int s, int y) {  // input row 2rp + y at column x + s % 3 of channel block 2 (s / 3) + h
        const uint4 v = P[(s / 3) * 2 * PIXS + y * WS + s % 3];
        b = v8i{(int)v.x, (int)v.y, (int)v.z, (int)v.w, 0, 0, 0, 0};
      };
      auto mfma = [&](const v8i (&b)[4], int s, int k) {  // k = 2 ky + dy
        acc[k & 1] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(wreg[((k >> 1) * 3 + s % 3) * KH + s / 3], b[(k >> 1) + (k & 1)], acc[k & 1], 4,
                                                                    4, 0, 0x7F7F7F7F, 0, 0x7F7F7F7F);
      };
      // the four reads of step s + 1 behind the first four MFMAs of step s, into the other register set
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
      const bool valid = t0 + c < nitems;  // (then im < nimg)
      if constexpr (POOL) {
        int v[16];  // vertical pool: the sign of the AND is "both rows negative"
#pragma unroll
        for (int k = 0; k < 16; k++) v[k] = __float_as_int(acc[0][k]) & __float_as_int(acc[1][k]);
        const uint32_t nf = or_halves(sign_nibbles(v, h));
        const uint32_t pooled = nf & (uint32_t)__builtin_amdgcn_mov_dpp((int)nf, 0xB1, 0xF, 0xF, true);  // & lane c ^ 1
        if (valid && h == 0 && !(c & 1)) out[(size_t)mine[im] * DWO + (rp * RP + (x >> 1)) * NT + mt] = ~pooled;
      } else {
        uint32_t nf[2];
#pragma unroll
        for (int dy = 0; dy < 2; dy++) {
          int v[16];
#pragma unroll
          for (int k = 0; k < 16; k++) v[k] = __float_as_int(acc[dy][k]);
          nf[dy] = sign_nibbles(v, h);  // this half's 16 neurons of output row 2rp + dy
        }
        const auto sw = __builtin_amdgcn_permlane32_swap(nf[0], nf[1], false, false);  // half h ends with row 2rp + h's word
        if (valid) out[(size_t)mine[im] * DWO + ((2 * rp + h) * WOUT + x) * NT + mt] = ~(sw[0] | sw[1]);
      }
      x += DX, rp += DR, ps += 2 * DR * WS + DX;
      if (x >= WOUT) x -= WOUT, rp += 1, ps += 2 * WS - WOUT;
      if (rp >= RP) rp -= RP, ps += IMGS - 2 * RP * WS, im += 1;
    }
  }
}

// ---------------------------------------------------------------------------
// cnvW1A2 and cnvW2A2 layers 1-3 of the listed slots: k_conv_mfma_a2's tile loop.
// ---------------------------------------------------------------------------
template <int WIN, int CD, int NT, bool POOL, int G>
__global__ __launch_bounds__(256, 2) void k_list_conv_mfma_a2(const uint4 *__restrict__ in, uint32_t *__restrict__ out,
                                                               const uint8_t *__restrict__ tab, const uint32_t *__restrict__ list, int count) {
  constexpr int WOUT = WIN - 2, RP = WOUT / 2, IPI = RP * WOUT, KH = CD / 2, KS = 9 * KH, STREAMS = 4 / NT;
  constexpr int PIX = WIN * WIN, QWI = PIX * KH, NPF = (G * QWI + 255) / 256;  // QWI: source uint4 per image
  static_assert(WOUT % 2 == 0 && IPI % 2 == 0 && (NT == 2 || NT == 4) && G <= 256, "tile geometry");
  const int ntiles = (count + G - 1) / G;
  if ((int)blockIdx.x >= ntiles) return;
  __shared__ uint4 plane[G][CD][PIX];
  __shared__ uint32_t lutz[256], luts[256];
  __shared__ uint32_t slots[2][G];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, mt = wave % NT, c = lane & 31, h = lane >> 5;
  lutz[tid] = nibble_spread((uint32_t)tid) << 1;
  luts[tid] = nibble_spread((uint32_t)tid) << 3;
  tile_slots<G>(slots, 0, list, count, blockIdx.x);
  // the weights, then the seeds and the t1 - t0, each [tile][h][16] floats
  const uint4 *__restrict__ wt = reinterpret_cast<const uint4 *>(tab);
  v8i wreg[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ks++) {
    const uint4 v = wt[(ks * NT + mt) * 64 + lane];
    wreg[ks] = v8i{(int)v.x, (int)v.y, (int)v.z, (int)v.w, 0, 0, 0, 0};
  }
  const v16f *__restrict__ cst = reinterpret_cast<const v16f *>(tab + (size_t)KS * NT * 64 * 16);
  const v16f seed = cst[mt * 2 + h], dt = cst[NT * 2 + mt * 2 + h];
  uint4 pre[NPF];
  auto fetch = [&](int t, int set) {
    const int lim = min(G, count - t * G) * QWI;
#pragma unroll
    for (int j = 0; j < NPF; j++) {
      const int d = tid + 256 * j, i = d / QWI;
      pre[j] = make_uint4(0u, 0u, 0u, 0u);
      if (d < lim) pre[j] = in[(size_t)slots[set][i] * QWI + (d - i * QWI)];
    }
  };
  __syncthreads();  // the first tile's slots
  fetch(blockIdx.x, 0);
  int set = 0;
  for (int t = blockIdx.x; t < ntiles; t += gridDim.x, set ^= 1) {
    const int nimg = min(G, count - t * G), nitems = nimg * IPI;
    const bool more = t + (int)gridDim.x < ntiles;
    __syncthreads();  // the previous tile's planes and the other set of slots are no longer read
#pragma unroll
    for (int j = 0; j < NPF; j++) {  // one source uint4 (64 channels of a pixel: sign lo, hi, non-zero lo, hi) per iteration
      const int d = tid + 256 * j;
      if (d < nimg * QWI) {
        const int i = d / QWI, e = d - i * QWI, pix = e / KH, cw = e % KH;
        const uint4 v = pre[j];
        plane[i][2 * cw][pix] = fp4_planes(lutz, luts, v.x, v.z);
        plane[i][2 * cw + 1][pix] = fp4_planes(lutz, luts, v.y, v.w);
      }
    }
    if (more) tile_slots<G>(slots, set ^ 1, list, count, t + gridDim.x);
    __syncthreads();
    if (more) fetch(t + gridDim.x, set ^ 1);
    for (int t0 = (wave / NT) * 32; t0 < nitems; t0 += 32 * STREAMS) {
      const int item = min(t0 + c, nitems - 1);
      const int i = item / IPI, rem = item - i * IPI, rp = rem / WOUT, x = rem - rp * WOUT;
      v16f acc[2] = {seed, seed};  // output rows 2rp, 2rp + 1
#pragma unroll
      for (int kh = 0; kh < KH; kh++) {
        const uint4 *__restrict__ P = &plane[i][kh * 2 + h][2 * rp * WIN + x];
#pragma unroll
        for (int kx = 0; kx < 3; kx++) {
          v8i b[4];  // input rows 2rp .. 2rp + 3 at column x + kx
#pragma unroll
          for (int y = 0; y < 4; y++) {
            const uint4 v = P[y * WIN + kx];
            b[y] = v8i{(int)v.x, (int)v.y, (int)v.z, (int)v.w, 0, 0, 0, 0};
          }
#pragma unroll
          for (int ky = 0; ky < 3; ky++)
#pragma unroll
            for (int dy = 0; dy < 2; dy++)
              acc[dy] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(wreg[(ky * 3 + kx) * KH + kh], b[ky + dy], acc[dy], 4, 4, 0,
                                                                         0x7F7F7F7F, 0, 0x7F7F7F7F);
        }
      }
      const bool valid = t0 + c < nitems;
      const size_t img = slots[set][i];  // the image's slot: where its output goes (i < nimg)
      if constexpr (POOL) {
        v16f top;
#pragma unroll
        for (int k = 0; k < 16; k++) top[k] = fmaxf(acc[0][k], acc[1][k]);
        uint32_t n0, n1;
        not_fired(top, dt, h, n0, n1);
        n0 &= (uint32_t)__builtin_amdgcn_mov_dpp((int)n0, 0xB1, 0xF, 0xF, true);  // & lane c ^ 1
        n1 &= (uint32_t)__builtin_amdgcn_mov_dpp((int)n1, 0xB1, 0xF, 0xF, true);
        const size_t w64 = (img * (RP * RP) + rp * RP + (x >> 1)) * (NT / 2) + mt / 2;
        if (valid && !(x & 1)) out[(w64 * 2 + h) * 2 + (mt & 1)] = h ? ~(n0 ^ n1) : (n0 & n1);
      } else {
        uint32_t n0[2], n1[2];
#pragma unroll
        for (int dy = 0; dy < 2; dy++) not_fired(acc[dy], dt, h, n0[dy], n1[dy]);
        const uint32_t m0 = h ? n0[1] : n0[0], m1 = h ? n1[1] : n1[0];
        const size_t w64 = (img * (WOUT * WOUT) + (2 * rp + h) * WOUT + x) * (NT / 2) + mt / 2;
        if (valid) {
          out[(w64 * 2 + 0) * 2 + (mt & 1)] = m0 & m1;
          out[(w64 * 2 + 1) * 2 + (mt & 1)] = ~(m0 ^ m1);
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------
// Layers 4-7 of the listed slots: k_tail_mfma's three shapes (CONV: layer 4; dense over 2304 bits: layer 5; layers 6 and
// 7).  KS: k steps, NT: neuron tiles, WAVES: waves per block, G: images per tile.
// ---------------------------------------------------------------------------
template <bool A2, int KS, int NT, bool CONV, int WAVES, int G>
__global__ __launch_bounds__(64 * WAVES, 8 / WAVES) void k_list_tail_mfma(const std::conditional_t<A2, uint4, uint32_t> *__restrict__ in,
                                                                           uint32_t *__restrict__ out, const uint8_t *__restrict__ tab,
                                                                           const uint32_t *__restrict__ list, int count) {
  using U = std::conditional_t<A2, uint4, uint32_t>;  // source unit: 64 channels in two planes, or 32 channels
  constexpr int T = 64 * WAVES, TPW = NT / WAVES, IPI = CONV ? 9 : 1, W64 = CONV ? 25 * 2 : KS, UPI = A2 ? W64 : 2 * W64;
  constexpr int GP = G + 1, NPL = CONV ? G * 4 * 25 : 2 * KS * GP, NPF = (G * UPI + T - 1) / T, NC = (A2 ? 2 : 1) * NT * 2;
  static_assert(NT % WAVES == 0 && (!CONV || KS == 18) && (G * IPI) % 32 == 0 && G <= T, "tile geometry");
  const int ntiles = (count + G - 1) / G;
  if ((int)blockIdx.x >= ntiles) return;
  __shared__ uint4 plane[NPL];
  __shared__ uint32_t lut[A2 ? 512 : 256];  // A2: lutz, then luts (fp4_planes)
  __shared__ v16f cst[NC];                  // the seeds [tile][h], then (A2) t1 - t0 [tile][h]
  __shared__ uint32_t slots[2][G];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, mt0 = wave * TPW, c = lane & 31, h = lane >> 5;
  for (int k = tid; k < 256; k += T) {
    if constexpr (A2) {
      lut[k] = nibble_spread((uint32_t)k) << 1;
      lut[256 + k] = nibble_spread((uint32_t)k) << 3;
    } else {
      lut[k] = fp4_pm1((uint32_t)k);
    }
  }
  for (int k = tid; k < NC * 16; k += T) reinterpret_cast<float *>(cst)[k] = reinterpret_cast<const float *>(tab + (size_t)KS * NT * 64 * 16)[k];
  tile_slots<G>(slots, 0, list, count, blockIdx.x);
  // the weights [k step][neuron tile][lane] x 16 bytes
  const uint4 *__restrict__ wt = reinterpret_cast<const uint4 *>(tab);
  v8i wreg[TPW][KS];
#pragma unroll
  for (int j = 0; j < TPW; j++)
#pragma unroll
    for (int ks = 0; ks < KS; ks++) {
      const uint4 v = wt[(ks * NT + mt0 + j) * 64 + lane];
      wreg[j][ks] = v8i{(int)v.x, (int)v.y, (int)v.z, (int)v.w, 0, 0, 0, 0};
    }
  U pre[NPF];
  auto fetch = [&](int t, int set) {
    const int lim = min(G, count - t * G) * UPI;
#pragma unroll
    for (int j = 0; j < NPF; j++) {
      const int d = tid + T * j, i = d / UPI;
      pre[j] = U{};
      if (d < lim) pre[j] = in[(size_t)slots[set][i] * UPI + (d - i * UPI)];
    }
  };
  __syncthreads();  // the first tile's slots (and lut, cst)
  fetch(blockIdx.x, 0);
  int set = 0;
  for (int t = blockIdx.x; t < ntiles; t += gridDim.x, set ^= 1) {
    const int nimg = min(G, count - t * G), nitems = nimg * IPI;
    const bool more = t + (int)gridDim.x < ntiles;
    __syncthreads();  // the previous tile's planes and the other set of slots are no longer read
#pragma unroll
    for (int j = 0; j < NPF; j++) {
      const int d = tid + T * j;
      if (d < nimg * UPI) {
        const int i = d / UPI, e = d - i * UPI;
        if constexpr (A2) {  // one source uint4: sign lo, hi, non-zero lo, hi of 64 channels
          const uint4 v = pre[j];
          const int p0 = CONV ? (i * 4 + 2 * (e & 1)) * 25 + (e >> 1) : 2 * e * GP + i, step = CONV ? 25 : GP;
          plane[p0] = fp4_planes(lut, lut + 256, v.x, v.z);
          plane[p0 + step] = fp4_planes(lut, lut + 256, v.y, v.w);
        } else {  // one source dword: 32 channels
          const uint32_t bits = pre[j];
          const int p0 = CONV ? (i * 4 + (e & 3)) * 25 + (e >> 2) : e * GP + i;
          plane[p0] = make_uint4(lut[bits & 255], lut[(bits >> 8) & 255], lut[(bits >> 16) & 255], lut[bits >> 24]);
        }
      }
    }
    if (more) tile_slots<G>(slots, set ^ 1, list, count, t + gridDim.x);
    __syncthreads();
    if (more) fetch(t + gridDim.x, set ^ 1);
#pragma clang loop unroll(disable) interleave(disable) vectorize(disable)
    for (int t0 = 0; t0 < nitems; t0 += 32) {
      const int item = min(t0 + c, nitems - 1);
      int base, img = item, p = 0;  // the item's image in the tile and its position in the image
      if constexpr (CONV) {
        img = item / 9, p = item - img * 9;
        const int oy = p / 3, ox = p - oy * 3;
        base = (img * 4 + h) * 25 + oy * 5 + ox;
      } else {
        base = h * GP + item;
      }
      v16f acc[TPW];
#pragma unroll
      for (int j = 0; j < TPW; j++) acc[j] = cst[(mt0 + j) * 2 + h];
#pragma unroll
      for (int ks = 0; ks < KS; ks++) {
        const int off = CONV ? (ks & 1) * 2 * 25 + ((ks >> 1) / 3) * 5 + (ks >> 1) % 3 : ks * 2 * GP;
        const uint4 v = plane[base + off];
        const v8i b = v8i{(int)v.x, (int)v.y, (int)v.z, (int)v.w, 0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < TPW; j++)
          acc[j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(wreg[j][ks], b, acc[j], 4, 4, 0, 0x7F7F7F7F, 0, 0x7F7F7F7F);
      }
      const bool valid = t0 + c < nitems;
      const size_t gitem = (size_t)slots[set][img] * IPI + p;  // counted from slot 0: where the item's output goes (img < nimg)
#pragma unroll
      for (int j = 0; j < TPW; j++) {
        const int mt = mt0 + j;
        if constexpr (A2) {
          uint32_t n0, n1;
          not_fired(acc[j], cst[NT * 2 + mt * 2 + h], h, n0, n1);
          const size_t w64 = gitem * (NT / 2) + mt / 2;  // lane half h stores plane h
          if (valid) out[(w64 * 2 + h) * 2 + (mt & 1)] = h ? ~(n0 ^ n1) : (n0 & n1);
        } else {
          int v[16];
#pragma unroll
          for (int k = 0; k < 16; k++) v[k] = __float_as_int(acc[j][k]);
          const uint32_t nf = or_halves(sign_nibbles(v, h));
          if (valid && h == (j & 1)) out[gitem * NT + mt] = ~nf;
        }
      }
    }
  }
}

// resident blocks of the list kernels: two 4-wave blocks per CU, one 8-wave block (256 CUs)
constexpr long long kListGrid4 = 512, kListGrid8 = 256;
constexpr int kListImgsL1 = 2, kListImgs = 8, kListImgsL4 = 32, kListImgsL5 = 32, kListImgsFc = 128;

inline dim3 list_grid(const ListLaunch &a, int g, long long resident) {
  return dim3((unsigned)std::min<long long>(((long long)a.count + g - 1) / g, resident));
}
#define BNN_LIST(kern, G, resident, T, in, out, off) \
  hipLaunchKernelGGL(kern, list_grid(a, (G), (resident)), dim3(T), 0, a.stream, in, out, a.tables + (off), a.list, a.count)

}  // namespace

hipError_t run_cnv_list_mfma(NetId net, int layer, const ListLaunch &a) {
  const bool cnv = net == NET_CNVW1A1 || net == NET_CNVW1A2 || net == NET_CNVW2A2;
  if (!cnv || !a.tables || !a.list || !a.buf0 || !a.buf1 || layer < 1 || layer > 7 || a.count < 1) return hipErrorInvalidValue;
  // odd layers read buf0 and write buf1, even layers the other way round (stage_output_bytes)
  const void *const src = layer & 1 ? a.buf0 : a.buf1;
  uint32_t *const dst = reinterpret_cast<uint32_t *>(layer & 1 ? a.buf1 : a.buf0);
  if (net == NET_CNVW1A1) {
    const uint32_t *const in = static_cast<const uint32_t *>(src);
    switch (layer) {
      case 1: BNN_LIST((k_list_conv_mfma<30, 2, 2, true, kListImgsL1>), kListImgsL1, kListGrid4, 256, in, dst, 0); break;
      case 2: BNN_LIST((k_list_conv_mfma<14, 2, 4, false, kListImgs>), kListImgs, kListGrid4, 256, in, dst, kConvMfmaL2Off); break;
      case 3: BNN_LIST((k_list_conv_mfma<12, 4, 4, true, kListImgs>), kListImgs, kListGrid4, 256, in, dst, kConvMfmaL3Off); break;
      case 4: BNN_LIST((k_list_tail_mfma<false, 18, 8, true, 8, kListImgsL4>), kListImgsL4, kListGrid8, 512, in, dst, kTailMfmaL4Off); break;
      case 5: BNN_LIST((k_list_tail_mfma<false, 36, 8, false, 8, kListImgsL5>), kListImgsL5, kListGrid8, 512, in, dst, kTailMfmaL5Off); break;
      case 6: BNN_LIST((k_list_tail_mfma<false, 4, 16, false, 4, kListImgsFc>), kListImgsFc, kListGrid4, 256, in, dst, kTailMfmaL6Off); break;
      default: BNN_LIST((k_list_tail_mfma<false, 8, 16, false, 8, kListImgsFc>), kListImgsFc, kListGrid8, 512, in, dst, kTailMfmaL7Off); break;
    }
  } else {
    const uint4 *const in = static_cast<const uint4 *>(src);
    switch (layer) {
      case 1: BNN_LIST((k_list_conv_mfma_a2<30, 2, 2, true, kListImgsL1>), kListImgsL1, kListGrid4, 256, in, dst, 0); break;
      case 2: BNN_LIST((k_list_conv_mfma_a2<14, 2, 4, false, kListImgs>), kListImgs, kListGrid4, 256, in, dst, kConvMfmaA2L2Off); break;
      case 3: BNN_LIST((k_list_conv_mfma_a2<12, 4, 4, true, kListImgs>), kListImgs, kListGrid4, 256, in, dst, kConvMfmaA2L3Off); break;
      case 4: BNN_LIST((k_list_tail_mfma<true, 18, 8, true, 8, kListImgsL4>), kListImgsL4, kListGrid8, 512, in, dst, kTailMfmaA2L4Off); break;
      case 5: BNN_LIST((k_list_tail_mfma<true, 36, 8, false, 8, kListImgsL5>), kListImgsL5, kListGrid8, 512, in, dst, kTailMfmaA2L5Off); break;
      case 6: BNN_LIST((k_list_tail_mfma<true, 4, 16, false, 4, kListImgsFc>), kListImgsFc, kListGrid4, 256, in, dst, kTailMfmaA2L6Off); break;
      default: BNN_LIST((k_list_tail_mfma<true, 8, 16, false, 8, kListImgsFc>), kListImgsFc, kListGrid8, 512, in, dst, kTailMfmaA2L7Off); break;
    }
  }
  return hipPeekAtLastError();  // (left pending, as run_cnv_multi_mfma's: the sweep reports it with its stage)
}

}  // namespace bnn
