// multi_mfma_kernels.hip -- layers 1-7 of the campaign launches on the matrix cores (multi_mfma_kernels.h; DESIGN.md 9
// "Campaigns on the matrix cores").
//
// The arithmetic, the FP4 encodings, the seeds, the LDS planes, the read-ahead and the epilogues are those of k_conv_mfma,
// k_conv_mfma_a2 and k_tail_mfma (kernels.hip), whose comments derive them; what is stated here is what differs.
//   * A launch is a set of SEGMENT RECORDS (kernels.h, MultiSeg): grid (bx, nsegs).  Block (x, y) reads record y through
//     scalar loads: run, slot and len are block-uniform, so the table pointer tab + run * tab_stride and the activation
//     pointers in + slot * (image's input) / out + slot * (image's output) stay in SGPRs.
//   * The record is then a batch of its own of `len` images: the block loads its wave's neuron tile(s) of ITS RUN's tables
//     into VGPRs once and walks the record's groups x, x + bx, ...  A block whose x has no group in the record returns
//     before it writes LDS or reaches a barrier (x and the record are block-uniform: all of a block's waves leave together).
//   * The tables are per run: k_seg_table / k_seg_table_a2 make all runs' tables of a layer in one launch, blockIdx.y the
//     run, from the run's own copy of the packed rows.
// Outputs are the words the MULTI instantiations of k_quad_x / k_quad / k_vec_x / k_vec leave in the record's slots.
#include "multi_mfma_kernels.h"

#include <type_traits>

#include "mfma_device.h"

namespace bnn {
namespace {

// the block's record: four dwords, scalar loads
__device__ __forceinline__ MultiSeg seg_record(const MultiSeg *segs) {
  kptr32 p = (kptr32)(uintptr_t)(segs + blockIdx.y);
  return MultiSeg{(int)p[0], (int)p[1], (int)p[2], (int)p[3]};
}

// ---------------------------------------------------------------------------
// The tables of all runs of one layer: k_conv_mfma_table's entries, blockIdx.y the run.  One thread per 16-byte weight entry
// [k step][neuron tile][lane], then one per seed [tile][h][16].  stride_dw: dwords between two runs' copies of the rows.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_seg_table(const uint32_t *__restrict__ rows, size_t stride_dw, int row_dw, int ksteps, int tiles, int mw,
                                                    uint8_t *__restrict__ dst, size_t tab_stride) {
  rows += (size_t)blockIdx.y * stride_dw;
  dst += (size_t)blockIdx.y * tab_stride;
  const int idx = blockIdx.x * 256 + threadIdx.x, nw = ksteps * tiles * 64;
  if (idx < nw) {
    const int ks = idx / (tiles * 64), mt = (idx / 64) % tiles, lane = idx & 63, n = 32 * mt + (lane & 31), h = lane >> 5;
    const uint32_t bits = rows[(size_t)n * row_dw + 2 + 2 * ks + h];  // channels 32h .. 32h + 31 of k step ks
    reinterpret_cast<uint4 *>(dst)[idx] = make_uint4(fp4_pm1(bits & 255), fp4_pm1((bits >> 8) & 255), fp4_pm1((bits >> 16) & 255),
                                                     fp4_pm1(bits >> 24));
  } else if (idx < nw + tiles * 32) {
    const int j = idx - nw, mt = j >> 5, h = (j >> 4) & 1, reg = j & 15;
    const int n = 32 * mt + (reg & 3) + 8 * (reg >> 2) + 4 * h;
    // fire <=> dot > mw - 2t =: theta; the clamp keeps never / always firing rows exact in f32 (a faulted threshold is any 32-bit value)
    long long t = (int)rows[(size_t)n * row_dw];
    t = t < -1 ? -1 : (t > mw + 2 ? mw + 2 : t);
    reinterpret_cast<float *>(dst + (size_t)nw * 16)[j] = (float)(-(mw - 2 * t) - 1);
  }
}

// k_conv_mfma_a2_table's entries, blockIdx.y the run: weights, then the seeds -(t0 + 1/2) and the t1 - t0, each [tile][h][16].
// TT: AR_TT rows {t0, t1, ksteps x {sign u64, non-zero u64}, ksteps x "weight is -2" u64, flag, pad}: a -2 is taken from its
// own plane, never from the flag dword, so a flip that creates or removes one needs nothing else; else AR_TB rows.
template <bool TT>
__global__ __launch_bounds__(256) void k_seg_table_a2(const uint32_t *__restrict__ rows, size_t stride_dw, int ksteps, int tiles,
                                                       uint8_t *__restrict__ dst, size_t tab_stride) {
  rows += (size_t)blockIdx.y * stride_dw;
  dst += (size_t)blockIdx.y * tab_stride;
  const int idx = blockIdx.x * 256 + threadIdx.x, nw = ksteps * tiles * 64, row_dw = TT ? 4 + 6 * ksteps : 2 + 2 * ksteps;
  if (idx < nw) {
    const int ks = idx / (tiles * 64), mt = (idx / 64) % tiles, lane = idx & 63, n = 32 * mt + (lane & 31), h = lane >> 5;
    const uint32_t *__restrict__ row = rows + (size_t)n * row_dw;
    uint32_t b1, b2 = 0, b3;  // channels 32h .. 32h + 31 of k step ks: bits 1, 2, 3 of their nibbles
    if constexpr (TT) {
      const uint32_t sg = row[2 + 4 * ks + h], two = row[2 + 4 * ksteps + 2 * ks + h], nz = row[2 + 4 * ks + 2 + h] | two;
      b1 = nz & ~two;         // +-1: 0x2 / 0xA
      b2 = two;               // -2: 0xC
      b3 = (sg & nz) | two;
    } else {
      b1 = 0xFFFFFFFFu;
      b3 = row[2 + 2 * ks + h];
    }
    uint32_t v[4];
#pragma unroll
    for (int k = 0; k < 4; k++)
      v[k] = (nibble_spread(b1 >> (8 * k)) << 1) | (nibble_spread(b2 >> (8 * k)) << 2) | (nibble_spread(b3 >> (8 * k)) << 3);
    reinterpret_cast<uint4 *>(dst)[idx] = make_uint4(v[0], v[1], v[2], v[3]);
  } else if (idx < nw + tiles * 64) {
    const int j = idx - nw, second = j >= tiles * 32, jj = second ? j - tiles * 32 : j, mt = jj >> 5, h = (jj >> 4) & 1, reg = jj & 15;
    const int n = 32 * mt + (reg & 3) + 8 * (reg >> 2) + 4 * h;
    // fire_i <=> t_i < d and |d| <= 2 * MW: a threshold outside [-2 MW - 1, 2 MW] decides like the nearer end of it
    const int lim = 2 * 64 * ksteps;
    int t0 = (int)rows[(size_t)n * row_dw], t1 = (int)rows[(size_t)n * row_dw + 1];
    t0 = t0 < -lim - 1 ? -lim - 1 : (t0 > lim ? lim : t0);
    t1 = t1 < -lim - 1 ? -lim - 1 : (t1 > lim ? lim : t1);
    reinterpret_cast<float *>(dst + (size_t)nw * 16)[j] = second ? (float)(t1 - t0) : -(float)t0 - 0.5f;
  }
}

// ---------------------------------------------------------------------------
// cnvW1A1 layers 1-3 of a record: k_conv_mfma's tile loop on the record's images.
// WIN: input width, CD: input dwords per pixel, NT: neuron tiles, POOL: 2x2 max-pool behind, G: images per group.
// ---------------------------------------------------------------------------
template <int WIN, int CD, int NT, bool POOL, int G>
__global__ __launch_bounds__(256, 2) void k_seg_conv_mfma(const uint32_t *__restrict__ in, uint32_t *__restrict__ out,
                                                           const uint8_t *__restrict__ tab, size_t tab_stride, const MultiSeg *__restrict__ segs) {
  constexpr int WOUT = WIN - 2, RP = WOUT / 2, IPI = RP * WOUT, KH = CD / 2, KS = 9 * KH, NS = 3 * KH, STREAMS = 4 / NT;
  constexpr int PIX = WIN * WIN, DWI = PIX * CD, NPF = (G * DWI + 255) / 256, DWO = (POOL ? RP * RP : WOUT * WOUT) * NT;
  constexpr int WS = conv_mfma_row_stride(WIN), PIXS = WIN * WS, IMGS = conv_mfma_img_stride(WIN, CD);
  static_assert(WOUT % 2 == 0 && IPI % 2 == 0 && (NT == 2 || NT == 4), "tile geometry");
  // the record: a batch of its own.  No group for this block: gone before LDS is touched
  const MultiSeg sg = seg_record(segs);
  const int n_images = sg.len, ngroups = (n_images + G - 1) / G;
  if ((int)blockIdx.x >= ngroups) return;
  tab += (size_t)sg.run * tab_stride;
  in += (size_t)sg.slot * DWI;
  out += (size_t)sg.slot * DWO;
  __shared__ uint4 plane[G * IMGS];  // [image][32-channel block q][row][column], strides IMGS, PIXS, WS, 1
  __shared__ uint32_t lut[256];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), mt = wave % NT, c = lane & 31, h = lane >> 5;
  lut[tid] = fp4_pm1((uint32_t)tid);
  // the run's weights [k step = tap * KH + kh][neuron tile][lane] x 16 bytes, then the seeds [tile][h][16] floats
  const uint4 *__restrict__ wt = reinterpret_cast<const uint4 *>(tab);
  v8i wreg[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ks++) {
    const uint4 v = wt[(ks * NT + mt) * 64 + lane];
    wreg[ks] = v8i{(int)v.x, (int)v.y, (int)v.z, (int)v.w, 0, 0, 0, 0};
  }
  const v16f seed = reinterpret_cast<const v16f *>(tab + (size_t)KS * NT * 64 * 16)[mt * 2 + h];
  uint32_t pre[NPF];
  auto fetch = [&](int grp) {
    const int img0 = grp * G, lim = min(G, n_images - img0) * DWI;
#pragma unroll
    for (int j = 0; j < NPF; j++) {
      const int d = tid + 256 * j;
      pre[j] = d < lim ? in[(size_t)img0 * DWI + d] : 0u;
    }
  };
  // source dword d of the group (32 channels of a pixel) -> its 16-byte slot in the planes
  auto slot = [&](int d) {
    const int i = d / DWI, e = d - i * DWI, pix = e / CD, q = e % CD;
    return i * IMGS + q * PIXS + (WS == WIN ? pix : pix / WIN * WS + pix % WIN);
  };
  // item arithmetic carried from tile to tile, as in k_conv_mfma; PS_LAST keeps ragged lanes' reads inside the planes
  constexpr int STEP = 32 * STREAMS, DR = STEP / WOUT, DX = STEP % WOUT, PS_LAST = (G - 1) * IMGS + 2 * (RP - 1) * WS + WOUT - 1;
  constexpr bool RAGGED = (G * IPI) % 32 != 0;
  static_assert(DX % 2 == 0 && DR + 1 <= RP, "a lane's column keeps its parity; one row-pair wrap and one image wrap per step");
  const int item0 = (wave / NT) * 32 + c, i0 = item0 / IPI, rem0 = item0 - i0 * IPI, rp0 = rem0 / WOUT, x0 = rem0 - rp0 * WOUT;
  const int ps0 = i0 * IMGS + 2 * rp0 * WS + x0;
  const uint32_t ob0 = (uint32_t)((i0 * (WOUT * WOUT) + (2 * rp0 + h) * WOUT + x0) * NT + mt) * 4;
  fetch(blockIdx.x);
  for (int grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
    const int img0 = grp * G, nimg = min(G, n_images - img0), nitems = nimg * IPI;
    uint32_t *__restrict__ gout = out + (size_t)img0 * DWO;  // the group's outputs: wave-uniform
    __syncthreads();  // the previous group's planes are no longer read
#pragma unroll
    for (int j = 0; j < NPF; j++) {  // one source dword (32 channels of a pixel) per iteration
      const int d = tid + 256 * j;
      if (d < nimg * DWI) {
        const uint32_t bits = pre[j];
        plane[slot(d)] = make_uint4(lut[bits & 255], lut[(bits >> 8) & 255], lut[(bits >> 16) & 255], lut[bits >> 24]);
      }
    }
    if (grp + (int)gridDim.x < ngroups) fetch(grp + gridDim.x);
    __syncthreads();
    int x = x0, rp = rp0, ps = ps0;
    [[maybe_unused]] uint32_t ob = ob0;
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
      const bool valid = t0 + c < nitems;
      if constexpr (POOL) {
        int v[16];  // vertical pool: the sign of the AND is "both rows negative"
#pragma unroll
        for (int k = 0; k < 16; k++) v[k] = __float_as_int(acc[0][k]) & __float_as_int(acc[1][k]);
        const uint32_t nf = or_halves(sign_nibbles(v, h));
        const uint32_t pooled = nf & (uint32_t)__builtin_amdgcn_mov_dpp((int)nf, 0xB1, 0xF, 0xF, true);  // & lane c ^ 1
        if (valid && h == 0 && !(c & 1)) gout[(size_t)(t0 >> 1) * NT + (c >> 1) * NT + mt] = ~pooled;
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
        if (valid) *reinterpret_cast<uint32_t *>(reinterpret_cast<char *>(gout) + ob) = ~(sw[0] | sw[1]);
      }
      x += DX, rp += DR, ps += 2 * DR * WS + DX;
      if constexpr (!POOL) ob += (2 * DR * WOUT + DX) * NT * 4;
      if (x >= WOUT) {
        x -= WOUT, rp += 1, ps += 2 * WS - WOUT;
        if constexpr (!POOL) ob += WOUT * NT * 4;
      }
      if (rp >= RP) rp -= RP, ps += IMGS - 2 * RP * WS;
    }
  }
}

// ---------------------------------------------------------------------------
// cnvW1A2 and cnvW2A2 layers 1-3 of a record: k_conv_mfma_a2's tile loop on the record's images.
// ---------------------------------------------------------------------------
template <int WIN, int CD, int NT, bool POOL, int G>
__global__ __launch_bounds__(256, 2) void k_seg_conv_mfma_a2(const uint4 *__restrict__ in, uint32_t *__restrict__ out,
                                                              const uint8_t *__restrict__ tab, size_t tab_stride, const MultiSeg *__restrict__ segs) {
  constexpr int WOUT = WIN - 2, RP = WOUT / 2, IPI = RP * WOUT, KH = CD / 2, KS = 9 * KH, STREAMS = 4 / NT;
  constexpr int PIX = WIN * WIN, QWI = PIX * KH, NPF = (G * QWI + 255) / 256;  // QWI: source uint4 per image
  static_assert(WOUT % 2 == 0 && IPI % 2 == 0 && (NT == 2 || NT == 4), "tile geometry");
  const MultiSeg sg = seg_record(segs);
  const int n_images = sg.len, ngroups = (n_images + G - 1) / G;
  if ((int)blockIdx.x >= ngroups) return;
  tab += (size_t)sg.run * tab_stride;
  in += (size_t)sg.slot * QWI;
  __shared__ uint4 plane[G][CD][PIX];
  __shared__ uint32_t lutz[256], luts[256];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, mt = wave % NT, c = lane & 31, h = lane >> 5;
  lutz[tid] = nibble_spread((uint32_t)tid) << 1;
  luts[tid] = nibble_spread((uint32_t)tid) << 3;
  // the run's weights, then the seeds and the t1 - t0, each [tile][h][16] floats
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
  auto fetch = [&](int grp) {
    const int img0 = grp * G, lim = min(G, n_images - img0) * QWI;
#pragma unroll
    for (int j = 0; j < NPF; j++) {
      const int d = tid + 256 * j;
      pre[j] = d < lim ? in[(size_t)img0 * QWI + d] : make_uint4(0u, 0u, 0u, 0u);
    }
  };
  fetch(blockIdx.x);
  for (int grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
    const int img0 = grp * G, nimg = min(G, n_images - img0), nitems = nimg * IPI;
    __syncthreads();  // the previous group's planes are no longer read
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
    if (grp + (int)gridDim.x < ngroups) fetch(grp + gridDim.x);
    __syncthreads();
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
      const size_t img = (size_t)(sg.slot + img0 + i);  // the image's slot: where its output goes
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
// Layers 4-7 of a record: k_tail_mfma's three shapes (CONV: layer 4; dense over 2304 bits: layer 5; layers 6 and 7) on the
// record's images.  KS: k steps, NT: neuron tiles, WAVES: waves per block, G: images per group.
// ---------------------------------------------------------------------------
template <bool A2, int KS, int NT, bool CONV, int WAVES, int G>
__global__ __launch_bounds__(64 * WAVES, 8 / WAVES) void k_seg_tail_mfma(const std::conditional_t<A2, uint4, uint32_t> *__restrict__ in,
                                                                          uint32_t *__restrict__ out, const uint8_t *__restrict__ tab,
                                                                          size_t tab_stride, const MultiSeg *__restrict__ segs) {
  using U = std::conditional_t<A2, uint4, uint32_t>;  // source unit: 64 channels in two planes, or 32 channels
  constexpr int T = 64 * WAVES, TPW = NT / WAVES, IPI = CONV ? 9 : 1, W64 = CONV ? 25 * 2 : KS, UPI = A2 ? W64 : 2 * W64;
  constexpr int GP = G + 1, NPL = CONV ? G * 4 * 25 : 2 * KS * GP, NPF = (G * UPI + T - 1) / T, NC = (A2 ? 2 : 1) * NT * 2;
  static_assert(NT % WAVES == 0 && (!CONV || KS == 18) && (G * IPI) % 32 == 0, "tile geometry");
  const MultiSeg sg = seg_record(segs);
  const int n_images = sg.len, ngroups = (n_images + G - 1) / G;
  if ((int)blockIdx.x >= ngroups) return;
  tab += (size_t)sg.run * tab_stride;
  in += (size_t)sg.slot * UPI;
  __shared__ uint4 plane[NPL];
  __shared__ uint32_t lut[A2 ? 512 : 256];  // A2: lutz, then luts (fp4_planes)
  __shared__ v16f cst[NC];                  // the run's seeds [tile][h], then (A2) t1 - t0 [tile][h]
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
  // the run's weights [k step][neuron tile][lane] x 16 bytes
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
  auto fetch = [&](int grp) {
    const int img0 = grp * G, lim = min(G, n_images - img0) * UPI;
#pragma unroll
    for (int j = 0; j < NPF; j++) {
      const int d = tid + T * j;
      pre[j] = d < lim ? in[(size_t)img0 * UPI + d] : U{};
    }
  };
  fetch(blockIdx.x);
  for (int grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
    const int img0 = grp * G, nimg = min(G, n_images - img0), nitems = nimg * IPI;
    __syncthreads();  // the previous group's planes are no longer read (first pass: lut and cst are written)
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
    if (grp + (int)gridDim.x < ngroups) fetch(grp + gridDim.x);
    __syncthreads();
#pragma clang loop unroll(disable) interleave(disable) vectorize(disable)
    for (int t0 = 0; t0 < nitems; t0 += 32) {
      const int item = min(t0 + c, nitems - 1);
      int base;
      if constexpr (CONV) {
        const int i = item / 9, p = item - i * 9, oy = p / 3, ox = p - oy * 3;
        base = (i * 4 + h) * 25 + oy * 5 + ox;
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
      const size_t gitem = (size_t)(sg.slot + img0) * IPI + item;  // counted from slot 0: where the item's output goes
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

// resident blocks of the segment kernels: two 4-wave blocks per CU, one 8-wave block (256 CUs)
constexpr long long kSegGrid4 = 512, kSegGrid8 = 256;
constexpr int kSegImgsL1 = 2, kSegImgs = 8, kSegImgsL4 = 32, kSegImgsL5 = 32, kSegImgsFc = 128;

inline dim3 seg_grid(const MultiLaunch &a, int g, long long resident) {
  return dim3(multi_mfma_bx(((long long)a.max_len + g - 1) / g, a.nsegs, resident), (unsigned)a.nsegs);
}
#define BNN_SEG(kern, G, resident, T, in, out, off) \
  hipLaunchKernelGGL(kern, seg_grid(a, (G), (resident)), dim3(T), 0, a.stream, in, out, a.multi_mfma + (off), a.mfma_stride, a.segs)

}  // namespace

size_t multi_mfma_bytes(NetId net) {
  static_assert(kConvMfmaBytes % 256 == 0 && kConvMfmaA2Bytes % 256 == 0, "a run's tables start on a 256-byte boundary");
  return net == NET_CNVW1A1 ? kConvMfmaBytes : (net == NET_CNVW1A2 || net == NET_CNVW2A2) ? kConvMfmaA2Bytes : 0;
}

hipError_t multi_mfma_tables(NetId net, const uint32_t *const rows[9], size_t stride, int runs, uint8_t *dst, size_t tab_stride, hipStream_t s) {
  if (multi_mfma_bytes(net) == 0 || runs < 1 || runs > 65535 || stride % 4 || tab_stride % 16) return hipErrorInvalidValue;
  const bool a2 = net != NET_CNVW1A1;
  // layer: k steps (K / 64), neuron tiles, table offsets of the 1-bit and of the 2-bit layout
  const struct { int layer, ksteps, tiles; size_t off, off_a2; } part[7] = {
      {1, 9, 2, 0, 0},  {2, 9, 4, kConvMfmaL2Off, kConvMfmaA2L2Off},  {3, 18, 4, kConvMfmaL3Off, kConvMfmaA2L3Off}, {4, 18, 8, kTailMfmaL4Off, kTailMfmaA2L4Off},
      {5, 36, 8, kTailMfmaL5Off, kTailMfmaA2L5Off}, {6, 4, 16, kTailMfmaL6Off, kTailMfmaA2L6Off}, {7, 8, 16, kTailMfmaL7Off, kTailMfmaA2L7Off}};
  for (const auto &p : part) {
    const int entries = p.ksteps * p.tiles * 64 + p.tiles * (a2 ? 64 : 32);
    const dim3 grid((unsigned)((entries + 255) / 256), (unsigned)runs);
    if (!a2) hipLaunchKernelGGL(k_seg_table, grid, dim3(256), 0, s, rows[p.layer], stride / 4, 2 + 2 * p.ksteps, p.ksteps, p.tiles, 64 * p.ksteps, dst + p.off, tab_stride);
    else if (net == NET_CNVW2A2) hipLaunchKernelGGL(k_seg_table_a2<true>, grid, dim3(256), 0, s, rows[p.layer], stride / 4, p.ksteps, p.tiles, dst + p.off_a2, tab_stride);
    else hipLaunchKernelGGL(k_seg_table_a2<false>, grid, dim3(256), 0, s, rows[p.layer], stride / 4, p.ksteps, p.tiles, dst + p.off_a2, tab_stride);
  }
  return hipGetLastError();
}

hipError_t run_cnv_multi_mfma(NetId net, int layer, const MultiLaunch &a) {
  if (multi_mfma_bytes(net) == 0 || !a.multi_mfma || layer < 1 || layer > 7 || a.nsegs < 1 || a.nsegs > 65535 || a.max_len < 1)
    return hipErrorInvalidValue;
  // odd layers read buf0 and write buf1, even layers the other way round (stage_output_bytes)
  const void *const src = layer & 1 ? a.buf0 : a.buf1;
  uint32_t *const dst = reinterpret_cast<uint32_t *>(layer & 1 ? a.buf1 : a.buf0);
  if (net == NET_CNVW1A1) {
    const uint32_t *const in = static_cast<const uint32_t *>(src);
    switch (layer) {
      case 1: BNN_SEG((k_seg_conv_mfma<30, 2, 2, true, kSegImgsL1>), kSegImgsL1, kSegGrid4, 256, in, dst, 0); break;
      case 2: BNN_SEG((k_seg_conv_mfma<14, 2, 4, false, kSegImgs>), kSegImgs, kSegGrid4, 256, in, dst, kConvMfmaL2Off); break;
      case 3: BNN_SEG((k_seg_conv_mfma<12, 4, 4, true, kSegImgs>), kSegImgs, kSegGrid4, 256, in, dst, kConvMfmaL3Off); break;
      case 4: BNN_SEG((k_seg_tail_mfma<false, 18, 8, true, 8, kSegImgsL4>), kSegImgsL4, kSegGrid8, 512, in, dst, kTailMfmaL4Off); break;
      case 5: BNN_SEG((k_seg_tail_mfma<false, 36, 8, false, 8, kSegImgsL5>), kSegImgsL5, kSegGrid8, 512, in, dst, kTailMfmaL5Off); break;
      case 6: BNN_SEG((k_seg_tail_mfma<false, 4, 16, false, 4, kSegImgsFc>), kSegImgsFc, kSegGrid4, 256, in, dst, kTailMfmaL6Off); break;
      default: BNN_SEG((k_seg_tail_mfma<false, 8, 16, false, 8, kSegImgsFc>), kSegImgsFc, kSegGrid8, 512, in, dst, kTailMfmaL7Off); break;
    }
  } else {
    const uint4 *const in = static_cast<const uint4 *>(src);
    switch (layer) {
      case 1: BNN_SEG((k_seg_conv_mfma_a2<30, 2, 2, true, kSegImgsL1>), kSegImgsL1, kSegGrid4, 256, in, dst, 0); break;
      case 2: BNN_SEG((k_seg_conv_mfma_a2<14, 2, 4, false, kSegImgs>), kSegImgs, kSegGrid4, 256, in, dst, kConvMfmaA2L2Off); break;
      case 3: BNN_SEG((k_seg_conv_mfma_a2<12, 4, 4, true, kSegImgs>), kSegImgs, kSegGrid4, 256, in, dst, kConvMfmaA2L3Off); break;
      case 4: BNN_SEG((k_seg_tail_mfma<true, 18, 8, true, 8, kSegImgsL4>), kSegImgsL4, kSegGrid8, 512, in, dst, kTailMfmaA2L4Off); break;
      case 5: BNN_SEG((k_seg_tail_mfma<true, 36, 8, false, 8, kSegImgsL5>), kSegImgsL5, kSegGrid8, 512, in, dst, kTailMfmaA2L5Off); break;
      case 6: BNN_SEG((k_seg_tail_mfma<true, 4, 16, false, 4, kSegImgsFc>), kSegImgsFc, kSegGrid4, 256, in, dst, kTailMfmaA2L6Off); break;
      default: BNN_SEG((k_seg_tail_mfma<true, 8, 16, false, 8, kSegImgsFc>), kSegImgsFc, kSegGrid8, 512, in, dst, kTailMfmaA2L7Off); break;
    }
  }
  return hipPeekAtLastError();  // (left pending: run_cnv_multi reports it behind its last stage)
}

}  // namespace bnn
