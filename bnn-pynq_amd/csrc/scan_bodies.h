// The lane bodies of the dense scan (scan_kernels.hip) and of the clip scan (scan_clip_kernels.hip), stated once: what a
// lane does once it knows its item, as __device__ __forceinline__ functions that take the item, and the order of the two
// resize passes (resize_route, host).  The two kernel files differ only in how a lane finds its item and its map.  The
// neuron loops are copies of k_conv0's, k_quad_x's and k_vec_x's, statement for statement: the shipped bodies
// (kernels.hip) are pinned by build tests and stay where they are (see the comment above vec_x_group there).
//
// The mapping is that of DESIGN.md 5: one lane owns one output pixel (layers 0, 4, 5) or one 2 x 2 quad (layers 1-3; the
// pool is a min over the quad before the sign), `cg` picks the group of 32 neurons, whose rows are wave-uniform and come
// through scalar loads from the packed blob as it is ({t0, t1, words...}); 32 decisions make one dword of the bit-packed
// HWC map.  No LDS.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bnn {
namespace {

typedef const uint32_t __attribute__((address_space(4))) *kptr32;  // scalar (constant) address space: uniform loads become s_load_*

constexpr int kBlock = 256;

// ---- the helpers of kernels.hip these loops are written with (copies: that file's are in its anonymous namespace) ----
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
__device__ __forceinline__ uint32_t chain_temp() {
  uint32_t t;
  asm("" : "=v"(t));
  return t;
}
#define SCAN_SCALAR_COUNTER(c) asm volatile("" : "+s"(c))
// one (v_xor, v_bcnt) pair per statement, `t` threaded through all of them (kernels.hip: the cadence of the XNOR path)
__device__ __forceinline__ void xpop(int &acc, uint32_t w, uint32_t a, uint32_t &t) {
  asm("v_xor_b32 %0, %2, %3\n\tv_bcnt_u32_b32 %1, %0, %1" : "+v"(t), "+v"(acc) : "s"(w), "v"(a));
}
__device__ __forceinline__ void xpop4(int &m0, int &m1, int &m2, int &m3, uint32_t w, uint32_t a0, uint32_t a1, uint32_t a2, uint32_t a3,
                                      uint32_t &t) {
  xpop(m0, w, a0, t); xpop(m1, w, a1, t); xpop(m2, w, a2, t); xpop(m3, w, a3, t);
}
__device__ __forceinline__ int xpop_seed(uint32_t w, uint32_t a, int seed, uint32_t &t) {
  int acc;
  asm("v_xor_b32 %0, %2, %3\n\tv_bcnt_u32_b32 %1, %0, %4" : "+v"(t), "=v"(acc) : "s"(w), "v"(a), "s"(seed));
  return acc;
}

// ---- layer 0: planar uint8 picture -> (ow x oh) x 64 thresholded map ---------------------------------------------------
// item = oy * ow + ox.  The 27 taps are read as bytes (a row of an arbitrary picture is not dword aligned) and packed as
// k_conv0 packs them: tap 3 (3 c + ky) + kx at byte tau % 4 of dword tau / 4, byte 27 a zero whose weight byte is 0.
__device__ __forceinline__ void scan_conv0_item(const uint8_t *__restrict__ planes, long row_stride, long plane_stride, uint32_t *__restrict__ out,
                                                const uint32_t *__restrict__ rows, int ow, int item, int cg) {
  const int oy = item / ow, ox = item - oy * ow;
  const uint8_t *__restrict__ p = planes + (size_t)oy * row_stride + ox;
  uint32_t g[9];
#pragma unroll
  for (int c = 0; c < 3; c++)
#pragma unroll
    for (int r = 0; r < 3; r++) {
      const uint8_t *__restrict__ q = p + (size_t)c * plane_stride + (size_t)r * row_stride;
      g[c * 3 + r] = (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16);
    }
  uint32_t a[7];
#pragma unroll
  for (int h = 0; h < 2; h++) {
    a[3 * h + 0] = __builtin_amdgcn_perm(g[4 * h + 1], g[4 * h + 0], 0x04020100u);
    a[3 * h + 1] = __builtin_amdgcn_perm(g[4 * h + 2], g[4 * h + 1], 0x05040201u);
    a[3 * h + 2] = __builtin_amdgcn_perm(g[4 * h + 3], g[4 * h + 2], 0x06050402u);
  }
  a[6] = g[8];
#pragma unroll
  for (int j = 0; j < 7; j++) a[j] = quantise4(a[j]);
  kptr32 w = (kptr32)(uintptr_t)(rows + (size_t)cg * 32 * 12);
  uint32_t b0 = 0;
  // two neurons per iteration; each accumulator starts at ~t, so that acc < 0 <=> dot <= t <=> !fire (k_conv0)
  for (int c = 31; c >= 0; c -= 2) {
    kptr32 rA = w + c * 12, rB = rA - 12;
    int accA = ~(int)rA[0], accB = ~(int)rB[0];
#pragma unroll
    for (int k = 0; k < 7; k++) {
      accA = __builtin_amdgcn_sdot4((int)a[k], (int)rA[2 + k], accA, false);
      asm("" : "+v"(accA));
      accB = __builtin_amdgcn_sdot4((int)a[k], (int)rB[2 + k], accB, false);
      asm("" : "+v"(accB));
    }
    b0 = shift_in_sign(b0, accA);
    b0 = shift_in_sign(b0, accB);
  }
  out[(size_t)item * 2 + cg] = ~b0;  // collected !fire
}

// ---- layers 1-3: one lane = one 2 x 2 quad of conv outputs ----------------------------------------------------------------
// in: [ih][iw][CW] u64; item = qy * qw + qx, the quad at conv outputs (2 qy .. 2 qy + 1, 2 qx .. 2 qx + 1), whose 4 x 4
// input patch starts at the same coordinates.  POOL: out [qh][qw][groups]; else out [2 qh][2 qw][groups].
template <int CW, bool POOL>
__device__ __forceinline__ void scan_quad_item(const uint64_t *__restrict__ in, uint32_t *__restrict__ out, const uint32_t *__restrict__ rows, int iw,
                                               int qw, int item, int cg, int groups) {
  constexpr int KW = 9 * CW, ROW_DW = 2 + 2 * KW;
  const int qy = item / qw, qx = item - qy * qw;
  const uint64_t *__restrict__ base = in + ((size_t)(2 * qy) * iw + 2 * qx) * CW;
  uint32_t wl[4][4][CW], wh[4][4][CW];
#pragma unroll
  for (int y = 0; y < 4; y++)
#pragma unroll
    for (int x = 0; x < 4; x++)
#pragma unroll
      for (int k = 0; k < CW; k++) {
        const uint64_t v = base[((size_t)y * iw + x) * CW + k];
        wl[y][x][k] = (uint32_t)v;
        wh[y][x][k] = (uint32_t)(v >> 32);
      }
  uint32_t t = chain_temp();
  kptr32 w = (kptr32)(uintptr_t)(rows + (size_t)cg * 32 * ROW_DW);
  uint32_t b[4] = {0, 0, 0, 0};
  for (int c = 31; c >= 0; c--) {
    kptr32 r = w + c * ROW_DW;
    SCAN_SCALAR_COUNTER(c);
    const int nt = -(int)r[0];  // every chain starts at -t: it ends on m - t, whose sign is the decision
    int m[2][2];
#pragma unroll
    for (int j = 0; j < KW; j++) {
      const int ky = j / (3 * CW), kx = (j / CW) % 3, k = j % CW;
      const uint32_t w0 = r[2 + 2 * j], w1 = r[3 + 2 * j];
      if (j == 0) {
#pragma unroll
        for (int i = 0; i < 4; i++) m[i >> 1][i & 1] = xpop_seed(w0, wl[ky + (i >> 1)][kx + (i & 1)][k], nt, t);
      } else {
        xpop4(m[0][0], m[0][1], m[1][0], m[1][1], w0, wl[ky][kx][k], wl[ky][kx + 1][k], wl[ky + 1][kx][k], wl[ky + 1][kx + 1][k], t);
      }
      xpop4(m[0][0], m[0][1], m[1][0], m[1][1], w1, wh[ky][kx][k], wh[ky][kx + 1][k], wh[ky + 1][kx][k], wh[ky + 1][kx + 1][k], t);
    }
    if constexpr (POOL) {  // OR of the four fire bits == (min (m - t)) < 0
      b[0] = shift_in_sign(b[0], min(min(m[0][0], m[0][1]), min(m[1][0], m[1][1])));
    } else {
#pragma unroll
      for (int i = 0; i < 4; i++) b[i] = shift_in_sign(b[i], m[i >> 1][i & 1]);
    }
  }
  if constexpr (POOL) {
    out[(size_t)item * groups + cg] = b[0];
  } else {
    const int ow = 2 * qw;
#pragma unroll
    for (int i = 0; i < 4; i++) out[((size_t)(2 * qy + (i >> 1)) * ow + 2 * qx + (i & 1)) * groups + cg] = b[i];
  }
}

// ---- layers 4 and 5: one lane = one output pixel, its 3 x 3 window gathered into KW = 9 CW words ------------------------
// in: [ih][iw][CW] u64; item = oy * ow + ox; out [oh][ow][groups].  Two neurons per iteration (k_vec_x).
template <int CW>
__device__ __forceinline__ void scan_vec_item(const uint64_t *__restrict__ in, uint32_t *__restrict__ out, const uint32_t *__restrict__ rows, int iw,
                                              int ow, int item, int cg, int groups) {
  constexpr int KW = 9 * CW, ROW_DW = 2 + 2 * KW;
  const int oy = item / ow, ox = item - oy * ow;
  const uint64_t *__restrict__ base = in + ((size_t)oy * iw + ox) * CW;
  uint32_t al[KW], ah[KW];
#pragma unroll
  for (int ky = 0; ky < 3; ky++)
#pragma unroll
    for (int kx = 0; kx < 3; kx++)
#pragma unroll
      for (int k = 0; k < CW; k++) {
        const uint64_t v = base[((size_t)ky * iw + kx) * CW + k];
        al[(ky * 3 + kx) * CW + k] = (uint32_t)v;
        ah[(ky * 3 + kx) * CW + k] = (uint32_t)(v >> 32);
      }
  uint32_t t = chain_temp();
  kptr32 w = (kptr32)(uintptr_t)(rows + (size_t)cg * 32 * ROW_DW);
  uint32_t b = 0;
  for (int c = 31; c >= 0; c -= 2) {
    kptr32 r1 = w + c * ROW_DW, r0 = r1 - ROW_DW;
    int m1 = xpop_seed(r1[2], al[0], -(int)r1[0], t), m0 = xpop_seed(r0[2], al[0], -(int)r0[0], t);
    xpop(m1, r1[3], ah[0], t);
    xpop(m0, r0[3], ah[0], t);
#pragma unroll
    for (int k = 1; k < KW; k++) {
      xpop(m1, r1[2 + 2 * k], al[k], t);
      xpop(m0, r0[2 + 2 * k], al[k], t);
      xpop(m1, r1[3 + 2 * k], ah[k], t);
      xpop(m0, r0[3 + 2 * k], ah[k], t);
    }
    b = shift_in_sign(b, m1);
    b = shift_in_sign(b, m0);
  }
  out[(size_t)item * groups + cg] = b;
}

// ---- Image.resize(..., LANCZOS): Pillow's two 8-bit passes, one lane per output pixel ----------------------------------
constexpr int kPrec = 22;
__device__ __forceinline__ uint8_t clip8(uint32_t ss) {
  const int v = (int)ss >> kPrec;
  return (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v);
}
// where an output sample goes: band b of pixel (y, x) at dst + b * plane + y * row + x * pix; `triple`: a grey sample
// into three planes
struct ResizeOut { uint8_t *dst; long plane, row, pix; int triple; };
template <int BANDS>
__device__ __forceinline__ void put(const ResizeOut &o, int y, int x, const uint32_t (&acc)[BANDS]) {
  uint8_t *__restrict__ d = o.dst + (size_t)y * o.row + (size_t)x * o.pix;
  if (BANDS == 1 && o.triple) {
    const uint8_t v = clip8(acc[0]);
    d[0] = v; d[o.plane] = v; d[2 * o.plane] = v;
  } else {
#pragma unroll
    for (int b = 0; b < BANDS; b++) d[(size_t)b * o.plane] = clip8(acc[b]);
  }
}
//   out[y][xx][b] = clip8(2^21 + sum_x src[y][xmin + x][b] * k[xx][x])      (sums wrap mod 2^32 like Pillow's ints)
template <int BANDS>
__device__ __forceinline__ void resize_h_item(const uint8_t *__restrict__ src, long pitch, int out_w, const int32_t *__restrict__ kk,
                                              const int32_t *__restrict__ bounds, int ksize, const ResizeOut &o, long idx) {
  const int y = (int)(idx / out_w), xx = (int)(idx - (long)y * out_w);
  const int xmin = bounds[2 * xx], xmax = bounds[2 * xx + 1];
  const uint8_t *__restrict__ row = src + (size_t)y * pitch + (size_t)xmin * BANDS;
  const int32_t *__restrict__ k = kk + (size_t)xx * ksize;
  uint32_t acc[BANDS];
#pragma unroll
  for (int b = 0; b < BANDS; b++) acc[b] = 1u << (kPrec - 1);
  for (int j = 0; j < xmax; j++)
#pragma unroll
    for (int b = 0; b < BANDS; b++) acc[b] += (uint32_t)row[j * BANDS + b] * (uint32_t)k[j];
  put<BANDS>(o, y, xx, acc);
}
//   out[yy][x][b] = clip8(2^21 + sum_y src[ymin + y][x][b] * k[yy][y]);   !vertical: out = src (the re-layout alone)
template <int BANDS>
__device__ __forceinline__ void resize_v_item(const uint8_t *__restrict__ src, long pitch, int w, const int32_t *__restrict__ kk,
                                              const int32_t *__restrict__ bounds, int ksize, int vertical, const ResizeOut &o, long idx) {
  const int yy = (int)(idx / w), x = (int)(idx - (long)yy * w);
  uint32_t acc[BANDS];
  if (vertical) {
    const int ymin = bounds[2 * yy], ymax = bounds[2 * yy + 1];
    const uint8_t *__restrict__ col = src + (size_t)ymin * pitch + (size_t)x * BANDS;
    const int32_t *__restrict__ k = kk + (size_t)yy * ksize;
#pragma unroll
    for (int b = 0; b < BANDS; b++) acc[b] = 1u << (kPrec - 1);
    for (int y = 0; y < ymax; y++)
#pragma unroll
      for (int b = 0; b < BANDS; b++) acc[b] += (uint32_t)col[(size_t)y * pitch + b] * (uint32_t)k[y];
  } else {
#pragma unroll
    for (int b = 0; b < BANDS; b++) acc[b] = (uint32_t)src[(size_t)yy * pitch + (size_t)x * BANDS + b] << kPrec;
  }
  put<BANDS>(o, yy, x, acc);
}

inline dim3 grid_of(long items) { return dim3((unsigned)((items + kBlock - 1) / kBlock)); }

// ---- the order of the passes of Image.resize((out_w, out_h)) of an h x w x bands picture, rows `stride` bytes apart ------
// A pass reads the picture or (from_tmp) the pass before it in `tmp`, packed rows.  horizontal: the resize_h kernel with
// the horizontal tables over `extent` rows, `out` = out_w; else the resize_v kernel with the vertical tables over
// `extent` columns, `out` = out_h, which only re-lays its source out where !vertical.
struct ResizePass { bool horizontal, from_tmp; long items, pitch; int extent, out, vertical; ResizeOut o; };
struct ResizeRoute { int n; ResizePass pass[2]; };
inline ResizeRoute resize_route(int w, int h, int bands, int out_w, int out_h, bool vertical_first, long stride, uint8_t *tmp, uint8_t *planes) {
  const bool horizontal = out_w != w, vertical = out_h != h;
  const ResizeOut planar{planes, (long)out_w * out_h, out_w, 1, bands == 1 ? 1 : 0};
  if (horizontal && vertical && vertical_first) {
    const ResizeOut mid{tmp, 1, (long)w * bands, bands, 0};
    return {2, {{false, false, (long)out_h * w, stride, w, out_h, 1, mid}, {true, true, (long)out_h * out_w, mid.row, out_h, out_w, 0, planar}}};
  }
  // a pass whose size does not change is skipped; the vertical kernel always runs last, for the planar layout
  // (Pillow runs the horizontal pass over the rows the vertical pass will read; over all rows it gives the same samples)
  const ResizeOut mid{tmp, 1, (long)out_w * bands, bands, 0};
  const ResizePass first{true, false, (long)h * out_w, stride, h, out_w, 0, mid};
  const ResizePass last{false, horizontal, (long)out_h * out_w, horizontal ? mid.row : stride, out_w, out_h, vertical ? 1 : 0, planar};
  return horizontal ? ResizeRoute{2, {first, last}} : ResizeRoute{1, {last}};
}

}  // namespace
}  // namespace bnn
