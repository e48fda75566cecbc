// glyph_kernels.hip -- one picture and N boxes -> N MNIST-format records (see glyphs.h, glyph_kernels.h).
//
// Four small kernels, each the integer or IEEE form of one of Pillow's steps:
//   k_glyph_luma     L = (R 19595 + G 38470 + B 7471 + 0x8000) >> 16, a thread per 16 pixels of a row (16-byte lanes in,
//                    one 16-byte lane out), the pixel sum through wave shuffles into one 64-bit atomic per block
//   k_glyph_enhance  ImageEnhance.Contrast / .Brightness (Image.blend in single precision, multiply and add rounded
//                    separately: contraction off, never an FMA) and the hard threshold, in place
//   k_glyph_bbox     the bounding box of the pixels != 255 of every box: wave min / max, then four atomics per wave
//   k_glyph_record   one block per glyph: Pillow's two resampling passes of the ink box (arithmetic as in
//                    window_kernels.hip: sums in uint32 that wrap, + 2^21, >> 22, clipped to 8 bits), the horizontal
//                    pass's 8-bit output in LDS (or, past the budget, in a global temporary), the paste on white and
//                    255 / 1 per pixel, written as 49 16-byte stores
#include "glyph_kernels.h"

#include <limits.h>

namespace bnn {
namespace {

constexpr int kPrec = 22;
constexpr int kThreads = 256;
constexpr int kWave = 64;

__device__ __forceinline__ uint8_t clip8(uint32_t ss) {
  const int v = (int)ss >> kPrec;
  return (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v);
}

__device__ __forceinline__ uint32_t byte_of(const uint32_t *raw, int k) { return (raw[k >> 2] >> (8 * (k & 3))) & 0xFF; }

template <int BANDS>
__global__ __launch_bounds__(kThreads) void k_glyph_luma(const GlyphPicture p) {
  __shared__ uint32_t wave_sum[kThreads / kWave];
  const long lanes_per_row = p.plane_pitch / 16;
  const long lane = (long)blockIdx.x * kThreads + threadIdx.x;
  uint32_t sum = 0;
  if (lane < lanes_per_row * p.height) {
    const long y = lane / lanes_per_row, c = lane - y * lanes_per_row;
    // 16 pixels: BANDS whole 16-byte lanes of the row (its pitch is BANDS * plane_pitch)
    const uint4 *__restrict__ in = reinterpret_cast<const uint4 *>(p.src + (size_t)y * (size_t)(p.plane_pitch * BANDS) + (size_t)c * 16 * BANDS);
    uint32_t raw[4 * BANDS];
#pragma unroll
    for (int q = 0; q < BANDS; q++) {
      const uint4 v = in[q];
      raw[4 * q] = v.x; raw[4 * q + 1] = v.y; raw[4 * q + 2] = v.z; raw[4 * q + 3] = v.w;
    }
    const int valid = p.width - (int)(c * 16);  // pixels of this lane inside the picture (the rest is padding)
    uint32_t out[4] = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 16; j++) {
      uint32_t L;
      if constexpr (BANDS == 1) {
        L = byte_of(raw, j);
      } else {
        const uint32_t r = byte_of(raw, BANDS * j), g = byte_of(raw, BANDS * j + 1), b = byte_of(raw, BANDS * j + 2);
        L = (r * 19595u + g * 38470u + b * 7471u + 0x8000u) >> 16;  // Pillow's rgb2l; alpha is ignored
      }
      if (j < valid) sum += L;
      else L = 255;
      out[j >> 2] |= L << (8 * (j & 3));
    }
    *reinterpret_cast<uint4 *>(p.plane + (size_t)y * (size_t)p.plane_pitch + (size_t)c * 16) = make_uint4(out[0], out[1], out[2], out[3]);
  }
  // at most 256 x 16 x 255 per block: 32 bits hold it
#pragma unroll
  for (int d = kWave / 2; d > 0; d >>= 1) sum += __shfl_down(sum, d, kWave);
  if ((threadIdx.x & (kWave - 1)) == 0) wave_sum[threadIdx.x / kWave] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long total = 0;
#pragma unroll
    for (int w = 0; w < kThreads / kWave; w++) total += wave_sum[w];
    if (total) atomicAdd(p.sum, total);
  }
}

// Pillow's ImagingBlend on one 8-bit sample: float(a) + alpha * float(b - a), the multiply and the add rounded
// separately; 0 for t <= 0, 255 for t >= 255, else truncated.  Plain operators with contraction switched off HERE (and
// for the whole file in the Makefile): __fmul_rn / __fadd_rn are plain operators inside the device library's headers,
// and HIP's default -ffp-contract=fast fuses the pair into one v_fma_f32 all the same -- which gives other bytes
// (contrast 1.7, m = 23, v = 13: 6 unfused, 5 fused).
__device__ __forceinline__ uint32_t blend(int a, int b, float alpha) {
#pragma clang fp contract(off)
  const float scaled = alpha * (float)(b - a);
  const float t = (float)a + scaled;
  return t <= 0.f ? 0u : t >= 255.f ? 255u : (uint32_t)(int)t;
}

__global__ __launch_bounds__(kThreads) void k_glyph_enhance(const GlyphPicture p, float contrast, float brightness, int threshold) {
  const long lanes = p.plane_pitch / 16 * p.height;
  const long lane = (long)blockIdx.x * kThreads + threadIdx.x;
  if (lane >= lanes) return;
  const unsigned long long n = (unsigned long long)p.width * (unsigned long long)p.height;
  const int m = (int)((2 * *p.sum + n) / (2 * n));  // int(ImageStat.mean + 0.5)
  uint4 *q = reinterpret_cast<uint4 *>(p.plane) + lane;
  const uint4 v = *q;
  uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int i = 0; i < 4; i++) {
    uint32_t o = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      uint32_t x = (w[i] >> (8 * j)) & 0xFF;
      if (contrast != 1.0f) x = blend(m, (int)x, contrast);
      if (brightness != 1.0f) x = blend(0, (int)x, brightness);
      if (threshold >= 0) x = (int)x > threshold ? 255u : 0u;
      o |= x << (8 * j);
    }
    w[i] = o;
  }
  *q = make_uint4(w[0], w[1], w[2], w[3]);
}

constexpr int kBboxRows = 32;  // rows of a box per block of k_glyph_bbox

__global__ __launch_bounds__(kThreads) void k_glyph_bbox(const GlyphPicture p, const int32_t *__restrict__ boxes, int32_t *found) {
  const int i = blockIdx.y;
  const int4 box = reinterpret_cast<const int4 *>(boxes)[i];
  const int y_first = box.y + (int)blockIdx.x * kBboxRows;
  if (y_first >= box.w) return;  // (the grid is sized for the tallest box of the call)
  const int y_end = min(y_first + kBboxRows, box.w);
  int lo_x = INT_MAX, lo_y = INT_MAX, hi_x = -1, hi_y = -1;
  const int bw = box.z - box.x;
  const int cells = bw * (y_end - y_first);
  for (int c = threadIdx.x; c < cells; c += kThreads) {
    const int dy = c / bw, x = box.x + (c - dy * bw), y = y_first + dy;
    if (p.plane[(size_t)y * (size_t)p.plane_pitch + x] != 255) {
      lo_x = min(lo_x, x); hi_x = max(hi_x, x);
      lo_y = min(lo_y, y); hi_y = max(hi_y, y);
    }
  }
#pragma unroll
  for (int d = kWave / 2; d > 0; d >>= 1) {
    lo_x = min(lo_x, __shfl_xor(lo_x, d, kWave)); lo_y = min(lo_y, __shfl_xor(lo_y, d, kWave));
    hi_x = max(hi_x, __shfl_xor(hi_x, d, kWave)); hi_y = max(hi_y, __shfl_xor(hi_y, d, kWave));
  }
  if ((threadIdx.x & (kWave - 1)) == 0 && hi_x >= 0) {
    atomicMin(found + 4 * (size_t)i, lo_x); atomicMin(found + 4 * (size_t)i + 1, lo_y);
    atomicMax(found + 4 * (size_t)i + 2, hi_x); atomicMax(found + 4 * (size_t)i + 3, hi_y);
  }
}

__global__ __launch_bounds__(kThreads) void k_glyph_record(const GlyphPicture p, const GlyphDesc *__restrict__ desc, const int32_t *__restrict__ coef,
                                                           uint8_t *tmp, uint8_t *__restrict__ records) {
  __shared__ __attribute__((aligned(16))) uint8_t lds_mid[kGlyphMidBytes];  // the horizontal pass's output, h x out_w
  __shared__ __attribute__((aligned(16))) uint8_t fin[kGlyphRecord];        // the resized glyph, out_h x out_w
  const int t = threadIdx.x;
  const GlyphDesc d = desc[blockIdx.x];
  if (d.flags & kGlyphSkip) return;  // status 2: nothing is written
  const bool blank = (d.flags & kGlyphBlank) != 0;
  const bool horizontal = (d.flags & kGlyphHorizontal) != 0, vertical = (d.flags & kGlyphVertical) != 0;
  const int out_w = d.out_w, out_h = d.out_h;
  const size_t pitch = (size_t)p.plane_pitch;
  const uint8_t *__restrict__ origin = p.plane + (size_t)d.y0 * pitch + (size_t)d.x0;
  uint8_t *mid = (d.flags & kGlyphGlobalMid) ? tmp + (size_t)d.tmp : lds_mid;
  if (!blank) {
    if (horizontal) {
      // mid[y][xx] = clip8(2^21 + sum_x ink[y][xmin + x] * k[xx][x]); all h rows when a vertical pass follows, which
      // then is out_h of them
      const int32_t *__restrict__ kh = coef + d.kh, *__restrict__ bh = coef + d.bh;
      const int n = d.h * out_w;
      for (int i = t; i < n; i += kThreads) {
        const int y = i / out_w, xx = i - y * out_w;
        const int xmin = bh[2 * xx], taps = bh[2 * xx + 1];
        const int32_t *__restrict__ k = kh + (size_t)xx * d.ksize_h;
        const uint8_t *__restrict__ px = origin + (size_t)y * pitch + xmin;
        uint32_t acc = 1u << (kPrec - 1);
        for (int x = 0; x < taps; x++) acc += (uint32_t)px[x] * (uint32_t)k[x];
        mid[i] = clip8(acc);
      }
      __syncthreads();
    }
    const int32_t *__restrict__ kv = coef + d.kv, *__restrict__ bv = coef + d.bv;
    const int n = out_h * out_w;
    for (int i = t; i < n; i += kThreads) {
      const int yy = i / out_w, xx = i - yy * out_w;
      uint8_t v;
      if (vertical) {
        const int ymin = bv[2 * yy], taps = bv[2 * yy + 1];
        const int32_t *__restrict__ k = kv + (size_t)yy * d.ksize_v;
        uint32_t acc = 1u << (kPrec - 1);
        if (horizontal) {
          const uint8_t *px = mid + (size_t)ymin * out_w + xx;
          for (int y = 0; y < taps; y++) acc += (uint32_t)px[(size_t)y * out_w] * (uint32_t)k[y];
        } else {  // out_w == w: straight from the plane
          const uint8_t *__restrict__ px = origin + (size_t)ymin * pitch + xx;
          for (int y = 0; y < taps; y++) acc += (uint32_t)px[(size_t)y * pitch] * (uint32_t)k[y];
        }
        v = clip8(acc);
      } else if (horizontal) {
        v = mid[i];
      } else {  // already out_w x out_h: Image.resize returns a copy
        v = origin[(size_t)yy * pitch + xx];
      }
      fin[i] = v;
    }
    __syncthreads();
  }
  // paste on white, then cell 13's rule: 255 where the pasted pixel is exactly 0, 1 everywhere else
  if (t < kGlyphRecord / 16) {
    uint32_t out[4] = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 16; j++) {
      const int pos = 16 * t + j;
      const int cy = pos / kGlyphSide, cx = pos - cy * kGlyphSide;
      const int yy = cy - d.off_y, xx = cx - d.off_x;
      uint32_t v = 255;
      if (!blank && yy >= 0 && yy < out_h && xx >= 0 && xx < out_w) v = fin[yy * out_w + xx];
      out[j >> 2] |= (v == 0 ? 255u : 1u) << (8 * (j & 3));
    }
    reinterpret_cast<uint4 *>(records + (size_t)blockIdx.x * kGlyphRecord)[t] = make_uint4(out[0], out[1], out[2], out[3]);
  }
}

}  // namespace

hipError_t launch_glyph_luma(const GlyphPicture &p, hipStream_t s) {
  const long lanes = p.plane_pitch / 16 * p.height;
  const dim3 grid((unsigned)((lanes + kThreads - 1) / kThreads)), block(kThreads);
  if (p.bands == 3) hipLaunchKernelGGL(k_glyph_luma<3>, grid, block, 0, s, p);
  else if (p.bands == 4) hipLaunchKernelGGL(k_glyph_luma<4>, grid, block, 0, s, p);
  else hipLaunchKernelGGL(k_glyph_luma<1>, grid, block, 0, s, p);
  return hipGetLastError();
}

hipError_t launch_glyph_enhance(const GlyphPicture &p, float contrast, float brightness, int threshold, hipStream_t s) {
  const long lanes = p.plane_pitch / 16 * p.height;
  const dim3 grid((unsigned)((lanes + kThreads - 1) / kThreads)), block(kThreads);
  hipLaunchKernelGGL(k_glyph_enhance, grid, block, 0, s, p, contrast, brightness, threshold);
  return hipGetLastError();
}

hipError_t launch_glyph_bbox(const GlyphPicture &p, const int32_t *boxes, int32_t *found, int n, int max_box_height, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  const dim3 block(kThreads);
  // the y dimension of a grid holds 65535 blocks: more boxes than that go in slices
  for (int first = 0; first < n; first += 65535) {
    const int m = n - first < 65535 ? n - first : 65535;
    const dim3 grid((unsigned)((max_box_height + kBboxRows - 1) / kBboxRows), (unsigned)m);
    hipLaunchKernelGGL(k_glyph_bbox, grid, block, 0, s, p, boxes + 4 * (size_t)first, found + 4 * (size_t)first);
  }
  return hipGetLastError();
}

hipError_t launch_glyph_record(const GlyphPicture &p, const GlyphDesc *desc, const int32_t *coef, uint8_t *tmp, uint8_t *records, int n,
                               hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_glyph_record, dim3((unsigned)n), dim3(kThreads), 0, s, p, desc, coef, tmp, records);
  return hipGetLastError();
}

}  // namespace bnn
