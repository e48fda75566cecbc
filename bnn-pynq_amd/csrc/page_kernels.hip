// page_kernels.hip -- one picture, its label plane and N components -> N MNIST-format records, each of the component's own
// ink alone (see page.h, page_kernels.h).
//
//   k_page_record   the masked twin of k_glyph_record (glyph_kernels.hip): one 256-thread block per glyph, Pillow's two
//                   resampling passes in the same fixed-point arithmetic (sums in uint32 that wrap, + 2^21, >> 22, clipped
//                   to 8 bits), the horizontal pass's 8-bit output in LDS (or, past the budget, in a global temporary),
//                   the paste on white and 255 / 1 per pixel, written as 49 16-byte stores.  The three places that read
//                   the plane -- the horizontal pass's taps, the vertical-only pass when out_w == w, the plain copy when
//                   the box already is the output size -- take member ? plane[p] : 255, where member is one compare of
//                   the pixel's label against each of the glyph's two key values.
#include "page_kernels.h"

namespace bnn {
namespace {

constexpr int kPrec = 22;
constexpr int kThreads = 256;

__device__ __forceinline__ uint8_t clip8(uint32_t ss) {
  const int v = (int)ss >> kPrec;
  return (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v);
}

__global__ __launch_bounds__(kThreads) void k_page_record(const GlyphPicture p, const int32_t *__restrict__ label,
                                                          const GlyphDesc *__restrict__ desc, const int32_t *__restrict__ keys,
                                                          const int32_t *__restrict__ coef, uint8_t *tmp, uint8_t *__restrict__ records) {
  __shared__ __attribute__((aligned(16))) uint8_t lds_mid[kGlyphMidBytes];  // the horizontal pass's output, h x out_w
  __shared__ __attribute__((aligned(16))) uint8_t fin[kGlyphRecord];        // the resized glyph, out_h x out_w
  const int t = threadIdx.x;
  const GlyphDesc d = desc[blockIdx.x];
  if (d.flags & kGlyphSkip) return;  // status 2: nothing is written
  const bool blank = (d.flags & kGlyphBlank) != 0;
  const bool horizontal = (d.flags & kGlyphHorizontal) != 0, vertical = (d.flags & kGlyphVertical) != 0;
  const int out_w = d.out_w, out_h = d.out_h;
  const size_t pitch = (size_t)p.plane_pitch, width = (size_t)p.width;
  const uint8_t *__restrict__ origin = p.plane + (size_t)d.y0 * pitch + (size_t)d.x0;
  const int32_t *__restrict__ owner = label + (size_t)d.y0 * width + (size_t)d.x0;
  const int32_t key_first = keys[2 * (size_t)blockIdx.x], key_root = keys[2 * (size_t)blockIdx.x + 1];
  // the glyph's picture at (x, y) of its box: its own ink, white everywhere else
  // (both loads are issued whatever the label says -- either address lies inside the picture -- so that a tap is two
  // independent loads and a select, not a load behind a branch)
  auto ink = [&](size_t y, size_t x) -> uint32_t {
    const int32_t l = owner[y * width + x];
    const uint32_t v = origin[y * pitch + x];
    return (l == key_first || l == key_root) ? v : 255u;
  };
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
        uint32_t acc = 1u << (kPrec - 1);
        for (int x = 0; x < taps; x++) acc += ink((size_t)y, (size_t)(xmin + x)) * (uint32_t)k[x];
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
          for (int y = 0; y < taps; y++) acc += ink((size_t)(ymin + y), (size_t)xx) * (uint32_t)k[y];
        }
        v = clip8(acc);
      } else if (horizontal) {
        v = mid[i];
      } else {  // already out_w x out_h: Image.resize returns a copy
        v = (uint8_t)ink((size_t)yy, (size_t)xx);
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

hipError_t launch_page_record(const GlyphPicture &p, const int32_t *label, const GlyphDesc *desc, const int32_t *keys, const int32_t *coef,
                              uint8_t *tmp, uint8_t *records, int n, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_page_record, dim3((unsigned)n), dim3(kThreads), 0, s, p, label, desc, keys, coef, tmp, records);
  return hipGetLastError();
}

}  // namespace bnn
