// The pixel formats' kernel (pixfmt_kernels.h; the model: pixfmt.h; DESIGN.md 9, "Camera frames").
//
// A unit is 8 pixels of one row (two rows for the 4:2:0 formats); unit u of a frame is lane u of the launch, so that the
// lanes of a wave read and write consecutive addresses.  The wide path holds its input and its 24 output bytes a row in
// registers: every index below is a constant after unrolling.
#define BNN_HD __host__ __device__
#include "pixfmt_kernels.h"

namespace bnn {
namespace {

// byte k of words held in registers (k is a constant where this is called)
__device__ __forceinline__ int byte_of(const uint32_t *w, int k) { return (int)((w[k >> 2] >> (8 * (k & 3))) & 255u); }
__device__ __forceinline__ void put_byte(uint32_t *w, int k, int v) { w[k >> 2] |= (uint32_t)v << (8 * (k & 3)); }

__device__ __forceinline__ void load8(uint32_t *w, const uint8_t *p) {
  const uint2 v = *reinterpret_cast<const uint2 *>(p);
  w[0] = v.x; w[1] = v.y;
}

// the 24 bytes of 8 RGB pixels to p, which is `align`-byte aligned (uniform over the launch)
__device__ __forceinline__ void store24(uint8_t *p, const uint32_t *w, int align) {
  if (align >= 8) {
#pragma unroll
    for (int k = 0; k < 3; k++) reinterpret_cast<uint2 *>(p)[k] = make_uint2(w[2 * k], w[2 * k + 1]);
  } else if (align >= 4) {
#pragma unroll
    for (int k = 0; k < 6; k++) reinterpret_cast<uint32_t *>(p)[k] = w[k];
  } else {
#pragma unroll
    for (int k = 0; k < 24; k++) p[k] = (uint8_t)byte_of(w, k);
  }
}

template <int FORMAT>
__global__ __launch_bounds__(kUnpackBlock) void k_unpack_frames(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, int w, int h, long stride,
                                                                long frame_stride, int range, int units_x, int units, int in_wide, int out_align) {
  constexpr int kRows = pix_is_420(FORMAT) ? 2 : 1, kN = kUnpackPixels;
  const int u = blockIdx.x * kUnpackBlock + threadIdx.x;
  if (u >= units) return;
  const int uy = u / units_x, x0 = (u - uy * units_x) * kN, y0 = uy * kRows;
  const uint8_t *__restrict__ f = src + (size_t)blockIdx.y * frame_stride;
  uint8_t *__restrict__ o = dst + (((size_t)blockIdx.y * h + y0) * w + x0) * 3;
  if (!in_wide || x0 + kN > w) {
    for (int r = 0; r < kRows; r++)
      for (int i = 0; i < kN && x0 + i < w; i++) pix_unpack_one(FORMAT, f, (size_t)stride, h, range, x0 + i, y0 + r, o + ((size_t)r * w + i) * 3);
    return;
  }

  uint32_t out[kRows][6] = {};
  if constexpr (FORMAT == PIX_RGB || FORMAT == PIX_BGR) {
    uint32_t q[6];
    const uint8_t *p = f + (size_t)y0 * stride + (size_t)x0 * 3;
#pragma unroll
    for (int k = 0; k < 3; k++) load8(q + 2 * k, p + 8 * k);
#pragma unroll
    for (int k = 0; k < 24; k++) put_byte(out[0], k, byte_of(q, FORMAT == PIX_BGR ? 3 * (k / 3) + 2 - k % 3 : k));
  } else if constexpr (FORMAT == PIX_L) {
    uint32_t q[2];
    load8(q, f + (size_t)y0 * stride + x0);
#pragma unroll
    for (int k = 0; k < 24; k++) put_byte(out[0], k, byte_of(q, k / 3));
  } else {
    // luma[r]: the 8 Y bytes of row r; cbw, crw: the 4 Cb and the 4 Cr bytes of the unit
    uint32_t luma[kRows][2], cbw[1] = {0}, crw[1] = {0};
    if constexpr (FORMAT == PIX_YUYV) {
      uint32_t q[4];
      const uint4 v = *reinterpret_cast<const uint4 *>(f + (size_t)y0 * stride + (size_t)x0 * 2);
      q[0] = v.x; q[1] = v.y; q[2] = v.z; q[3] = v.w;
      luma[0][0] = luma[0][1] = 0;
#pragma unroll
      for (int j = 0; j < 4; j++) {  // a dword is Y0 Cb Y1 Cr
        put_byte(luma[0], 2 * j, byte_of(q, 4 * j));
        put_byte(luma[0], 2 * j + 1, byte_of(q, 4 * j + 2));
        put_byte(cbw, j, byte_of(q, 4 * j + 1));
        put_byte(crw, j, byte_of(q, 4 * j + 3));
      }
    } else {
#pragma unroll
      for (int r = 0; r < kRows; r++) load8(luma[r], f + (size_t)(y0 + r) * stride + x0);
      if constexpr (FORMAT == PIX_NV12) {
        uint32_t q[2];
        load8(q, f + (size_t)(h + uy) * stride + x0);
#pragma unroll
        for (int j = 0; j < 4; j++) {
          put_byte(cbw, j, byte_of(q, 2 * j));
          put_byte(crw, j, byte_of(q, 2 * j + 1));
        }
      } else {
        const size_t half = (size_t)stride / 2;
        const uint8_t *p = f + (size_t)h * stride + (size_t)uy * half + x0 / 2;
        cbw[0] = *reinterpret_cast<const uint32_t *>(p);
        crw[0] = *reinterpret_cast<const uint32_t *>(p + (size_t)(h / 2) * half);
      }
    }
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const PixChroma c = pix_chroma(range, byte_of(cbw, j), byte_of(crw, j));
#pragma unroll
      for (int r = 0; r < kRows; r++)
#pragma unroll
        for (int i = 2 * j; i < 2 * j + 2; i++) {
          const int y = byte_of(luma[r], i);
          put_byte(out[r], 3 * i, pix_channel(range, y, c.r));
          put_byte(out[r], 3 * i + 1, pix_channel(range, y, c.g));
          put_byte(out[r], 3 * i + 2, pix_channel(range, y, c.b));
        }
    }
  }
#pragma unroll
  for (int r = 0; r < kRows; r++) store24(o + (size_t)r * w * 3, out[r], out_align);
}

template <int FORMAT>
void launch(const UnpackLaunch &a, dim3 grid, int units_x, int units, int in_wide, int out_align) {
  hipLaunchKernelGGL(k_unpack_frames<FORMAT>, grid, dim3(kUnpackBlock), 0, a.stream, a.src, a.dst, a.frames.width, a.frames.height,
                     (long)a.layout.rows_apart, (long)a.layout.frames_apart, a.frames.range, units_x, units, in_wide, out_align);
}

}  // namespace

hipError_t run_unpack_frames(const UnpackLaunch &a) {
  const Frames &f = a.frames;
  const PixLayout &l = a.layout;
  if (f.format < 0 || f.format >= PIX_FORMATS || f.width < 1 || f.height < 1 || f.width > kPixMaxSide || f.height > kPixMaxSide || f.n_frames < 1 ||
      f.n_frames > kPixMaxFrames || l.n_frames != f.n_frames || l.rows_apart < (size_t)pix_row_bytes(f.format, f.width) ||
      l.frames_apart < l.rows_apart * (size_t)l.rows || (pix_is_yuv(f.format) && (f.width & 1)) || (pix_is_420(f.format) && (f.height & 1)) ||
      (f.format == PIX_I420 && (l.rows_apart & 1)))
    return hipErrorInvalidValue;
  // the wide loads: 16 bytes a lane for YUYV, 8 for the others (I420's 4-byte chroma loads lie at half an 8-byte stride)
  const uintptr_t need = f.format == PIX_YUYV ? 16 : 8;
  const int in_wide = reinterpret_cast<uintptr_t>(a.src) % need == 0 && l.rows_apart % need == 0 && (f.n_frames == 1 || l.frames_apart % need == 0);
  const size_t out_row = (size_t)f.width * 3;
  const uintptr_t out = reinterpret_cast<uintptr_t>(a.dst);
  const int out_align = (out % 8 == 0 && out_row % 8 == 0) ? 8 : ((out % 4 == 0 && out_row % 4 == 0) ? 4 : 1);
  const int units_x = (f.width + kUnpackPixels - 1) / kUnpackPixels, units = units_x * (pix_is_420(f.format) ? f.height / 2 : f.height);
  const dim3 grid((unsigned)((units + kUnpackBlock - 1) / kUnpackBlock), (unsigned)f.n_frames);
  switch (f.format) {
    case PIX_RGB: launch<PIX_RGB>(a, grid, units_x, units, in_wide, out_align); break;
    case PIX_L: launch<PIX_L>(a, grid, units_x, units, in_wide, out_align); break;
    case PIX_BGR: launch<PIX_BGR>(a, grid, units_x, units, in_wide, out_align); break;
    case PIX_NV12: launch<PIX_NV12>(a, grid, units_x, units, in_wide, out_align); break;
    case PIX_I420: launch<PIX_I420>(a, grid, units_x, units, in_wide, out_align); break;
    default: launch<PIX_YUYV>(a, grid, units_x, units, in_wide, out_align); break;
  }
  return hipGetLastError();
}

}  // namespace bnn
