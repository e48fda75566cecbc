// window_kernels.hip -- windows of one scene -> CIFAR-10 records, one launch per window size (see windows.h).
//
// One block per window, both of Pillow's passes fused.  A window is small (the notebook's are 64 and 96 pixels wide:
// 13-19 taps per output sample), so -- unlike preprocess.hip, which spends a wave on one sample of a megapixel picture --
// a THREAD owns an output sample and loops over its taps.  The horizontal pass reads the shared scene in HBM at the
// window's origin plus the table's xmin (the tables are relative to the window), rounds to 8 bits like Pillow does
// between its passes and leaves h x out_w x bands bytes in LDS; after a barrier the vertical pass reads them from there,
// and the paste writes the planar record.  Arithmetic as in preprocess.hip: sums in uint32 that wrap, + 2^21, >> 22,
// clipped to 8 bits.  RGBA windows are premultiplied while they are LOADED (the scene is never modified: other groups
// and unresampled windows read it raw) and un-premultiplied in the paste.
#include "window_kernels.h"

namespace bnn {
namespace {

constexpr int kPrec = 22;
constexpr int kThreads = 256;

__device__ __forceinline__ uint8_t clip8(uint32_t ss) {
  const int v = (int)ss >> kPrec;
  return (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v);
}

// Pillow's rgbA2rgba on one colour byte: MULDIV255(c, a)
__device__ __forceinline__ uint32_t muldiv255(uint32_t c, uint32_t a) {
  const uint32_t t = c * a + 128;
  return (((t >> 8) + t) >> 8) & 0xFF;
}

// acc[b] += pixel[b] * k for the BANDS bytes at p (RGBA: one aligned dword, premultiplied on the way in when asked for)
template <int BANDS>
__device__ __forceinline__ void tap(uint32_t (&acc)[BANDS], const uint8_t *__restrict__ p, uint32_t k, bool premultiply) {
  if constexpr (BANDS == 4) {
    const uint32_t v = *reinterpret_cast<const uint32_t *>(p);  // (the scene is packed on the device: pixels are dword aligned)
    const uint32_t a = v >> 24;
#pragma unroll
    for (int b = 0; b < 3; b++) {
      const uint32_t c = (v >> (8 * b)) & 0xFF;
      acc[b] += (premultiply ? muldiv255(c, a) : c) * k;
    }
    acc[3] += a * k;
  } else {
#pragma unroll
    for (int b = 0; b < BANDS; b++) acc[b] += (uint32_t)p[b] * k;
  }
}

template <int BANDS>
__global__ __launch_bounds__(kThreads) void k_windows_to_cifar(const WindowLaunch a) {
  __shared__ __attribute__((aligned(16))) uint8_t mid[kWindowMidBytes];  // the horizontal pass's output, h x out_w x BANDS
  __shared__ __attribute__((aligned(16))) uint8_t fin[kWindowOutBytes];  // the resampled window, out_h x out_w x BANDS
  const int t = threadIdx.x;
  const int widx = a.order[blockIdx.x];  // the caller's number of this block's window: where its record goes
  const int4 box = reinterpret_cast<const int4 *>(a.boxes)[widx];
  const int out_w = a.out_w, out_h = a.out_h;
  const bool premultiplied = BANDS == 4 && (a.horizontal || a.vertical);
  const uint8_t *__restrict__ origin = a.scene + (size_t)box.y * a.stride + (size_t)box.x * BANDS;

  if (a.horizontal) {
    // mid[y][xx][b] = clip8(2^21 + sum_x window[y][xmin + x][b] * k[xx][x]) for all h rows of the window
    const int n = a.h * out_w;
    for (int i = t; i < n; i += kThreads) {
      const int y = i / out_w, xx = i - y * out_w;
      const int xmin = a.bh[2 * xx], taps = a.bh[2 * xx + 1];
      const int32_t *__restrict__ k = a.kh + (size_t)xx * a.ksize_h;
      const uint8_t *__restrict__ p = origin + (size_t)y * a.stride + (size_t)xmin * BANDS;
      uint32_t acc[BANDS];
#pragma unroll
      for (int b = 0; b < BANDS; b++) acc[b] = 1u << (kPrec - 1);
      for (int x = 0; x < taps; x++) tap<BANDS>(acc, p + (size_t)x * BANDS, (uint32_t)k[x], premultiplied);
#pragma unroll
      for (int b = 0; b < BANDS; b++) mid[(size_t)i * BANDS + b] = clip8(acc[b]);
    }
    __syncthreads();
  }
  {
    // fin[yy][xx][b]: the vertical pass over mid (or over the scene itself when no horizontal pass ran: out_w == w), or
    // a copy when the height stays
    const int n = out_h * out_w;
    for (int i = t; i < n; i += kThreads) {
      const int yy = i / out_w, xx = i - yy * out_w;
      uint32_t acc[BANDS];
      if (a.vertical) {
        const int ymin = a.bv[2 * yy], taps = a.bv[2 * yy + 1];
        const int32_t *__restrict__ k = a.kv + (size_t)yy * a.ksize_v;
#pragma unroll
        for (int b = 0; b < BANDS; b++) acc[b] = 1u << (kPrec - 1);
        if (a.horizontal) {
          const uint8_t *p = mid + ((size_t)ymin * out_w + xx) * BANDS;
          for (int y = 0; y < taps; y++) tap<BANDS>(acc, p + (size_t)y * out_w * BANDS, (uint32_t)k[y], false);
        } else {
          const uint8_t *__restrict__ p = origin + (size_t)ymin * a.stride + (size_t)xx * BANDS;
          for (int y = 0; y < taps; y++) tap<BANDS>(acc, p + (size_t)y * a.stride, (uint32_t)k[y], premultiplied);
        }
#pragma unroll
        for (int b = 0; b < BANDS; b++) fin[(size_t)i * BANDS + b] = clip8(acc[b]);
      } else if (a.horizontal) {
#pragma unroll
        for (int b = 0; b < BANDS; b++) fin[(size_t)i * BANDS + b] = mid[(size_t)i * BANDS + b];
      } else {  // the window fits: pasted as it is (RGBA: raw, never premultiplied)
        const uint8_t *__restrict__ p = origin + (size_t)yy * a.stride + (size_t)xx * BANDS;
#pragma unroll
        for (int b = 0; b < BANDS; b++) fin[(size_t)i * BANDS + b] = p[b];
      }
    }
    __syncthreads();
  }
  // paste centred on the canvas (255, 255, 255, 0) and write the planes; alpha is not part of the record
  const int off_x = (32 - out_w) / 2, off_y = (32 - out_h) / 2;  // int((32 - size) / 2), size <= 32
  uint8_t *__restrict__ rec = a.out + (size_t)widx * a.out_pitch;
  if (a.label && t == 0) *rec = 1;  // the label byte the reference writes (np.identity(1))
  uint8_t *__restrict__ body = rec + (a.label ? 1 : 0);
  for (int q = t; q < 3072 / 4; q += kThreads) {  // four consecutive canvas columns of one plane per thread
    const int ch = q >> 8, cy = (q >> 3) & 31, cx0 = (q & 7) * 4;
    const int yy = cy - off_y;
    uint32_t four = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int xx = cx0 + j - off_x;
      uint32_t v = 255;
      if (yy >= 0 && yy < out_h && xx >= 0 && xx < out_w) {
        const uint8_t *px = fin + ((size_t)yy * out_w + xx) * BANDS;
        v = px[BANDS >= 3 ? ch : 0];
        if constexpr (BANDS == 4) {
          // back from premultiplied alpha (Pillow's rgba2rgbA): copied when alpha is 0 or 255, else 255 c / a clipped
          const uint32_t al = px[3];
          if (premultiplied && al != 255 && al != 0) {
            const uint32_t d = (255u * v) / al;
            v = d > 255 ? 255 : d;
          }
        }
      }
      four |= v << (8 * j);
    }
    if (a.label) {  // a record's body starts at an odd byte
#pragma unroll
      for (int j = 0; j < 4; j++) body[4 * q + j] = (uint8_t)(four >> (8 * j));
    } else {  // bodies alone: out is 16-byte aligned and the pitch a multiple of 4
      reinterpret_cast<uint32_t *>(body)[q] = four;
    }
  }
}

}  // namespace

hipError_t launch_windows_to_cifar(const WindowLaunch &a, int n_windows, hipStream_t s) {
  if (n_windows <= 0) return hipSuccess;
  const dim3 grid((unsigned)n_windows), block(kThreads);
  if (a.bands == 3) hipLaunchKernelGGL(k_windows_to_cifar<3>, grid, block, 0, s, a);
  else if (a.bands == 4) hipLaunchKernelGGL(k_windows_to_cifar<4>, grid, block, 0, s, a);
  else hipLaunchKernelGGL(k_windows_to_cifar<1>, grid, block, 0, s, a);
  return hipGetLastError();
}

}  // namespace bnn
