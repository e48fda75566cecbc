// scan_kernels.hip -- the dense scan (scan.h): layers 0-5 of cnvW1A1 over a whole picture with runtime sizes, and the
// general Lanczos resize of a pyramid level.
//
// The shipped stage kernels (kernels.hip) are templated on the 32 x 32 geometry and address [image][pixel]; these take
// the map's width and height as arguments and address [row][column].  One map a launch: a lane's item is its global
// index, blockIdx.y the group of 32 neurons, and the item range's tail is guarded.  From there on a lane does what
// scan_bodies.h states (the mapping of DESIGN.md 5, the neuron loops, Pillow's two passes); the kernels of the other
// file that shares that header look their item up in a table first.  No LDS.
#include "scan_kernels.h"
#include "scan_bodies.h"

namespace bnn {
namespace {

// ---- layer 0: planar uint8 picture -> (ow x oh) x 64 thresholded map; item = oy * ow + ox ---------------------------------
__global__ __launch_bounds__(kBlock) void k_scan_conv0(const uint8_t *__restrict__ planes, long row_stride, long plane_stride,
                                                        uint32_t *__restrict__ out, const uint32_t *__restrict__ rows, int ow, int n_items) {
  const int item = blockIdx.x * kBlock + threadIdx.x, cg = blockIdx.y;
  if (item >= n_items) return;
  scan_conv0_item(planes, row_stride, plane_stride, out, rows, ow, item, cg);
}

// ---- layers 1-3: one lane = one 2 x 2 quad of conv outputs; item = qy * qw + qx ------------------------------------------
template <int CW, bool POOL>
__global__ __launch_bounds__(kBlock) void k_scan_quad(const uint64_t *__restrict__ in, uint32_t *__restrict__ out,
                                                       const uint32_t *__restrict__ rows, int iw, int qw, int n_items, int groups) {
  const int item = blockIdx.x * kBlock + threadIdx.x, cg = blockIdx.y;
  if (item >= n_items) return;
  scan_quad_item<CW, POOL>(in, out, rows, iw, qw, item, cg, groups);
}

// ---- layers 4 and 5: one lane = one output pixel; item = oy * ow + ox -----------------------------------------------------
template <int CW>
__global__ __launch_bounds__(kBlock) void k_scan_vec(const uint64_t *__restrict__ in, uint32_t *__restrict__ out,
                                                      const uint32_t *__restrict__ rows, int iw, int ow, int n_items, int groups) {
  const int item = blockIdx.x * kBlock + threadIdx.x, cg = blockIdx.y;
  if (item >= n_items) return;
  scan_vec_item<CW>(in, out, rows, iw, ow, item, cg, groups);
}

// ---- Image.resize(..., LANCZOS): Pillow's two 8-bit passes, one lane per output pixel ----------------------------------
template <int BANDS>
__global__ __launch_bounds__(kBlock) void k_scan_resize_h(const uint8_t *__restrict__ src, long pitch, int rows, int out_w,
                                                           const int32_t *__restrict__ kk, const int32_t *__restrict__ bounds, int ksize,
                                                           ResizeOut o) {
  const long idx = (long)blockIdx.x * kBlock + threadIdx.x;
  if (idx >= (long)rows * out_w) return;
  resize_h_item<BANDS>(src, pitch, out_w, kk, bounds, ksize, o, idx);
}
template <int BANDS>
__global__ __launch_bounds__(kBlock) void k_scan_resize_v(const uint8_t *__restrict__ src, long pitch, int w, int out_h,
                                                           const int32_t *__restrict__ kk, const int32_t *__restrict__ bounds, int ksize,
                                                           int vertical, ResizeOut o) {
  const long idx = (long)blockIdx.x * kBlock + threadIdx.x;
  if (idx >= (long)out_h * w) return;
  resize_v_item<BANDS>(src, pitch, w, kk, bounds, ksize, vertical, o, idx);
}

}  // namespace

hipError_t run_scan(const ScanLaunch &a) {
  const ScanPlan &p = a.plan;
  if (p.nx < 1 || p.ny < 1) return hipErrorInvalidValue;
  uint32_t *A = reinterpret_cast<uint32_t *>(a.buf0), *B = reinterpret_cast<uint32_t *>(a.buf1);
  const uint64_t *A64 = reinterpret_cast<const uint64_t *>(a.buf0), *B64 = reinterpret_cast<const uint64_t *>(a.buf1);
  hipStream_t s = a.stream;
  // work items of a stage: its output pixels, or its 2 x 2 quads of conv outputs (stage 2 too: its map is even)
  const int n0 = p.w[0] * p.h[0], q1 = p.w[1] * p.h[1], qw2 = p.w[2] / 2, q2 = qw2 * (p.h[2] / 2), q3 = p.w[3] * p.h[3], n4 = p.w[4] * p.h[4],
            n5 = p.w[5] * p.h[5];
  auto grid = [](int items, int groups) { dim3 g = grid_of(items); g.y = (unsigned)groups; return g; };
  if (a.last_stage >= 0) hipLaunchKernelGGL(k_scan_conv0, grid(n0, 2), dim3(kBlock), 0, s, a.planes, a.row_stride, a.plane_stride, A, a.rows[0], p.w[0], n0);
  if (a.last_stage >= 1) hipLaunchKernelGGL((k_scan_quad<1, true>), grid(q1, 2), dim3(kBlock), 0, s, A64, B, a.rows[1], p.w[0], p.w[1], q1, 2);
  if (a.last_stage >= 2) hipLaunchKernelGGL((k_scan_quad<1, false>), grid(q2, 4), dim3(kBlock), 0, s, B64, A, a.rows[2], p.w[1], qw2, q2, 4);
  if (a.last_stage >= 3) hipLaunchKernelGGL((k_scan_quad<2, true>), grid(q3, 4), dim3(kBlock), 0, s, A64, B, a.rows[3], p.w[2], p.w[3], q3, 4);
  if (a.last_stage >= 4) hipLaunchKernelGGL((k_scan_vec<2>), grid(n4, 8), dim3(kBlock), 0, s, B64, A, a.rows[4], p.w[3], p.w[4], n4, 8);
  if (a.last_stage >= 5) hipLaunchKernelGGL((k_scan_vec<4>), grid(n5, 8), dim3(kBlock), 0, s, A64, B, a.rows[5], p.w[4], p.w[5], n5, 8);
  return hipGetLastError();
}

hipError_t launch_scan_resize(const ScanResize &j, hipStream_t s) {
  if ((j.bands != 1 && j.bands != 3) || j.w < 1 || j.h < 1 || j.out_w < 1 || j.out_h < 1) return hipErrorInvalidValue;
  const auto vertical = j.bands == 3 ? k_scan_resize_v<3> : k_scan_resize_v<1>;
  const auto horizontal = j.bands == 3 ? k_scan_resize_h<3> : k_scan_resize_h<1>;
  const ResizeRoute r = resize_route(j.w, j.h, j.bands, j.out_w, j.out_h, j.vertical_first, j.stride, j.tmp, j.planes);
  for (int i = 0; i < r.n; i++) {
    const ResizePass &p = r.pass[i];
    const uint8_t *src = p.from_tmp ? j.tmp : j.src;
    if (p.horizontal) hipLaunchKernelGGL(horizontal, grid_of(p.items), dim3(kBlock), 0, s, src, p.pitch, p.extent, p.out, j.kh, j.bh, j.ksize_h, p.o);
    else hipLaunchKernelGGL(vertical, grid_of(p.items), dim3(kBlock), 0, s, src, p.pitch, p.extent, p.out, j.kv, j.bv, j.ksize_v, p.vertical, p.o);
  }
  return hipGetLastError();
}

}  // namespace bnn
