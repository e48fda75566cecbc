// scan_clip_kernels.hip -- the clip scan (scan_clip.h): the dense scan's stage kernels over all (frame, level) maps of a
// clip at once, and its resize kernels over all frames of a level at once.
//
// A stage is ONE launch: blockIdx.y stays the group of 32 neurons and blockIdx.x runs over the blocks of all maps, each
// map having ceil(items / 256) blocks of its own.  A block reads its map's number from the stage's block -> map table
// and the map's descriptor (ClipMapDesc: input and output offsets, widths, item count, first block) from the stage's
// descriptor table; both reads are wave-uniform and go through scalar loads, like the neuron rows.  Lanes past the
// map's item count return.  From there on a lane does exactly what it does in scan_kernels.hip: both files call the
// bodies of scan_bodies.h, and the order of the resize passes is that header's too.  No LDS, no scratch.
#include "scan_clip_kernels.h"
#include "scan_bodies.h"

namespace bnn {
namespace {

static_assert(kBlock == kScanClipBlock, "the model counts blocks of the size the kernels are launched with");

typedef const int32_t __attribute__((address_space(4))) *kptr_map;
typedef const ClipMapDesc __attribute__((address_space(4))) *kptr_desc;

// the block's map and its item; false for a lane past the map's items
__device__ __forceinline__ bool clip_item(const ClipMapDesc *__restrict__ descs, const int32_t *__restrict__ block_map, ClipMapDesc &d, int &item) {
  const int m = ((kptr_map)(uintptr_t)block_map)[blockIdx.x];
  const kptr_desc q = (kptr_desc)(uintptr_t)descs + m;
  d.in_off = q->in_off; d.out_off = q->out_off; d.row_stride = q->row_stride; d.plane_stride = q->plane_stride;
  d.iw = q->iw; d.ow = q->ow; d.n_items = q->n_items; d.first_block = q->first_block;
  item = ((int)blockIdx.x - d.first_block) * kBlock + (int)threadIdx.x;
  return item < d.n_items;
}

__global__ __launch_bounds__(kBlock) void k_clip_conv0(const uint8_t *__restrict__ planes, uint8_t *__restrict__ out, const uint32_t *__restrict__ rows,
                                                        const ClipMapDesc *__restrict__ descs, const int32_t *__restrict__ block_map) {
  ClipMapDesc d;
  int item;
  if (!clip_item(descs, block_map, d, item)) return;
  scan_conv0_item(planes + d.in_off, (long)d.row_stride, (long)d.plane_stride, reinterpret_cast<uint32_t *>(out + d.out_off), rows, d.ow, item,
                  blockIdx.y);
}

template <int CW, bool POOL>
__global__ __launch_bounds__(kBlock) void k_clip_quad(const uint8_t *__restrict__ in, uint8_t *__restrict__ out, const uint32_t *__restrict__ rows,
                                                       const ClipMapDesc *__restrict__ descs, const int32_t *__restrict__ block_map, int groups) {
  ClipMapDesc d;
  int item;
  if (!clip_item(descs, block_map, d, item)) return;
  scan_quad_item<CW, POOL>(reinterpret_cast<const uint64_t *>(in + d.in_off), reinterpret_cast<uint32_t *>(out + d.out_off), rows, d.iw, d.ow, item,
                           blockIdx.y, groups);
}

template <int CW>
__global__ __launch_bounds__(kBlock) void k_clip_vec(const uint8_t *__restrict__ in, uint8_t *__restrict__ out, const uint32_t *__restrict__ rows,
                                                      const ClipMapDesc *__restrict__ descs, const int32_t *__restrict__ block_map, int groups) {
  ClipMapDesc d;
  int item;
  if (!clip_item(descs, block_map, d, item)) return;
  // (the output base in vector registers: layer 5's neuron loop has no scalar registers to spare for it, and would
  // otherwise spill four of them)
  uint32_t *o = reinterpret_cast<uint32_t *>(out + d.out_off);
  asm("" : "+v"(o));
  scan_vec_item<CW>(reinterpret_cast<const uint64_t *>(in + d.in_off), o, rows, d.iw, d.ow, item, blockIdx.y, groups);
}

// ---- the resize passes, blockIdx.y the frame ------------------------------------------------------------------------------
template <int BANDS>
__global__ __launch_bounds__(kBlock) void k_clip_resize_h(const uint8_t *__restrict__ src, long pitch, long src_frame, int rows, int out_w,
                                                           const int32_t *__restrict__ kk, const int32_t *__restrict__ bounds, int ksize,
                                                           ResizeOut o, long out_frame) {
  const long idx = (long)blockIdx.x * kBlock + threadIdx.x;
  if (idx >= (long)rows * out_w) return;
  o.dst += (size_t)blockIdx.y * out_frame;
  resize_h_item<BANDS>(src + (size_t)blockIdx.y * src_frame, pitch, out_w, kk, bounds, ksize, o, idx);
}
template <int BANDS>
__global__ __launch_bounds__(kBlock) void k_clip_resize_v(const uint8_t *__restrict__ src, long pitch, long src_frame, int w, int out_h,
                                                           const int32_t *__restrict__ kk, const int32_t *__restrict__ bounds, int ksize,
                                                           int vertical, ResizeOut o, long out_frame) {
  const long idx = (long)blockIdx.x * kBlock + threadIdx.x;
  if (idx >= (long)out_h * w) return;
  o.dst += (size_t)blockIdx.y * out_frame;
  resize_v_item<BANDS>(src + (size_t)blockIdx.y * src_frame, pitch, w, kk, bounds, ksize, vertical, o, idx);
}

}  // namespace

hipError_t run_scan_clip(const ScanClipLaunch &a) {
  for (int l = 0; l <= a.last_stage && l < kScanStages; l++)
    if (a.blocks[l] < 1 || a.blocks[l] > INT32_MAX) return hipErrorInvalidValue;
  uint8_t *A = static_cast<uint8_t *>(a.buf0), *B = static_cast<uint8_t *>(a.buf1);
  hipStream_t s = a.stream;
  auto grid = [&](int stage, int groups) { return dim3((unsigned)a.blocks[stage], (unsigned)groups); };
  auto descs = [&](int stage) { return reinterpret_cast<const ClipMapDesc *>(a.tables + a.desc[stage]); };
  auto bmap = [&](int stage) { return a.tables + a.block_map[stage]; };
  if (a.last_stage >= 0) hipLaunchKernelGGL(k_clip_conv0, grid(0, 2), dim3(kBlock), 0, s, a.planes, A, a.rows[0], descs(0), bmap(0));
  if (a.last_stage >= 1) hipLaunchKernelGGL((k_clip_quad<1, true>), grid(1, 2), dim3(kBlock), 0, s, A, B, a.rows[1], descs(1), bmap(1), 2);
  if (a.last_stage >= 2) hipLaunchKernelGGL((k_clip_quad<1, false>), grid(2, 4), dim3(kBlock), 0, s, B, A, a.rows[2], descs(2), bmap(2), 4);
  if (a.last_stage >= 3) hipLaunchKernelGGL((k_clip_quad<2, true>), grid(3, 4), dim3(kBlock), 0, s, A, B, a.rows[3], descs(3), bmap(3), 4);
  if (a.last_stage >= 4) hipLaunchKernelGGL((k_clip_vec<2>), grid(4, 8), dim3(kBlock), 0, s, B, A, a.rows[4], descs(4), bmap(4), 8);
  if (a.last_stage >= 5) hipLaunchKernelGGL((k_clip_vec<4>), grid(5, 8), dim3(kBlock), 0, s, A, B, a.rows[5], descs(5), bmap(5), 8);
  return hipGetLastError();
}

hipError_t launch_clip_resize(const ScanClipResize &j, hipStream_t s) {
  if ((j.bands != 1 && j.bands != 3) || j.w < 1 || j.h < 1 || j.out_w < 1 || j.out_h < 1 || j.frames < 1 || j.frames > kScanClipMaxFrames)
    return hipErrorInvalidValue;
  const auto vertical = j.bands == 3 ? k_clip_resize_v<3> : k_clip_resize_v<1>;
  const auto horizontal = j.bands == 3 ? k_clip_resize_h<3> : k_clip_resize_h<1>;
  const ResizeRoute r = resize_route(j.w, j.h, j.bands, j.out_w, j.out_h, j.vertical_first, j.stride, j.tmp, j.planes);
  for (int i = 0; i < r.n; i++) {
    const ResizePass &p = r.pass[i];
    // the frame strides of a pass's source and of its output: tmp's, else the clip's and that of the three planes
    const uint8_t *src = p.from_tmp ? j.tmp : j.src;
    const long src_frame = p.from_tmp ? j.tmp_frame : j.src_frame, out_frame = p.o.dst == j.tmp ? j.tmp_frame : 3 * p.o.plane;
    dim3 grid = grid_of(p.items);
    grid.y = (unsigned)j.frames;
    if (p.horizontal) hipLaunchKernelGGL(horizontal, grid, dim3(kBlock), 0, s, src, p.pitch, src_frame, p.extent, p.out, j.kh, j.bh, j.ksize_h, p.o, out_frame);
    else hipLaunchKernelGGL(vertical, grid, dim3(kBlock), 0, s, src, p.pitch, src_frame, p.extent, p.out, j.kv, j.bv, j.ksize_v, p.vertical, p.o, out_frame);
  }
  return hipGetLastError();
}

}  // namespace bnn
