// Device half of the dense scan (see scan.h): layers 0-5 of cnvW1A1 over a whole picture, and the two-pass Lanczos
// resize that makes a pyramid level of it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "scan.h"

namespace bnn {

constexpr int kScanLdsBytes = 0;  // none of the kernels uses LDS

struct ScanLaunch {
  const uint8_t *planes;  // device, planar uint8 [3][height][width]: plane c, row y at planes + c * plane_stride + y * row_stride
  long row_stride, plane_stride;
  ScanPlan plan;          // plan_scan of the picture (only plan.wu x plan.hu of it is read)
  void *buf0, *buf1;      // device, plan.buf0 / plan.buf1 bytes, 16-byte aligned
  const uint32_t *rows[6];  // device, the packed rows of layers 0-5 (packed_params.h)
  hipStream_t stream;
  int last_stage;         // run stages 0..last_stage only (bnn_mi355x_debug_scan_stage); kScanStages - 1 = all
};
// Enqueues the stages; stage s leaves its map [h][w][dwords] (scan.h) in buf(s & 1).  The layer-5 map in buf1 is the
// stage-5 output of plan.nx * plan.ny images in the layout of the per-image pass: run_cnv with first_stage = 6 goes on.
hipError_t run_scan(const ScanLaunch &a);

// Image.resize((out_w, out_h), Image.LANCZOS) of an 8-bit picture, Pillow's fixed-point passes (resample.h), written as
// planar [3][out_h][out_w] (bands == 1: the grey plane three times).  A pass whose size does not change is skipped, as
// Pillow skips it; with neither the picture is only re-laid out.
struct ScanResize {
  const uint8_t *src;  // device, h x w x bands, rows `stride` bytes apart; read only
  int w, h, bands;     // bands: 1 (L) or 3 (RGB)
  long stride;
  int out_w, out_h;
  bool vertical_first;     // resample.h, vertical_pass_first
  const int32_t *kh, *bh;  // horizontal coefficients [out_w][ksize_h], bounds [out_w][2] (device)
  int ksize_h;
  const int32_t *kv, *bv;  // vertical
  int ksize_v;
  uint8_t *tmp;        // device, max(h x out_w, out_h x w) x bands bytes: the first pass's output
  uint8_t *planes;     // device, 3 x out_h x out_w bytes
};
hipError_t launch_scan_resize(const ScanResize &j, hipStream_t s);

}  // namespace bnn
