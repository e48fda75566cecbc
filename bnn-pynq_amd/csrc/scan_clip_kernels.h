// Device half of the clip scan (see scan_clip.h): layers 0-5 of cnvW1A1 over ALL (frame, level) maps of a clip in one
// launch per stage, and the Lanczos resize of one level of all frames in one pair of launches.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "scan_clip.h"

namespace bnn {

constexpr int kScanClipLdsBytes = 0;  // none of the kernels uses LDS

struct ScanClipLaunch {
  const uint8_t *planes;    // device: every level's planar picture of every frame (ClipPlan::planes_bytes, ClipMap::planes)
  void *buf0, *buf1;        // device, ClipPlan::buf0 / buf1 bytes, 16-byte aligned
  const uint32_t *rows[6];  // device, the packed rows of layers 0-5 (packed_params.h)
  const int32_t *tables;    // device copy of ClipTables::words (8-byte aligned)
  size_t desc[kScanStages], block_map[kScanStages];  // ClipTables' offsets
  long blocks[kScanStages]; // ClipPlan::blocks
  hipStream_t stream;
  int last_stage;           // run stages 0..last_stage only (bnn_mi355x_debug_scan_clip_stage); kScanStages - 1 = all
};
// Enqueues one launch per stage; stage s leaves every map [h][w][dwords] at its offset (ClipMap::off) of buf(s & 1).  The
// layer-5 maps in buf1 are the stage-5 output of ClipPlan::windows images in result order: run_cnv with first_stage = 6
// goes on, once.
hipError_t run_scan_clip(const ScanClipLaunch &a);

// launch_scan_resize (scan_kernels.h) for `frames` pictures of one size at once: blockIdx.y is the frame, the frames
// share the level's tables.  Pass order, skipped passes and the re-layout of an unresized level are launch_scan_resize's:
// both launchers ask resize_route (scan_bodies.h) for the passes.
struct ScanClipResize {
  const uint8_t *src;  // device, frames x h x w x bands, rows `stride` bytes and frames `src_frame` bytes apart; read only
  int frames, w, h, bands;
  long stride, src_frame;
  int out_w, out_h;
  bool vertical_first;     // resample.h, vertical_pass_first
  const int32_t *kh, *bh;  // horizontal coefficients [out_w][ksize_h], bounds [out_w][2] (device)
  int ksize_h;
  const int32_t *kv, *bv;  // vertical
  int ksize_v;
  uint8_t *tmp;        // device, frames x tmp_frame bytes: the first pass's output
  long tmp_frame;      // max(h x out_w, out_h x w) x bands or more
  uint8_t *planes;     // device, frames x 3 x out_h x out_w bytes
};
hipError_t launch_clip_resize(const ScanClipResize &j, hipStream_t s);

}  // namespace bnn
