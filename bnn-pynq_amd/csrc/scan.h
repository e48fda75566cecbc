// Host half of the dense scan (bnn_mi355x_scan_*): every 32 x 32 window of a picture at stride 4, classified from ONE
// pass over the whole picture.  All convolutions of the CNV nets are "valid" 3 x 3 and the two pools are 2 x 2, so the
// network is fully convolutional up to layer 5: the layer-5 pixel (i, j) of the picture holds exactly the 256 bits the
// per-window pass computes for the record cut at columns 4i .. 4i + 31, rows 4j .. 4j + 31 ("Dense scan":
// the pool cells lie on even global coordinates and every window offset is a multiple of 4, so each window sees the
// global pool grid as its own).  Layers 6-8 and the decode then run on nx * ny "images" as they always do.
//
// This file is host-only (no HIP): the grid rule, the sizes of the six maps, the level and box rule of a multi-level
// call, validation and limits.  csrc/scan_kernels.hip holds the kernels, csrc/runtime.hip the entry points.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace bnn {

// Limits (include/bnn_mi355x.h states them): a side of a picture or of a level; the windows of one level; the bytes of
// the two activation buffers of one level.  Checked before anything touches the GPU; every index of the kernels fits an
// int below them (the largest map, layer 0's at 8 bytes a pixel, has fewer than 2^24 pixels).
constexpr int kScanMaxSide = 8192;
constexpr long kScanMaxWindows = 1L << 20;
constexpr size_t kScanMaxMapBytes = (size_t)1 << 27;

constexpr int kScanWindow = 32, kScanStride = 4, kScanStages = 6;

// nx = (width - 32) / 4 + 1, ny alike; false for a side below 32
bool scan_grid(int width, int height, int *nx, int *ny);

// The maps of one picture.  Only the used extent (wu x hu, up to 3 columns and rows less than the picture) is read.
//   stage   0 (L0)   1 (L1 + pool)   2 (L2)   3 (L3 + pool)   4 (L4)   5 (L5)
//   width   wu - 2   14 + 2 (nx-1)   .. - 2   5 + (nx - 1)    .. - 2   nx
//   dwords  2        2               4        4               8        8        per pixel (bit-packed HWC)
// Even stages lie in buffer 0, odd ones in buffer 1; layers 6 and 7 (64 bytes per window) ping-pong in the same two.
struct ScanPlan {
  int nx = 0, ny = 0, wu = 0, hu = 0;
  int w[kScanStages] = {}, h[kScanStages] = {};
  size_t buf0 = 0, buf1 = 0;  // bytes
};
constexpr int kScanStageDwords[kScanStages] = {2, 2, 4, 4, 8, 8};
inline size_t scan_stage_bytes(const ScanPlan &p, int stage) { return (size_t)p.w[stage] * p.h[stage] * kScanStageDwords[stage] * 4; }

// Empty when a width x height picture can be scanned, else the message for last_error (`what`: the entry point's name)
std::string plan_scan(const char *what, int width, int height, ScanPlan &plan);

// One level of a multi-level call, for a window size s (8 <= s, a multiple of 8): the picture is resized to
//   level_w = width * 32 / s, level_h = height * 32 / s     (integer division; refused below 32)
// and scanned; cell (i, j) of that scan is the window
//   (i s / 8, j s / 8, i s / 8 + s, j s / 8 + s)            in the picture's coordinates
// (a step of 4 level pixels is s / 8 picture pixels).  Such a box lies inside the picture: i <= (level_w - 32) / 4, so
// i s / 8 + s <= (level_w - 32) s / 32 + s = level_w s / 32 <= width.  The rule is this project's own.
bool scan_level(int width, int height, int size, int *level_w, int *level_h);
// Returns the number of boxes of that level (raster order, rows outer) and writes the first `cap` of them, 4 ints each;
// -1 when the size or the level is refused (scan_level)
long scan_boxes(int width, int height, int size, int *boxes, long cap);

// A multi-level call: validated, with every level's plan.  Empty string when acceptable.
struct ScanLevel {
  int size = 0, level_w = 0, level_h = 0;
  bool resized = false;  // level != picture: the two Lanczos passes run
  ScanPlan plan;
  long first = 0;        // its windows in the call's result: [first, first + nx * ny)
};
struct ScenePlan {
  std::vector<ScanLevel> levels;
  long windows = 0;
};
// Refused: null pointers, bands other than 1 / 3, a row stride shorter than a row (0 = packed rows), a picture or a level
// outside the limits, a bad size, n_sizes < 1
std::string plan_scene(const char *what, const void *pixels, int width, int height, int bands, long row_stride, const int *sizes, int n_sizes,
                       const void *boxes_out, ScenePlan &plan);

}  // namespace bnn
