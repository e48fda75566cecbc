// Host half of bnn_mi355x_windows_to_cifar / bnn_mi355x_classify_windows: every window (`Image.crop` box) of ONE scene
// becomes a CIFAR-10 record on the device.  The reference does this in CNV-BNN_Road-Signs.ipynb cells 13-16 ("Locate
// objects within a scene"): it tiles a street picture into overlapping windows of sizes 64 and 96 (stride size // 4),
// crops each one and classifies the crops.  crop + thumbnail depends on the window's SIZE alone, so all windows of one
// (w, h) share one pair of Lanczos tables (resample.h) and go to the device as one launch.
//
// This file is host-only (no HIP): the tiling rule, the validation of the caller's boxes, the grouping by size with the
// permutation back to the caller's order, the route each group takes and its coefficient tables.  csrc/window_kernels.hip
// holds the kernel, csrc/runtime.hip the entry points.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace bnn {

// LDS budget of the fused window kernel: the horizontal pass's 8-bit output, h x out_w x bands bytes (6 KB for a 64-pixel
// RGB window, 9 KB for 96), stays in LDS for the vertical pass.  Windows whose intermediate is larger take the
// one-by-one route (launch_image_to_cifar on a packed copy of the window).  Well below the 64 KB a block may ask for.
constexpr int kWindowMidBytes = 32768;
// ... plus the resampled window itself (out_h x out_w x bands <= 32 x 32 x 4), from which the paste reads
constexpr int kWindowOutBytes = 4096;
constexpr int kWindowLdsBytes = kWindowMidBytes + kWindowOutBytes;

// The notebook's tiling rule for one window size (cell 13):
//   stride = size // 4; x_tiles = width // stride; y_tiles = height // stride
//   for j in range(y_tiles): for i in range(x_tiles):
//     bound = (stride * i, stride * j, stride * i + size, stride * j + size)
//     if bound[2] <= width and bound[3] < height: keep
// The notebook is strict on the height and not on the width (a window may touch the right edge, not the lower one);
// reproduced as it is.  Returns the number of boxes and writes the first `cap` of them (4 ints each); -1 for size < 4
// (stride 0) or a non-positive picture.
long tile_boxes(int width, int height, int size, int *boxes, long cap);

// Empty when the call is acceptable, else the message for last_error (it names the first offending box).  `what` is
// the entry point's name.  Refused: bands not 1 / 3 / 4, a picture outside 1..65535 x 1..65535, a row stride shorter
// than a row (0 = packed rows), null pointers with n > 0, empty or inverted boxes, boxes that leave the picture (Pillow
// would pad them with zeros; the notebook filters them out, so they are not modelled).
std::string validate_windows(const char *what, const void *pixels, int width, int height, int bands, long row_stride, const int *boxes,
                             int n_windows, const void *out);

struct WindowGroup {
  int w = 0, h = 0;          // the windows' size
  int out_w = 0, out_h = 0;  // Image.thumbnail((32, 32)) of it (== w, h: pasted unresampled)
  bool horizontal = false, vertical = false;  // which passes Pillow runs
  bool fused = false;        // true: one launch of the window kernel for the whole group; false: one by one (see window_fused)
  int ksize_h = 0, ksize_v = 0;
  size_t off_kh = 0, off_bh = 0, off_kv = 0, off_bv = 0;  // this group's tables in WindowPlan::coef (int32 units)
  int first = 0, count = 0;  // its windows: WindowPlan::order[first .. first + count)
};

struct WindowPlan {
  std::vector<WindowGroup> groups;  // ascending (w, h)
  std::vector<int32_t> order;       // window indices in the caller's numbering, grouped; within a group in the caller's order
  std::vector<int32_t> coef;        // all groups' tables, one upload
};

// The route of a (w, h) window of `bands` bytes per pixel: the fused kernel unless its intermediate exceeds
// kWindowMidBytes or Pillow resamples it vertical pass first (resample.h: vertical_pass_first).
bool window_fused(int w, int h, int bands);

// Groups n validated boxes by size.  Record i of the result belongs to the caller's box i whatever the grouping: the
// kernels write record order[k] for the k-th window they are given.
void plan_windows(const int *boxes, int n_windows, int bands, WindowPlan &plan);

}  // namespace bnn
