// Device half of windows_to_cifar / classify_windows (see windows.h): one launch turns all windows of one size into
// CIFAR-10 records (or their bare 3072-byte bodies).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "windows.h"

namespace bnn {

struct WindowLaunch {
  const uint8_t *scene;  // height x width x bands, rows `stride` bytes apart (device; RGBA: stride a multiple of 4); read only
  long stride;
  int bands;             // 1 (L), 3 (RGB) or 4 (RGBA)
  const int32_t *boxes;  // all windows of the call, 4 ints each (left, upper, right, lower), 16-byte aligned (device)
  const int32_t *order;  // this group's windows: indices into boxes, one per block (device)
  int w, h;              // the group's window size; h x out_w x bands <= kWindowMidBytes when `horizontal`
  int out_w, out_h;      // 1..32 each
  int horizontal, vertical;  // the passes Pillow runs (out_w != w, out_h != h)
  const int32_t *kh, *bh;    // horizontal coefficients [out_w][ksize_h], bounds [out_w][2] (device)
  int ksize_h;
  const int32_t *kv, *bv;    // vertical
  int ksize_v;
  uint8_t *out;          // record i of the CALL (not of the group) at out + i * out_pitch
  long out_pitch;        // 3073 with `label`; without, a multiple of 4 (3072) and `out` 16-byte aligned
  int label;             // 1: label byte 1, then the planes; 0: the planes alone
};

hipError_t launch_windows_to_cifar(const WindowLaunch &a, int n_windows, hipStream_t s);

}  // namespace bnn
