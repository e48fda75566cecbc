// Host half of the dense scan: see scan.h.
#include "scan.h"

#include <cassert>

namespace bnn {

bool scan_grid(int width, int height, int *nx, int *ny) {
  if (width < kScanWindow || height < kScanWindow) return false;
  if (nx) *nx = (width - kScanWindow) / kScanStride + 1;
  if (ny) *ny = (height - kScanWindow) / kScanStride + 1;
  return true;
}

namespace {

std::string dims(int w, int h) { return std::to_string(w) + " x " + std::to_string(h); }

// the six map sizes along one axis, from the used extent u = 32 + 4 (n - 1)
void axis_sizes(int u, int n, int (&s)[kScanStages]) {
  s[0] = u - 2;         // L0
  s[1] = (u - 4) / 2;   // L1 + pool: 14 + 2 (n - 1)
  s[2] = s[1] - 2;      // L2
  s[3] = (s[1] - 4) / 2;  // L3 + pool: 5 + (n - 1)
  s[4] = s[3] - 2;      // L4
  s[5] = s[3] - 4;      // L5
  assert(s[1] == 14 + 2 * (n - 1) && s[3] == 5 + (n - 1) && s[5] == n);
  assert((u - 4) % 2 == 0 && (s[1] - 4) % 2 == 0 && s[2] % 2 == 0);  // pooled layers (and L2): whole 2 x 2 quads
}

}  // namespace

std::string plan_scan(const char *what, int width, int height, ScanPlan &p) {
  const std::string name = std::string(what) + ": ";
  p = ScanPlan{};
  if (!scan_grid(width, height, &p.nx, &p.ny)) return name + "need a picture of 32 x 32 pixels or more (got " + dims(width, height) + ")";
  if (width > kScanMaxSide || height > kScanMaxSide)
    return name + "a " + dims(width, height) + " picture exceeds the limit of " + std::to_string(kScanMaxSide) + " pixels a side";
  if ((long)p.nx * p.ny > kScanMaxWindows)
    return name + "a " + dims(width, height) + " picture has " + std::to_string((long)p.nx * p.ny) + " windows, more than the limit of " +
           std::to_string(kScanMaxWindows);
  p.wu = kScanWindow + kScanStride * (p.nx - 1);
  p.hu = kScanWindow + kScanStride * (p.ny - 1);
  axis_sizes(p.wu, p.nx, p.w);
  axis_sizes(p.hu, p.ny, p.h);
  const size_t tail = (size_t)p.nx * p.ny * 64;  // layers 6 and 7: 512 bits per window
  for (int s = 0; s < kScanStages; s++) {
    size_t &b = (s & 1) ? p.buf1 : p.buf0;
    if (scan_stage_bytes(p, s) > b) b = scan_stage_bytes(p, s);
  }
  if (tail > p.buf0) p.buf0 = tail;
  if (tail > p.buf1) p.buf1 = tail;
  if (p.buf0 + p.buf1 > kScanMaxMapBytes)
    return name + "the maps of a " + dims(width, height) + " picture take " + std::to_string(p.buf0 + p.buf1) + " bytes, more than the limit of " +
           std::to_string(kScanMaxMapBytes);
  return "";
}

bool scan_level(int width, int height, int size, int *level_w, int *level_h) {
  if (size < 8 || size % 8 != 0 || width < 1 || height < 1) return false;
  const long lw = (long)width * kScanWindow / size, lh = (long)height * kScanWindow / size;
  if (lw < kScanWindow || lh < kScanWindow || lw > INT32_MAX || lh > INT32_MAX) return false;
  if (level_w) *level_w = (int)lw;
  if (level_h) *level_h = (int)lh;
  return true;
}

long scan_boxes(int width, int height, int size, int *boxes, long cap) {
  int lw = 0, lh = 0, nx = 0, ny = 0;
  if (!scan_level(width, height, size, &lw, &lh) || !scan_grid(lw, lh, &nx, &ny)) return -1;
  const int step = size / 8;
  long n = 0;
  for (int j = 0; j < ny; j++)
    for (int i = 0; i < nx; i++, n++) {
      const int l = i * step, u = j * step;
      assert(l + size <= width && u + size <= height);  // (scan.h: such boxes always lie inside the picture)
      if (boxes && n < cap) {
        int *b = boxes + 4 * n;
        b[0] = l; b[1] = u; b[2] = l + size; b[3] = u + size;
      }
    }
  return n;
}

std::string plan_scene(const char *what, const void *pixels, int width, int height, int bands, long row_stride, const int *sizes, int n_sizes,
                       const void *boxes_out, ScenePlan &plan) {
  const std::string name = std::string(what) + ": ";
  plan = ScenePlan{};
  if (n_sizes < 1) return name + "need one window size or more";
  if (!pixels || !sizes || !boxes_out) return name + "bad arguments (null pointer with " + std::to_string(n_sizes) + " window sizes)";
  if (bands != 1 && bands != 3) return name + "bands must be 1 (L) or 3 (RGB) bytes per pixel";
  if (width < kScanWindow || height < kScanWindow) return name + "need a picture of 32 x 32 pixels or more (got " + dims(width, height) + ")";
  if (width > kScanMaxSide || height > kScanMaxSide)
    return name + "a " + dims(width, height) + " picture exceeds the limit of " + std::to_string(kScanMaxSide) + " pixels a side";
  if (row_stride != 0 && row_stride < (long)width * bands) return name + "row stride shorter than a row";
  for (int k = 0; k < n_sizes; k++) {
    ScanLevel lv;
    lv.size = sizes[k];
    const std::string sz = "window size " + std::to_string(lv.size);
    if (lv.size < 8 || lv.size % 8 != 0) return name + sz + " is not a multiple of 8 (8 or more)";
    if (!scan_level(width, height, lv.size, &lv.level_w, &lv.level_h))
      return name + sz + " leaves a level below 32 x 32 pixels for a " + dims(width, height) + " picture";
    const std::string bad = plan_scan(what, lv.level_w, lv.level_h, lv.plan);
    if (!bad.empty()) return bad + " (the level of " + sz + ")";
    lv.resized = lv.level_w != width || lv.level_h != height;
    lv.first = plan.windows;
    plan.windows += (long)lv.plan.nx * lv.plan.ny;
    plan.levels.push_back(lv);
  }
  return "";
}

}  // namespace bnn
