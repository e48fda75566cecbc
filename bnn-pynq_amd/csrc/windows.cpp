// see windows.h
#include "windows.h"

#include <algorithm>
#include <numeric>

#include "resample.h"

namespace bnn {

long tile_boxes(int width, int height, int size, int *boxes, long cap) {
  if (size < 4 || width < 1 || height < 1) return -1;
  const int stride = size / 4;
  const int x_tiles = width / stride, y_tiles = height / stride;
  long n = 0;
  for (int j = 0; j < y_tiles; j++) {
    const long upper = (long)stride * j, lower = upper + size;
    if (!(lower < height)) break;  // (strict, like the notebook; rows further down only get lower)
    for (int i = 0; i < x_tiles; i++) {
      const long left = (long)stride * i, right = left + size;
      if (!(right <= width)) break;
      if (boxes && n < cap) {
        int *b = boxes + 4 * n;
        b[0] = (int)left; b[1] = (int)upper; b[2] = (int)right; b[3] = (int)lower;
      }
      n++;
    }
  }
  return n;
}

std::string validate_windows(const char *what, const void *pixels, int width, int height, int bands, long row_stride, const int *boxes,
                             int n_windows, const void *out) {
  const std::string name = std::string(what) + ": ";
  if (n_windows < 0) return name + "negative number of windows";
  if (n_windows == 0) return "";
  if (!pixels || !boxes || !out) return name + "bad arguments (null pointer with " + std::to_string(n_windows) + " windows)";
  if (bands != 1 && bands != 3 && bands != 4) return name + "bands must be 1 (L), 3 (RGB) or 4 (RGBA) bytes per pixel";
  if (width < 1 || height < 1 || width > 65535 || height > 65535) return name + "need a picture of 1..65535 x 1..65535 pixels";
  if (row_stride != 0 && row_stride < (long)width * bands) return name + "row stride shorter than a row";
  for (int i = 0; i < n_windows; i++) {
    const int *b = boxes + 4 * (size_t)i;
    const std::string box = "box " + std::to_string(i) + " (" + std::to_string(b[0]) + ", " + std::to_string(b[1]) + ", " +
                            std::to_string(b[2]) + ", " + std::to_string(b[3]) + ")";
    if (b[2] <= b[0] || b[3] <= b[1]) return name + box + " is empty or inverted (need right > left and lower > upper)";
    if (b[0] < 0 || b[1] < 0 || b[2] > width || b[3] > height)
      return name + box + " leaves the " + std::to_string(width) + " x " + std::to_string(height) + " picture";
  }
  return "";
}

bool window_fused(int w, int h, int bands) {
  int ow = w, oh = h;
  (void)thumbnail_size(w, h, 32, &ow, &oh);
  if (vertical_pass_first(w, h, oh)) return false;
  return ow == w || (size_t)h * ow * bands <= (size_t)kWindowMidBytes;
}

void plan_windows(const int *boxes, int n_windows, int bands, WindowPlan &plan) {
  plan.groups.clear();
  plan.coef.clear();
  plan.order.resize((size_t)(n_windows > 0 ? n_windows : 0));
  std::iota(plan.order.begin(), plan.order.end(), 0);
  auto size_of = [&](int i) { return std::pair<int, int>(boxes[4 * (size_t)i + 2] - boxes[4 * (size_t)i], boxes[4 * (size_t)i + 3] - boxes[4 * (size_t)i + 1]); };
  std::stable_sort(plan.order.begin(), plan.order.end(), [&](int a, int b) { return size_of(a) < size_of(b); });
  for (int k = 0; k < n_windows;) {
    const std::pair<int, int> wh = size_of(plan.order[(size_t)k]);
    WindowGroup g;
    g.w = wh.first; g.h = wh.second;
    g.out_w = g.w; g.out_h = g.h;
    (void)thumbnail_size(g.w, g.h, 32, &g.out_w, &g.out_h);
    g.horizontal = g.out_w != g.w;
    g.vertical = g.out_h != g.h;
    g.fused = window_fused(g.w, g.h, bands);
    g.first = k;
    while (k < n_windows && size_of(plan.order[(size_t)k]) == wh) k++;
    g.count = k - g.first;
    if (g.horizontal || g.vertical) {  // (a window that fits is pasted as it is: no tables)
      std::vector<int32_t> kh, bh, kv, bv;
      g.ksize_h = lanczos_coeffs(g.w, g.out_w, kh, bh);
      g.ksize_v = lanczos_coeffs(g.h, g.out_h, kv, bv);
      g.off_kh = plan.coef.size();
      g.off_bh = g.off_kh + kh.size();
      g.off_kv = g.off_bh + bh.size();
      g.off_bv = g.off_kv + kv.size();
      plan.coef.insert(plan.coef.end(), kh.begin(), kh.end());
      plan.coef.insert(plan.coef.end(), bh.begin(), bh.end());
      plan.coef.insert(plan.coef.end(), kv.begin(), kv.end());
      plan.coef.insert(plan.coef.end(), bv.begin(), bv.end());
    }
    plan.groups.push_back(g);
  }
}

}  // namespace bnn
