// Stand-alone driver for tests/test_host_sanitize_windows.py: the host-only planning code of windows_to_cifar /
// classify_windows (csrc/windows.cpp on top of csrc/resample.cpp) under AddressSanitizer + UBSan.  tile_boxes with every
// cap, validation of boxes on and off all four edges, grouping and the permutation back to the caller's order on one
// window, all-equal boxes, 10^5 boxes and mixed sizes, the route decision on both sides of the LDS budget.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "resample.h"
#include "windows.h"

using namespace bnn;

#define CHECK(x) do { if (!(x)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

// every window exactly once, grouped by size, the caller's order kept inside a group, tables inside `coef`
static int check_plan(const std::vector<int> &boxes, int bands) {
  const int n = (int)boxes.size() / 4;
  WindowPlan plan;
  plan_windows(boxes.data(), n, bands, plan);
  CHECK((int)plan.order.size() == n);
  std::vector<int> seen((size_t)n, 0);
  int covered = 0;
  std::pair<int, int> last(0, 0);
  for (const WindowGroup &g : plan.groups) {
    CHECK(g.count > 0 && g.first == covered);
    CHECK(std::make_pair(g.w, g.h) > last);  // ascending, each size once
    last = std::make_pair(g.w, g.h);
    for (int k = g.first; k < g.first + g.count; k++) {
      const int i = plan.order[(size_t)k];
      CHECK(i >= 0 && i < n && !seen[(size_t)i]++);
      CHECK(boxes[4 * (size_t)i + 2] - boxes[4 * (size_t)i] == g.w && boxes[4 * (size_t)i + 3] - boxes[4 * (size_t)i + 1] == g.h);
      if (k > g.first) CHECK(plan.order[(size_t)k - 1] < i);
    }
    covered += g.count;
    CHECK(g.out_w >= 1 && g.out_w <= 32 && g.out_h >= 1 && g.out_h <= 32);
    CHECK(g.horizontal == (g.out_w != g.w) && g.vertical == (g.out_h != g.h));
    CHECK(g.fused == window_fused(g.w, g.h, bands));
    if (g.fused && g.horizontal) CHECK((size_t)g.h * g.out_w * bands <= (size_t)kWindowMidBytes);
    if (g.fused) CHECK(!vertical_pass_first(g.w, g.h, g.out_h));
    if (g.horizontal || g.vertical) {
      CHECK(g.off_bh == g.off_kh + (size_t)g.out_w * g.ksize_h && g.off_kv == g.off_bh + 2 * (size_t)g.out_w);
      CHECK(g.off_bv == g.off_kv + (size_t)g.out_h * g.ksize_v && g.off_bv + 2 * (size_t)g.out_h <= plan.coef.size());
      for (int xx = 0; xx < g.out_w; xx++) {  // what the kernel reads: inside the window
        const int xmin = plan.coef[g.off_bh + 2 * (size_t)xx], taps = plan.coef[g.off_bh + 2 * (size_t)xx + 1];
        CHECK(xmin >= 0 && taps >= 0 && taps <= g.ksize_h && xmin + taps <= g.w);
      }
      for (int yy = 0; yy < g.out_h; yy++) {
        const int ymin = plan.coef[g.off_bv + 2 * (size_t)yy], taps = plan.coef[g.off_bv + 2 * (size_t)yy + 1];
        CHECK(ymin >= 0 && taps >= 0 && taps <= g.ksize_v && ymin + taps <= g.h);
      }
    }
  }
  CHECK(covered == n);
  return 0;
}

int main() {
  // tile_boxes: the count whatever the cap, never more than cap boxes written
  {
    CHECK(tile_boxes(640, 480, 64, nullptr, 0) == 962 && tile_boxes(640, 480, 96, nullptr, 0) == 368);
    for (long cap : {0L, 1L, 7L, 962L, 2000L}) {
      std::vector<int> b((size_t)cap * 4);
      CHECK(tile_boxes(640, 480, 64, b.data(), cap) == 962);
      for (long i = 0; i < std::min(cap, 962L); i++) CHECK(b[4 * i + 2] - b[4 * i] == 64 && b[4 * i + 2] <= 640 && b[4 * i + 3] < 480);
    }
    CHECK(tile_boxes(640, 480, 3, nullptr, 0) == -1 && tile_boxes(640, 480, -5, nullptr, 0) == -1 && tile_boxes(0, 480, 64, nullptr, 0) == -1);
    CHECK(tile_boxes(1, 1, 4, nullptr, 0) == 0 && tile_boxes(65535, 65535, 65532, nullptr, 0) == 1);
    for (int w = 1; w <= 40; w++)
      for (int h = 1; h <= 40; h++)
        for (int size : {4, 5, 9, 31, 32}) {
          std::vector<int> b((size_t)w * h * 4 + 4, -1);
          const long n = tile_boxes(w, h, size, b.data(), (long)w * h);
          CHECK(n >= 0 && n <= (long)w * h && b[(size_t)w * h * 4] == -1);
        }
  }
  // validation: boxes on all four edges pass, one pixel further they do not, and the message names the box
  {
    const int W = 50, H = 40;
    uint8_t px = 0, out = 0;
    const std::vector<int> on_edges = {0, 0, 50, 40, 0, 0, 1, 1, 49, 39, 50, 40, 0, 5, 7, 40, 45, 0, 50, 9, 0, 39, 50, 40, 49, 0, 50, 40};
    CHECK(validate_windows("t", &px, W, H, 3, 0, on_edges.data(), (int)on_edges.size() / 4, &out).empty());
    const int bad[][4] = {{-1, 0, 5, 5}, {0, -1, 5, 5}, {46, 0, 51, 5}, {0, 36, 5, 41}, {5, 5, 5, 9}, {5, 5, 9, 5}, {9, 5, 5, 9}, {5, 9, 9, 5},
                          {2147483647, 0, -2147483647 - 1, 5}};
    for (const auto &b : bad)
      for (int pos : {0, 3}) {
        std::vector<int> boxes;
        for (int k = 0; k < pos; k++) boxes.insert(boxes.end(), {0, 0, 50, 40});
        boxes.insert(boxes.end(), b, b + 4);
        const std::string e = validate_windows("t", &px, W, H, 3, 0, boxes.data(), pos + 1, &out);
        CHECK(e.find("box " + std::to_string(pos) + " ") != std::string::npos);
      }
    CHECK(!validate_windows("t", &px, W, H, 2, 0, on_edges.data(), 1, &out).empty());
    CHECK(!validate_windows("t", &px, W, H, 3, 149, on_edges.data(), 1, &out).empty());
    CHECK(validate_windows("t", &px, W, H, 3, 150, on_edges.data(), 1, &out).empty());
    CHECK(!validate_windows("t", nullptr, W, H, 3, 0, on_edges.data(), 1, &out).empty());
    CHECK(!validate_windows("t", &px, W, H, 3, 0, nullptr, 1, &out).empty());
    CHECK(!validate_windows("t", &px, W, H, 3, 0, on_edges.data(), 1, nullptr).empty());
    CHECK(!validate_windows("t", &px, W, H, 3, 0, on_edges.data(), -1, &out).empty());
    CHECK(validate_windows("t", nullptr, 0, 0, 0, 0, nullptr, 0, nullptr).empty());
    CHECK(!validate_windows("t", &px, 65536, H, 3, 0, on_edges.data(), 1, &out).empty());
  }
  // grouping and the permutation
  {
    CHECK(check_plan({}, 3) == 0);
    CHECK(check_plan({3, 4, 67, 68}, 3) == 0);  // one window
    CHECK(check_plan({0, 0, 1, 1}, 1) == 0);    // the smallest there is
    std::vector<int> same;
    for (int i = 0; i < 1000; i++) same.insert(same.end(), {16, 16, 80, 80});  // all-equal boxes
    CHECK(check_plan(same, 4) == 0);
    std::vector<int> many;  // 10^5 boxes of 97 sizes, shuffled by a multiplicative walk
    for (int i = 0; i < 100000; i++) {
      const int k = (int)(((long)i * 7919) % 100000);
      const int w = 1 + k % 97, h = 1 + (k / 97) % 89, x = k % 13, y = k % 11;
      many.insert(many.end(), {x, y, x + w, y + h});
    }
    CHECK(check_plan(many, 3) == 0);
    // the routes: both sides of the LDS budget for 3 and 4 bands, vertical pass first, windows that fit
    std::vector<int> routes = {0, 0, 341, 341, 0, 0, 342, 342, 0, 0, 256, 256, 0, 0, 257, 257, 0, 0, 2, 201, 0, 0, 7, 701,
                               0, 0, 32, 32, 0, 0, 31, 32, 0, 0, 5, 7, 0, 0, 1, 64, 0, 0, 40, 20, 0, 0, 20, 40, 0, 0, 65535, 65535,
                               0, 0, 65535, 1, 0, 0, 1, 65535};
    CHECK(check_plan(routes, 3) == 0 && check_plan(routes, 4) == 0 && check_plan(routes, 1) == 0);
    CHECK(window_fused(341, 341, 3) && !window_fused(342, 342, 3) && window_fused(256, 256, 4) && !window_fused(257, 257, 4));
    CHECK(window_fused(1024, 1024, 1) && !window_fused(1025, 1025, 1));
    CHECK(!window_fused(2, 201, 3) && !window_fused(7, 701, 3) && window_fused(2, 200, 3) && window_fused(32, 32, 4) && window_fused(1, 64, 3));
  }
  std::printf("windows sanitize run ok\n");
  return 0;
}
