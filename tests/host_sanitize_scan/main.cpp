// Stand-alone driver for tests/test_host_sanitize_scan.py: the host-only code of the dense scan (csrc/scan.cpp: the grid,
// the maps, the level and box rule, validation and limits) under AddressSanitizer + UBSan.  scan.cpp calls nothing of
// the project's outside itself.  Every picture size 32..120 with every window size, boxes into exactly-sized buffers,
// short buffers, the limits and the values around them, and the refusals of plan_scene.
#include <climits>
#include <cstdio>
#include <string>
#include <vector>

#include "scan.h"

using namespace bnn;

#define CHECK(x) do { if (!(x)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

static bool has(const std::string &s, const char *what) { return s.find(what) != std::string::npos; }

static int grids() {
  for (int w = 0; w <= 120; w++)
    for (int h = 0; h <= 120; h += (w % 7 == 0 ? 1 : 5)) {
      int nx = -1, ny = -1;
      ScanPlan p;
      const std::string bad = plan_scan("t", w, h, p);
      if (w < 32 || h < 32) {
        CHECK(!scan_grid(w, h, &nx, &ny) && has(bad, "32 x 32 pixels or more"));
        continue;
      }
      CHECK(scan_grid(w, h, &nx, &ny) && bad.empty());
      CHECK(nx == (w - 32) / 4 + 1 && ny == (h - 32) / 4 + 1 && p.nx == nx && p.ny == ny);
      CHECK(p.wu <= w && p.wu > w - 4 && p.hu <= h && p.hu > h - 4);
      CHECK(p.w[0] == p.wu - 2 && p.w[1] == 14 + 2 * (nx - 1) && p.w[2] == p.w[1] - 2 && p.w[3] == 5 + (nx - 1) && p.w[4] == p.w[3] - 2 && p.w[5] == nx);
      CHECK(p.h[0] == p.hu - 2 && p.h[1] == 14 + 2 * (ny - 1) && p.h[2] == p.h[1] - 2 && p.h[3] == 5 + (ny - 1) && p.h[4] == p.h[3] - 2 && p.h[5] == ny);
      // what the kernels read stays inside the map before it: a quad's 4 x 4 patch, a pixel's 3 x 3 window
      CHECK(2 * (p.w[1] - 1) + 3 <= p.w[0] - 1 && 2 * (p.h[1] - 1) + 3 <= p.h[0] - 1);
      CHECK(2 * (p.w[2] / 2 - 1) + 3 <= p.w[1] - 1 && 2 * (p.w[3] - 1) + 3 <= p.w[2] - 1 && p.w[4] + 1 <= p.w[3] - 1 && p.w[5] + 1 <= p.w[4] - 1);
      CHECK(2 * (p.h[2] / 2 - 1) + 3 <= p.h[1] - 1 && 2 * (p.h[3] - 1) + 3 <= p.h[2] - 1 && p.h[4] + 1 <= p.h[3] - 1 && p.h[5] + 1 <= p.h[4] - 1);
      for (int s = 0; s < kScanStages; s++) CHECK(scan_stage_bytes(p, s) <= ((s & 1) ? p.buf1 : p.buf0));
      CHECK(p.buf0 >= (size_t)nx * ny * 64 && p.buf1 >= (size_t)nx * ny * 64);
    }
  CHECK(scan_grid(40, 40, nullptr, nullptr));
  return 0;
}

static int boxes() {
  const int sizes[] = {8, 16, 24, 32, 40, 48, 64, 96, 128};
  for (int w = 32; w <= 120; w += 3)
    for (int h = 32; h <= 120; h += 5)
      for (int s : sizes) {
        int lw = 0, lh = 0;
        const long n = scan_boxes(w, h, s, nullptr, 0);
        if (!scan_level(w, h, s, &lw, &lh)) { CHECK(n == -1); continue; }
        CHECK(lw == w * 32 / s && lh == h * 32 / s && lw >= 32 && lh >= 32);
        CHECK(n == (long)((lw - 32) / 4 + 1) * ((lh - 32) / 4 + 1));
        std::vector<int> b((size_t)n * 4, -1);  // exactly sized: one box too many written is a heap overflow
        CHECK(scan_boxes(w, h, s, b.data(), n) == n);
        for (long k = 0; k < n; k++) {
          const int *x = &b[(size_t)k * 4];
          CHECK(x[0] >= 0 && x[1] >= 0 && x[2] == x[0] + s && x[3] == x[1] + s && x[2] <= w && x[3] <= h);
          CHECK(x[0] % (s / 8) == 0 && x[1] % (s / 8) == 0);
        }
        CHECK(b[0] == 0 && b[1] == 0);
        std::vector<int> few(4, -1);
        CHECK(scan_boxes(w, h, s, few.data(), 1) == n && few[2] == s);
        CHECK(scan_boxes(w, h, s, few.data(), 0) == n);
      }
  for (int s : {0, 4, 7, 9, 36, -8, INT_MIN, INT_MAX}) CHECK(scan_boxes(64, 64, s, nullptr, 0) == -1);
  CHECK(scan_boxes(INT_MAX, INT_MAX, 8, nullptr, 0) == -1);  // (a level beyond an int: refused, no overflow on the way)
  CHECK(!scan_level(0, 64, 32, nullptr, nullptr) && !scan_level(64, -1, 32, nullptr, nullptr) && scan_level(64, 64, 64, nullptr, nullptr));
  return 0;
}

static int limits() {
  ScanPlan p;
  CHECK(plan_scan("t", kScanMaxSide, 32, p).empty() && p.nx == (kScanMaxSide - 32) / 4 + 1 && p.ny == 1);
  CHECK(has(plan_scan("t", kScanMaxSide + 1, 32, p), "pixels a side") && has(plan_scan("t", 32, kScanMaxSide + 1, p), "pixels a side"));
  CHECK(has(plan_scan("t", INT_MAX, INT_MAX, p), "pixels a side") && has(plan_scan("t", INT_MIN, 40, p), "32 x 32"));
  CHECK(has(plan_scan("t", kScanMaxSide, kScanMaxSide, p), "windows, more than the limit"));
  CHECK(has(plan_scan("t", 4096, 4096, p), "bytes, more than the limit"));
  CHECK(plan_scan("t", 4096, 2048, p).empty() && p.buf0 + p.buf1 <= kScanMaxMapBytes && (long)p.nx * p.ny <= kScanMaxWindows);
  // the largest accepted maps: every item count of the kernels fits an int
  CHECK((long)p.w[0] * p.h[0] < INT_MAX / 8);
  return 0;
}

static int scenes() {
  ScenePlan plan;
  const int two[2] = {64, 48}, bad[2] = {64, 20}, big[1] = {8}, same[1] = {32};
  int px = 0;
  CHECK(plan_scene("t", &px, 80, 72, 3, 0, two, 2, &px, plan).empty());
  CHECK(plan.levels.size() == 2 && plan.levels[0].level_w == 40 && plan.levels[0].level_h == 36 && plan.levels[1].level_w == 53 && plan.levels[1].level_h == 48);
  CHECK(plan.levels[0].first == 0 && plan.levels[1].first == 3 * 2 && plan.windows == 3 * 2 + 6 * 5 && plan.levels[0].resized && plan.levels[1].resized);
  CHECK(plan_scene("t", &px, 80, 72, 1, 80, same, 1, &px, plan).empty() && !plan.levels[0].resized && plan.windows == 13 * 11);
  CHECK(has(plan_scene("t", &px, 80, 72, 3, 0, bad, 2, &px, plan), "window size 20 is not a multiple of 8"));
  CHECK(has(plan_scene("t", &px, 4096, 4096, 3, 0, big, 1, &px, plan), "pixels a side"));
  CHECK(has(plan_scene("t", nullptr, 80, 72, 3, 0, two, 2, &px, plan), "null pointer") && has(plan_scene("t", &px, 80, 72, 3, 0, nullptr, 2, &px, plan), "null pointer") &&
        has(plan_scene("t", &px, 80, 72, 3, 0, two, 2, nullptr, plan), "null pointer"));
  CHECK(has(plan_scene("t", &px, 80, 72, 3, 0, two, 0, &px, plan), "one window size or more") && has(plan_scene("t", &px, 80, 72, 3, 0, two, -3, &px, plan), "one window size"));
  CHECK(has(plan_scene("t", &px, 80, 72, 4, 0, two, 2, &px, plan), "bands must be") && has(plan_scene("t", &px, 80, 72, 3, 239, two, 2, &px, plan), "row stride"));
  CHECK(has(plan_scene("t", &px, 31, 72, 3, 0, two, 2, &px, plan), "32 x 32") && has(plan_scene("t", &px, 60, 60, 3, 0, two, 2, &px, plan), "level below 32 x 32"));
  return 0;
}

int main() {
  if (grids() || boxes() || limits() || scenes()) return 1;
  std::printf("scan sanitize run ok\n");
  return 0;
}
