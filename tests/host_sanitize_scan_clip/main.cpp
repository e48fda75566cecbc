// Stand-alone driver for tests/test_host_sanitize_scan_clip.py: the host-only code of the clip scan (csrc/scan_clip.cpp on
// top of csrc/scan.cpp: the order of the maps, the layout, the launch tables, the limits, the capacity) under
// AddressSanitizer + UBSan.  Frame sizes 32..120 with several size sets and frame counts; for each accepted clip the
// layout's invariants and the tables a merged launch reads -- every block of every stage names a map whose items it holds,
// and everything a lane of that block reads or writes lies inside the planes and the two buffers; the limits, the values
// around them, and the refusals.
#include <climits>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "scan_clip.h"

using namespace bnn;

#define CHECK(x) do { if (!(x)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

static bool has(const std::string &s, const char *what) { return s.find(what) != std::string::npos; }

// the invariants of an accepted plan and of its tables
static int check_plan(const ClipPlan &p, int n_sizes) {
  const size_t M = p.maps.size();
  CHECK(M == (size_t)p.frames * n_sizes && p.level_planes.size() == (size_t)n_sizes);
  long first = 0;
  size_t total[kScanStages] = {};
  long blocks[kScanStages] = {};
  for (size_t m = 0; m < M; m++) {
    const ClipMap &cm = p.maps[m];
    CHECK(cm.frame == (int)(m / n_sizes) && cm.level == (int)(m % n_sizes) && cm.first == first);
    const ScanLevel &lv = p.scene.levels[(size_t)cm.level];
    for (int s = 0; s < kScanStages; s++) {
      CHECK(cm.off[s] == total[s] && cm.off[s] % 8 == 0);
      total[s] += scan_stage_bytes(lv.plan, s);
      CHECK(total[s] <= ((s & 1) ? p.buf1 : p.buf0));
      blocks[s] += scan_clip_blocks(lv.plan, s);
    }
    CHECK(cm.off[5] == (size_t)cm.first * 32);
    CHECK(cm.planes + (size_t)3 * lv.level_w * lv.level_h <= p.planes_bytes);
    first += (long)lv.plan.nx * lv.plan.ny;
  }
  CHECK(first == p.windows && p.windows <= kScanMaxWindows);
  CHECK(p.buf0 >= (size_t)p.windows * 64 && p.buf1 >= (size_t)p.windows * 64 && p.buf0 <= kScanMaxMapBytes && p.buf1 <= kScanMaxMapBytes);
  for (int s = 0; s < kScanStages; s++) CHECK(total[s] == p.stage_bytes[s] && blocks[s] == p.blocks[s] && blocks[s] >= (long)M);

  ClipTables t;
  clip_tables(p, t);
  for (int s = 0; s < kScanStages; s++) {
    CHECK(t.desc[s] % 2 == 0 && t.block_map[s] == t.desc[s] + M * 12 && t.block_map[s] + (size_t)p.blocks[s] <= t.words.size());
    const size_t in_bytes = s == 0 ? p.planes_bytes : p.stage_bytes[s - 1];
    long covered = 0;
    for (long b = 0; b < p.blocks[s]; b++) {
      const int m = t.words[t.block_map[s] + (size_t)b];
      CHECK(m >= 0 && (size_t)m < M);
      ClipMapDesc d;
      std::memcpy(&d, &t.words[t.desc[s] + (size_t)m * 12], sizeof(d));
      const ScanLevel &lv = p.scene.levels[(size_t)p.maps[(size_t)m].level];
      const long nb = scan_clip_blocks(lv.plan, s);
      CHECK(d.first_block <= b && b < d.first_block + nb && d.n_items == scan_clip_items(lv.plan, s) && d.n_items > (b - d.first_block) * kScanClipBlock);
      if (b != d.first_block) continue;
      covered += nb;
      // the last item's reads and writes (the largest addresses of the map), as the kernels compute them
      const int w = lv.plan.w[s], h = lv.plan.h[s], dw = kScanStageDwords[s];
      CHECK(d.out_off == (long long)p.maps[(size_t)m].off[s] && (size_t)d.out_off + (size_t)w * h * dw * 4 <= p.stage_bytes[s]);
      if (s == 0) {
        CHECK(d.ow == w && d.n_items == w * h && d.row_stride == lv.level_w && d.plane_stride == (long long)lv.level_w * lv.level_h);
        // pixel (h - 1, w - 1) reads rows .. + 2, columns .. + 2 of plane 2
        CHECK(2 * (size_t)d.plane_stride + (size_t)(h + 1) * d.row_stride + (w + 1) < 3 * (size_t)d.plane_stride && w + 1 < d.row_stride);
        CHECK((size_t)d.in_off + 3 * (size_t)d.plane_stride <= in_bytes);
      } else {
        const int iw = lv.plan.w[s - 1], ih = lv.plan.h[s - 1], idw = kScanStageDwords[s - 1];
        CHECK(d.iw == iw && d.in_off == (long long)p.maps[(size_t)m].off[s - 1] && (size_t)d.in_off + (size_t)iw * ih * idw * 4 <= in_bytes);
        if (s <= 3) {  // quads: item (qh - 1, qw - 1) reads the 4 x 4 patch at (2 qy, 2 qx)
          const int qw = d.ow, qh = d.n_items / qw;
          CHECK(qw * qh == d.n_items && 2 * (qw - 1) + 3 <= iw - 1 && 2 * (qh - 1) + 3 <= ih - 1);
          CHECK(s == 2 ? (2 * qw == w && 2 * qh == h) : (qw == w && qh == h));
        } else {
          CHECK(d.ow == w && d.n_items == w * h && w + 1 <= iw - 1 && h + 1 <= ih - 1);
        }
      }
    }
    CHECK(covered == p.blocks[s]);
  }
  return 0;
}

static int clips() {
  const int sets[][3] = {{32, 0, 0}, {8, 0, 0}, {64, 48, 0}, {32, 40, 0}, {96, 64, 32}, {40, 40, 24}};
  int px = 0;
  for (int w = 32; w <= 120; w += 11)
    for (int h = 32; h <= 120; h += 13)
      for (const auto &set : sets)
        for (int frames : {1, 2, 5}) {
          const int n_sizes = set[1] == 0 ? 1 : set[2] == 0 ? 2 : 3;
          ClipPlan p;
          const std::string bad = plan_clip("t", &px, frames, 0, w, h, 3, 0, set, n_sizes, &px, p);
          ScenePlan scene;
          if (!plan_scene("t", &px, w, h, 3, 0, set, n_sizes, &px, scene).empty()) { CHECK(!bad.empty()); continue; }
          CHECK(bad.empty() && p.windows == scene.windows * frames);
          if (check_plan(p, n_sizes)) return 1;
        }
  // the GPU tests' clip, with strides
  const int two[2] = {32, 40};
  ClipPlan p;
  CHECK(plan_clip("t", &px, 3, 0, 100, 52, 3, 0, two, 2, &px, p).empty() && p.windows == 3 * 147 && p.blocks[0] == 3 * 32 && p.blocks[5] == 6);
  CHECK(plan_clip("t", &px, 2, 56 * 41 + 24, 50, 41, 1, 56, two, 2, &px, p).empty() && p.frame_stride == 56 * 41 + 24 && !check_plan(p, 2));
  return 0;
}

static int limits() {
  int px = 0;
  ClipPlan p;
  std::string why;
  const int vga[2] = {64, 96}, s32[1] = {32}, s8192[1] = {8192}, bad[2] = {64, 20};
  const int cap = scan_clip_capacity("t", 640, 480, vga, 2, why);
  CHECK(cap == 154 && why.empty());
  CHECK(plan_clip("t", &px, cap, 0, 640, 480, 3, 0, vga, 2, &px, p).empty() && p.windows == 154L * 5387 && !check_plan(p, 2));
  CHECK(has(plan_clip("t", &px, cap + 1, 0, 640, 480, 3, 0, vga, 2, &px, p), "bytes in one buffer, more than the limit"));
  CHECK(scan_clip_capacity("t", 32, 32, s32, 1, why) == kScanClipMaxFrames);
  CHECK(plan_clip("t", &px, kScanClipMaxFrames, 0, 32, 32, 3, 0, s32, 1, &px, p).empty() && p.windows == kScanClipMaxFrames && !check_plan(p, 1));
  CHECK(has(plan_clip("t", &px, kScanClipMaxFrames + 1, 0, 32, 32, 3, 0, s32, 1, &px, p), "need 1 to 4096 frames"));
  CHECK(has(plan_clip("t", &px, 0, 0, 32, 32, 3, 0, s32, 1, &px, p), "need 1 to 4096 frames") && has(plan_clip("t", &px, INT_MIN, 0, 32, 32, 3, 0, s32, 1, &px, p), "frames"));
  CHECK(has(plan_clip("t", &px, 5, 0, 2048, 2048, 3, 0, s32, 1, &px, p), "windows, more than the limit"));
  CHECK(scan_clip_capacity("t", 2048, 2048, s32, 1, why) == 4 && plan_clip("t", &px, 4, 0, 2048, 2048, 3, 0, s32, 1, &px, p).empty() && !check_plan(p, 1));
  const int c8k = scan_clip_capacity("t", 8192, 8192, s8192, 1, why);
  CHECK(c8k == 5 && plan_clip("t", &px, 5, 0, 8192, 8192, 3, 0, s8192, 1, &px, p).empty() && p.windows == 5);
  CHECK(has(plan_clip("t", &px, 6, 0, 8192, 8192, 3, 0, s8192, 1, &px, p), "bytes, more than the limit of 1073741824"));
  CHECK(plan_clip("t", &px, 6, 0, 8192, 8192, 1, 0, s8192, 1, &px, p).empty());  // L frames: a third of the bytes
  // strides
  CHECK(has(plan_clip("t", &px, 2, 80 * 72 * 3 - 1, 80, 72, 3, 0, vga, 1, &px, p), "frame stride shorter than a frame"));
  CHECK(has(plan_clip("t", &px, 2, 80 * 72 * 3, 80, 72, 3, 256, vga, 1, &px, p), "frame stride shorter than a frame"));
  CHECK(has(plan_clip("t", &px, 2, LONG_MIN, 80, 72, 3, 0, vga, 1, &px, p), "frame stride shorter than a frame"));
  CHECK(plan_clip("t", &px, 2, 256 * 72, 80, 72, 3, 256, vga, 1, &px, p).empty() && plan_clip("t", &px, 2, LONG_MAX, 80, 72, 3, 0, vga, 1, &px, p).empty());
  CHECK(has(plan_clip("t", &px, 2, 0, 80, 72, 3, 239, vga, 1, &px, p), "row stride"));
  // scan_scene's refusals, in its words
  CHECK(has(plan_clip("t", nullptr, 2, 0, 80, 72, 3, 0, vga, 1, &px, p), "null pointer") && has(plan_clip("t", &px, 2, 0, 80, 72, 3, 0, nullptr, 1, &px, p), "null pointer") &&
        has(plan_clip("t", &px, 2, 0, 80, 72, 3, 0, vga, 1, nullptr, p), "null pointer"));
  CHECK(has(plan_clip("t", &px, 2, 0, 80, 72, 4, 0, vga, 1, &px, p), "bands must be") && has(plan_clip("t", &px, 2, 0, 80, 72, 3, 0, vga, 0, &px, p), "one window size"));
  CHECK(has(plan_clip("t", &px, 2, 0, 80, 72, 3, 0, bad, 2, &px, p), "window size 20 is not a multiple of 8"));
  CHECK(scan_clip_capacity("t", 31, 40, s32, 1, why) == 0 && has(why, "32 x 32"));
  CHECK(scan_clip_capacity("t", 4096, 4096, s32, 1, why) == 0 && has(why, "bytes, more than the limit"));
  CHECK(scan_clip_capacity("t", 64, 64, nullptr, 1, why) == 0 && has(why, "null pointer"));
  CHECK(scan_clip_capacity("t", 64, 64, s32, -1, why) == 0 && has(why, "one window size"));
  return 0;
}

int main() {
  if (clips() || limits()) return 1;
  std::printf("scan clip sanitize run ok\n");
  return 0;
}
