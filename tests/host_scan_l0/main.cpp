// The tables of the clip scan's matrix-core stage 0 (clip_l0_tables) for tests/test_scan_l0_plan.py:
//   main WIDTH HEIGHT FRAMES SIZE...     (FRAMES 0: as many as scan_clip_capacity allows)
//   consts ROWS COLS / plan FRAMES PLANES_BYTES PLANES_TOP BLOCKS / band BLOCK M Y0 X0
//   map M IN_OFF OUT_OFF PLANE_STRIDE ROW_STRIDE OW OH FIRST_BLOCK LEVEL_W LEVEL_H    (LEVEL_W, LEVEL_H: from the plan)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "scan_clip.h"
using namespace bnn;

int main(int argc, char **argv) {
  if (argc < 5) return 2;
  const int width = std::atoi(argv[1]), height = std::atoi(argv[2]);
  int frames = std::atoi(argv[3]);
  std::vector<int> sizes;
  for (int i = 4; i < argc; i++) sizes.push_back(std::atoi(argv[i]));
  std::string bad;
  if (frames == 0) frames = scan_clip_capacity("plan", width, height, sizes.data(), (int)sizes.size(), bad);
  ClipPlan plan;
  bad = plan_clip("plan", &plan, frames, 0, width, height, 3, 0, sizes.data(), (int)sizes.size(), &plan, plan);
  if (!bad.empty()) { std::fprintf(stderr, "%s\n", bad.c_str()); return 1; }
  ClipL0Tables t;
  clip_l0_tables(plan, t);
  std::printf("consts %d %d\nplan %d %zu %zu %ld\n", kClipL0Rows, kClipL0Cols, frames, plan.planes_bytes, t.planes_top, t.blocks);
  for (size_t m = 0; m < plan.maps.size(); m++) {
    ClipL0Map d;
    std::memcpy(&d, &t.words[t.maps + m * (sizeof(d) / 4)], sizeof(d));
    const ScanLevel &lv = plan.scene.levels[(size_t)plan.maps[m].level];
    std::printf("map %zu %lld %lld %lld %d %d %d %d %d %d\n", m, d.in_off, d.out_off, d.plane_stride, d.row_stride, d.ow, d.oh, d.first_block,
                lv.level_w, lv.level_h);
  }
  if (t.bands + (size_t)t.blocks * 4 != t.words.size()) return 1;
  for (long b = 0; b < t.blocks; b++) {
    ClipMfmaBand q;
    std::memcpy(&q, &t.words[t.bands + (size_t)b * 4], sizeof(q));
    std::printf("band %ld %d %d %d\n", b, q.map, q.rp0, q.x0);
  }
  return 0;
}
