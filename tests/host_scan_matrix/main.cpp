// The band tables of the clip scan's matrix form (clip_mfma_tables) for tests/test_scan_matrix_plan.py:  main WIDTH HEIGHT FRAMES SIZE...
//   map   STAGE M IN_OFF OUT_OFF IW OW ROW_PAIRS FIRST_BLOCK IN_BYTES OUT_W OUT_H   (IN_BYTES .. OUT_H: from the plan, not the table)
//   band  STAGE BLOCK M RP0 X0
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "scan_clip.h"
using namespace bnn;

int main(int argc, char **argv) {
  if (argc < 5) return 2;
  const int width = std::atoi(argv[1]), height = std::atoi(argv[2]), frames = std::atoi(argv[3]);
  std::vector<int> sizes;
  for (int i = 4; i < argc; i++) sizes.push_back(std::atoi(argv[i]));
  ClipPlan plan;
  const std::string bad = plan_clip("plan", &plan, frames, 0, width, height, 3, 0, sizes.data(), (int)sizes.size(), &plan, plan);
  if (!bad.empty()) { std::fprintf(stderr, "%s\n", bad.c_str()); return 1; }
  ClipMfmaTables t;
  clip_mfma_tables(plan, t);
  std::printf("consts %d %d\n", kClipMfmaRowPairs, kClipMfmaChunk);
  for (int s = 1; s <= 3; s++) {
    for (size_t m = 0; m < plan.maps.size(); m++) {
      ClipMfmaMap d;
      std::memcpy(&d, &t.words[t.maps[s] + m * 8], sizeof(d));
      const ScanPlan &p = plan.scene.levels[(size_t)plan.maps[m].level].plan;
      std::printf("map %d %zu %lld %lld %d %d %d %d %zu %d %d\n", s, m, d.in_off, d.out_off, d.iw, d.ow, d.row_pairs, d.first_block,
                  scan_stage_bytes(p, s - 1), p.w[s], p.h[s]);
    }
    if (t.bands[s] + (size_t)t.blocks[s] * 4 > t.words.size()) return 1;
    for (long b = 0; b < t.blocks[s]; b++) {
      ClipMfmaBand q;
      std::memcpy(&q, &t.words[t.bands[s] + (size_t)b * 4], sizeof(q));
      std::printf("band %d %ld %d %d %d\n", s, b, q.map, q.rp0, q.x0);
    }
  }
  return 0;
}
