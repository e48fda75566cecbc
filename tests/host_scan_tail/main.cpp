// The band tables of the clip scan's stages 4 and 5 on the matrix cores (clip_tail_tables) for tests/test_scan_tail_plan.py:  main WIDTH HEIGHT FRAMES SIZE...
//   map   STAGE M IN_OFF OUT_OFF OW OH BAND_COLS BAND_RPS FIRST_BLOCK IN_BYTES IN_W IN_H   (IN_BYTES .. IN_H: from the plan, not the table)
//   band  STAGE BLOCK M RP0 X0
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "scan_clip.h"
using namespace bnn;

int main(int argc, char **argv) {
  if (argc < 5) return 2;
  std::vector<int> sizes;
  for (int i = 4; i < argc; i++) sizes.push_back(std::atoi(argv[i]));
  ClipPlan plan;
  if (!plan_clip("plan", &plan, std::atoi(argv[3]), 0, std::atoi(argv[1]), std::atoi(argv[2]), 3, 0, sizes.data(), (int)sizes.size(), &plan, plan).empty()) return 1;
  ClipTailTables t;
  clip_tail_tables(plan, t);
  std::printf("consts %d %d\n", kClipTailRowPairs, kClipTailCols);
  for (int s = 4; s <= 5; s++) {
    for (size_t m = 0; m < plan.maps.size(); m++) {
      ClipTailMap d;
      std::memcpy(&d, &t.words[t.maps[s - 4] + m * 12], sizeof(d));
      const ScanPlan &p = plan.scene.levels[(size_t)plan.maps[m].level].plan;
      std::printf("map %d %zu %lld %lld %d %d %d %d %d %zu %d %d\n", s, m, d.in_off, d.out_off, d.ow, d.oh, d.band_cols, d.band_rps, d.first_block,
                  scan_stage_bytes(p, s - 1), p.w[s - 1], p.h[s - 1]);
    }
    for (long b = 0; b < t.blocks[s - 4]; b++) {
      ClipTailBand q;
      std::memcpy(&q, &t.words[t.bands[s - 4] + (size_t)b * 4], sizeof(q));
      std::printf("band %d %ld %d %d %d\n", s, b, q.map, q.rp0, q.x0);
    }
  }
  return 0;
}
