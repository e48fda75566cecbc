// The host-only plan of the clip of glyphs (csrc/clip_glyphs.cpp) under AddressSanitizer and UBSan, driven by
// tests/test_clip_glyphs_plan.py.
//   main limits N_FRAMES FRAME_STRIDE W H ROW_BYTES CAP   -> the refusal, or "ok TILES_X TILES_Y TILES MAX_COMPONENTS"
//   main split N_FRAMES W H CAP LINES ORDER MIN_PIXELS    -> components "first left upper right lower pixels" from stdin (tall
//        coordinates, any order); prints "frame F TOTAL KEPT" and, per kept one, "first left upper right lower line gap" with
//        the box in frame coordinates
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "clip_glyphs.h"

using namespace bnn;

int main(int argc, char **argv) {
  if (argc == 8 && !std::strcmp(argv[1], "limits")) {
    const int n = std::atoi(argv[2]), w = std::atoi(argv[4]), h = std::atoi(argv[5]);
    const std::string bad = validate_clip_glyphs("clip", n, std::atol(argv[3]), w, h, std::atol(argv[6]), std::atoi(argv[7]));
    if (!bad.empty()) { std::printf("%s\n", bad.c_str()); return 0; }
    const ClipGlyphGeometry g = clip_glyph_geometry(n, w, h);
    std::printf("ok %d %d %ld %zu\n", g.tiles_x, g.tiles_y, g.tiles, g.max_components);
    return 0;
  }
  if (argc != 9 || std::strcmp(argv[1], "split")) return 2;
  const ClipGlyphGeometry g = clip_glyph_geometry(std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]));
  const int cap = std::atoi(argv[5]);
  PageOpts page;
  page.line_order = std::atoi(argv[6]);
  FindOpts find;
  find.order = std::atoi(argv[7]);
  find.min_pixels = std::atoi(argv[8]);
  std::vector<Component> all;
  Component c{};
  while (std::scanf("%d %d %d %d %d %d", &c.first, &c.left, &c.upper, &c.right, &c.lower, &c.pixels) == 6) {
    c.id = (int32_t)all.size();
    all.push_back(c);
  }
  ClipGlyphSplit s;
  const std::string bad = split_clip_components(all, g, find, &page, cap, s);
  if (!bad.empty()) { std::printf("%s\n", bad.c_str()); return 0; }
  for (int f = 0; f < g.frames; f++) {
    std::printf("frame %d %d %d\n", f, s.total[(size_t)f], s.start[(size_t)f + 1] - s.start[(size_t)f]);
    for (int k = s.start[(size_t)f]; k < s.start[(size_t)f + 1]; k++) {
      int32_t box[4];
      clip_frame_box(s.chosen[(size_t)k], f, g.height, box);
      std::printf("%d %d %d %d %d %d %d\n", s.chosen[(size_t)k].first, box[0], box[1], box[2], box[3], s.line[(size_t)k], s.gap[(size_t)k]);
    }
  }
  return 0;
}
