// see clip_glyphs.h
#include "clip_glyphs.h"

#include <algorithm>
#include <climits>

namespace bnn {

ClipGlyphGeometry clip_glyph_geometry(int n_frames, int width, int height) {
  ClipGlyphGeometry g;
  g.frames = n_frames; g.width = width; g.height = height;
  g.tall_height = (long)n_frames * height;
  g.frame_pixels = (long)width * height;
  g.tiles_x = (width + kClipTileW - 1) / kClipTileW;
  g.tiles_y = (height + kClipTileH - 1) / kClipTileH;
  g.tiles = (long)g.tiles_x * g.tiles_y * n_frames;
  g.max_components = (size_t)n_frames * max_components(width, height);
  return g;
}

std::string validate_clip_glyphs(const char *what, int n_frames, long frame_stride, int width, int height, long row_bytes, int cap) {
  const std::string name = std::string(what) + ": ";
  if (n_frames < 1 || n_frames > kClipGlyphMaxFrames) return name + "n_frames must be 1.." + std::to_string(kClipGlyphMaxFrames);
  if ((long)n_frames * width * height > kMaxComponentPixels)
    return name + "need a clip of at most " + std::to_string(kMaxComponentPixels) + " pixels to label (" + std::to_string(n_frames) + " x " +
           std::to_string(width) + " x " + std::to_string(height) + " given): cut it into several calls";
  if (frame_stride != 0 && frame_stride < row_bytes * height) return name + "frame stride shorter than a frame's rows";
  if (cap < 1 || cap > INT_MAX / 4 / n_frames) return name + "cap must be 1 or more per frame, and n_frames x cap x 4 must fit an int";
  return "";
}

std::string split_clip_components(const std::vector<Component> &all, const ClipGlyphGeometry &g, const FindOpts &find, const PageOpts *page,
                                  int cap, ClipGlyphSplit &out) {
  std::vector<std::vector<Component>> by_frame((size_t)g.frames);
  for (const Component &c : all) {
    const long f = c.first / g.frame_pixels;
    if (c.first < 0 || f >= g.frames || c.upper < f * g.height || c.lower > (f + 1) * g.height) return "internal: a component leaves its frame";
    by_frame[(size_t)f].push_back(c);
  }
  out = ClipGlyphSplit{};
  out.start.assign(1, 0);
  const bool lines = page && page->line_order;
  std::vector<Component> chosen;
  std::vector<int32_t> order, line, gap;
  for (int f = 0; f < g.frames; f++) {
    // (order and line model depend on differences of rows and on the order of first pixels alone: tall coordinates do)
    const long total = select_components(by_frame[(size_t)f], find, lines ? INT_MAX : cap, chosen);
    if (lines) {
      const std::string bad = order_lines(chosen, page->word_gap, order, line, gap);
      if (!bad.empty()) return "frame " + std::to_string(f) + ": " + bad;
      const size_t n = std::min(order.size(), (size_t)cap);
      for (size_t i = 0; i < n; i++) {
        out.chosen.push_back(chosen[(size_t)order[i]]);
        out.line.push_back(line[i]);
        out.gap.push_back(gap[i]);
      }
    } else {
      out.chosen.insert(out.chosen.end(), chosen.begin(), chosen.end());
      out.line.resize(out.chosen.size(), 0);
      out.gap.resize(out.chosen.size(), 0);
    }
    out.total.push_back((int32_t)total);
    out.start.push_back((int32_t)out.chosen.size());
  }
  return "";
}

}  // namespace bnn
