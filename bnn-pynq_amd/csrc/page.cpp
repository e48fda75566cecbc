// see page.h
#include "page.h"

#include <algorithm>
#include <numeric>
#include <tuple>

namespace bnn {

std::string validate_page(const char *what, const PageOpts *page) {
  const std::string name = std::string(what) + ": ";
  if (!page) return name + "bad arguments (null pointer)";
  if (page->mask != 0 && page->mask != 1) return name + "mask must be 0 (the crop of the box) or 1 (the glyph's own ink)";
  if (page->line_order != 0 && page->line_order != 1) return name + "line_order must be 0 (the order of find) or 1 (line by line)";
  if (page->word_gap < 0) return name + "word_gap must be 0 (none) or more";
  if (page->word_gap > 0 && page->line_order == 0) return name + "word_gap needs line_order 1";
  return "";
}

std::string validate_order_lines(const char *what, const int *boxes, const int *first, int n, int word_gap, const int *order) {
  const std::string name = std::string(what) + ": ";
  if (n < 0) return name + "negative number of boxes";
  if (!boxes || !first || !order) return name + "bad arguments (null pointer)";
  if (word_gap < 0) return name + "word_gap must be 0 (none) or more";
  if (n > kMaxLineComponents)
    return name + "more than " + std::to_string(kMaxLineComponents) + " components to put into lines (" + std::to_string(n) +
           "): raise min_pixels";
  for (int i = 0; i < n; i++) {
    const int *b = boxes + 4 * (size_t)i;
    if (b[2] <= b[0] || b[3] <= b[1])
      return name + "box " + std::to_string(i) + " (" + std::to_string(b[0]) + ", " + std::to_string(b[1]) + ", " + std::to_string(b[2]) + ", " +
             std::to_string(b[3]) + ") is empty or inverted (need right > left and lower > upper)";
  }
  return "";
}

std::string order_lines(const std::vector<Component> &kept, int word_gap, std::vector<int32_t> &order, std::vector<int32_t> &line,
                        std::vector<int32_t> &gap) {
  const size_t n = kept.size();
  order.clear();
  line.clear();
  gap.clear();
  if (n > (size_t)kMaxLineComponents)
    return "more than " + std::to_string(kMaxLineComponents) + " components to put into lines (" + std::to_string(n) + "): raise min_pixels";
  std::vector<int32_t> visit(n);
  std::iota(visit.begin(), visit.end(), 0);
  std::sort(visit.begin(), visit.end(), [&](int32_t a, int32_t b) {
    return std::tie(kept[(size_t)a].upper, kept[(size_t)a].first, a) < std::tie(kept[(size_t)b].upper, kept[(size_t)b].first, b);
  });
  struct Band {
    long top, bottom;
    std::vector<int32_t> members;
  };
  std::vector<Band> bands;
  for (const int32_t i : visit) {
    const Component &c = kept[(size_t)i];
    const long u = c.upper, b = c.lower, h = b - u;
    long best_ov = 0;
    int best = -1;
    for (size_t k = 0; k < bands.size(); k++) {
      const Band &band = bands[k];
      const long ov = std::min(b, band.bottom) - std::max(u, band.top);
      if (2 * ov >= std::min(h, band.bottom - band.top) && (best < 0 || ov > best_ov)) {
        best = (int)k;
        best_ov = ov;
      }
    }
    if (best < 0) {
      bands.push_back(Band{u, b, {i}});
    } else {
      bands[(size_t)best].bottom = std::max(bands[(size_t)best].bottom, b);
      bands[(size_t)best].members.push_back(i);
    }
  }
  order.reserve(n);
  line.reserve(n);
  gap.reserve(n);
  for (size_t k = 0; k < bands.size(); k++) {
    std::vector<int32_t> &m = bands[k].members;
    std::sort(m.begin(), m.end(), [&](int32_t a, int32_t b) {
      const Component &x = kept[(size_t)a], &y = kept[(size_t)b];
      return std::tie(x.left, x.upper, x.first, a) < std::tie(y.left, y.upper, y.first, b);
    });
    long right = 0;
    for (size_t j = 0; j < m.size(); j++) {
      const Component &c = kept[(size_t)m[j]];
      order.push_back(m[j]);
      line.push_back((int32_t)k);
      gap.push_back(word_gap > 0 && j > 0 && (long)c.left - right >= (long)word_gap ? 1 : 0);
      right = j == 0 ? (long)c.right : std::max(right, (long)c.right);
    }
  }
  return "";
}

std::string plan_page(const std::vector<Component> &chosen, int filter, int square_blank, GlyphPlan &plan, std::vector<int32_t> &keys) {
  const size_t n = chosen.size();
  std::vector<int> boxes(n * 4), found(n * 4);
  keys.assign(n * 2, 0);
  for (size_t i = 0; i < n; i++) {
    const Component &c = chosen[i];
    boxes[4 * i] = c.left; boxes[4 * i + 1] = c.upper; boxes[4 * i + 2] = c.right; boxes[4 * i + 3] = c.lower;
    // a component's extreme pixels are its own: what k_glyph_bbox would find in the masked picture
    found[4 * i] = c.left; found[4 * i + 1] = c.upper; found[4 * i + 2] = c.right - 1; found[4 * i + 3] = c.lower - 1;
    keys[2 * i] = c.first;
    keys[2 * i + 1] = -2 - c.id;
  }
  return plan_glyphs(boxes.data(), found.data(), (int)n, filter, square_blank, plan);
}

}  // namespace bnn
