// see components.h
#include "components.h"

#include <algorithm>
#include <climits>
#include <tuple>

namespace bnn {

std::string validate_find(const char *what, int width, int height, const FindOpts *find, const void *boxes, int cap) {
  const std::string name = std::string(what) + ": ";
  if (!find || !boxes) return name + "bad arguments (null pointer)";
  if (find->ink_level < 1 || find->ink_level > 255) return name + "ink_level must be 1..255";
  if (find->reach_x < 1 || find->reach_x > kMaxReach || find->reach_y < 1 || find->reach_y > kMaxReach)
    return name + "reach must be 1.." + std::to_string(kMaxReach) + " in x and in y";
  if (find->min_pixels < 1) return name + "min_pixels must be 1 or more";
  if (find->order != kOrderRaster && find->order != kOrderLeft) return name + "order must be 0 (raster) or 1 (left to right)";
  if (cap < 1) return name + "cap must be 1 or more";
  if ((long)width * (long)height > kMaxComponentPixels)
    return name + "need a picture of at most " + std::to_string(kMaxComponentPixels) + " pixels to label (" + std::to_string(width) + " x " +
           std::to_string(height) + " given)";
  return "";
}

namespace {

int32_t find_root(std::vector<int32_t> &parent, int32_t i) {
  while (parent[(size_t)i] != i) {
    parent[(size_t)i] = parent[(size_t)parent[(size_t)i]];  // path halving
    i = parent[(size_t)i];
  }
  return i;
}

// the smaller index becomes the root: a set's root is its first pixel
void unite(std::vector<int32_t> &parent, int32_t a, int32_t b) {
  a = find_root(parent, a);
  b = find_root(parent, b);
  if (a == b) return;
  if (a < b) parent[(size_t)b] = a;
  else parent[(size_t)a] = b;
}

}  // namespace

void label_components(const uint8_t *plane, int width, int height, long row_stride, const FindOpts &find, std::vector<Component> &all,
                      std::vector<int32_t> *roots) {
  const size_t stride = row_stride ? (size_t)row_stride : (size_t)width;
  const size_t n = (size_t)width * (size_t)height;
  std::vector<int32_t> parent(n);
  auto ink = [&](int x, int y) { return plane[(size_t)y * stride + (size_t)x] < find.ink_level; };
  for (int y = 0; y < height; y++)
    for (int x = 0; x < width; x++) parent[(size_t)y * width + x] = ink(x, y) ? (int32_t)((size_t)y * width + x) : -1;
  // first pass: every ink pixel with the ink of the forward half of its neighbourhood
  for (int y = 0; y < height; y++) {
    for (int x = 0; x < width; x++) {
      const int32_t p = (int32_t)((size_t)y * width + x);
      if (parent[(size_t)p] < 0) continue;
      for (int dy = 0; dy <= find.reach_y && y + dy < height; dy++) {
        const int from = dy == 0 ? x + 1 : std::max(0, x - find.reach_x), to = std::min(width - 1, x + find.reach_x);
        for (int xx = from; xx <= to; xx++) {
          const int32_t q = (int32_t)((size_t)(y + dy) * width + xx);
          if (parent[(size_t)q] >= 0) unite(parent, p, q);
        }
      }
    }
  }
  // second pass: roots, boxes and counts; a root is met before every other pixel of its set
  all.clear();
  std::vector<int32_t> slot(n, -1);  // root -> position in `all`
  if (roots) roots->assign(n, -1);
  for (int y = 0; y < height; y++) {
    for (int x = 0; x < width; x++) {
      const int32_t p = (int32_t)((size_t)y * width + x);
      if (parent[(size_t)p] < 0) continue;
      const int32_t r = find_root(parent, p);
      if (roots) (*roots)[(size_t)p] = r;
      if (slot[(size_t)r] < 0) {
        slot[(size_t)r] = (int32_t)all.size();
        all.push_back(Component{r, INT_MAX, INT_MAX, 0, 0, 0, r, 0});
      }
      Component &c = all[(size_t)slot[(size_t)r]];
      c.left = std::min(c.left, x); c.upper = std::min(c.upper, y);
      c.right = std::max(c.right, x + 1); c.lower = std::max(c.lower, y + 1);
      c.pixels++;
    }
  }
}

long select_components(const std::vector<Component> &all, const FindOpts &find, int cap, std::vector<Component> &chosen) {
  chosen.clear();
  for (const Component &c : all)
    if (c.pixels >= find.min_pixels) chosen.push_back(c);
  if (find.order == kOrderLeft)
    std::sort(chosen.begin(), chosen.end(), [](const Component &a, const Component &b) {
      return std::tie(a.left, a.upper, a.first) < std::tie(b.left, b.upper, b.first);
    });
  else
    std::sort(chosen.begin(), chosen.end(), [](const Component &a, const Component &b) { return a.first < b.first; });
  const long total = (long)chosen.size();
  if (cap < 0) cap = 0;
  if ((long)cap < total) chosen.resize((size_t)cap);
  return total;
}

long find_components_host(const uint8_t *plane, int width, int height, long row_stride, const FindOpts &find, int *boxes, int *pixel_counts,
                          int32_t *labels, int cap) {
  std::vector<Component> all, chosen;
  std::vector<int32_t> roots;
  label_components(plane, width, height, row_stride, find, all, labels ? &roots : nullptr);
  const long total = select_components(all, find, cap, chosen);
  for (size_t k = 0; k < chosen.size(); k++) {
    const Component &c = chosen[k];
    boxes[4 * k] = c.left; boxes[4 * k + 1] = c.upper; boxes[4 * k + 2] = c.right; boxes[4 * k + 3] = c.lower;
    if (pixel_counts) pixel_counts[k] = c.pixels;
  }
  if (labels) {
    const size_t n = (size_t)width * (size_t)height;
    std::vector<int32_t> index(n, -1);  // first pixel -> returned index
    for (size_t k = 0; k < chosen.size(); k++) index[(size_t)chosen[k].first] = (int32_t)k;
    for (size_t p = 0; p < n; p++) labels[p] = roots[p] < 0 ? -1 : index[(size_t)roots[p]];
  }
  return total;
}

}  // namespace bnn
