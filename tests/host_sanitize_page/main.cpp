// Stand-alone driver for tests/test_host_sanitize_page.py: the host-only code of read_page (csrc/page.cpp: validation,
// order_lines, the masked route's plan) under AddressSanitizer + UBSan, together with what it calls (components.cpp,
// glyphs.cpp, resample.cpp).  The hand-worked cases of tests/test_page_lines.py, random box sets, the components of
// labelled noise through select_components, order_lines and plan_page, and the limit.
#include <algorithm>
#include <climits>
#include <cstdio>
#include <string>
#include <tuple>
#include <vector>

#include "page.h"

using namespace bnn;

#define CHECK(x) do { if (!(x)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

struct Box { int l, u, r, b, first; };

static std::vector<Component> components(const std::vector<Box> &boxes) {
  std::vector<Component> c;
  for (const Box &x : boxes) c.push_back(Component{x.first, x.l, x.u, x.r, x.b, 1, x.first, 0});
  return c;
}

// order_lines on exactly-sized vectors, and what every caller relies on: a permutation, lines ascending from 0 without
// a hole, inside a line ascending (l, u, f), a gap only behind a glyph of the same line
static int lines(const std::vector<Box> &boxes, int word_gap, std::vector<int32_t> &order, std::vector<int32_t> &line, std::vector<int32_t> &gap) {
  const std::vector<Component> kept = components(boxes);
  CHECK(order_lines(kept, word_gap, order, line, gap).empty());
  const size_t n = boxes.size();
  CHECK(order.size() == n && line.size() == n && gap.size() == n);
  std::vector<int> seen(n, 0);
  for (size_t i = 0; i < n; i++) {
    CHECK(order[i] >= 0 && (size_t)order[i] < n && !seen[(size_t)order[i]]++);
    CHECK(line[i] == (i ? line[i - 1] : 0) || (i && line[i] == line[i - 1] + 1));
    CHECK(gap[i] == 0 || gap[i] == 1);
    if (i == 0 || line[i] != line[i - 1]) CHECK(gap[i] == 0);
    else {
      const Box &p = boxes[(size_t)order[i - 1]], &q = boxes[(size_t)order[i]];
      CHECK(std::make_tuple(p.l, p.u, p.first, order[i - 1]) < std::make_tuple(q.l, q.u, q.first, order[i]));
    }
    if (word_gap == 0) CHECK(gap[i] == 0);
  }
  return 0;
}

static int expect(const std::vector<Box> &boxes, int word_gap, const std::vector<int32_t> &order, const std::vector<int32_t> &line,
                  const std::vector<int32_t> &gap) {
  std::vector<int32_t> o, l, g;
  CHECK(lines(boxes, word_gap, o, l, g) == 0);
  CHECK(o == order && l == line && g == gap);
  return 0;
}

// plan_page on `chosen`: what the record kernel relies on -- the descriptor's box IS the component's box and lies where it
// did, tables inside the coefficient buffer, temporaries apart, two keys per glyph, never status 1
static int plan(const std::vector<Component> &chosen, int filter, int square_blank) {
  GlyphPlan p;
  std::vector<int32_t> keys;
  CHECK(plan_page(chosen, filter, square_blank, p, keys).empty());
  const size_t n = chosen.size();
  CHECK(p.desc.size() == n && p.status.size() == n && p.ink_boxes.size() == 4 * n && keys.size() == 2 * n);
  size_t tmp_end = 0;
  for (size_t i = 0; i < n; i++) {
    const Component &c = chosen[i];
    const GlyphDesc &d = p.desc[i];
    CHECK(keys[2 * i] == c.first && keys[2 * i + 1] == -2 - c.id);
    CHECK(p.ink_boxes[4 * i] == c.left && p.ink_boxes[4 * i + 1] == c.upper && p.ink_boxes[4 * i + 2] == c.right && p.ink_boxes[4 * i + 3] == c.lower);
    CHECK(p.status[i] == kGlyphOk || p.status[i] == kGlyphTooThin);
    CHECK((p.status[i] == kGlyphTooThin) == ((d.flags & kGlyphSkip) != 0));
    if (d.flags & kGlyphSkip) continue;
    CHECK(d.x0 == c.left && d.y0 == c.upper && d.w == c.right - c.left && d.h == c.lower - c.upper);
    CHECK(d.out_w >= 1 && d.out_w <= kGlyphSide && d.out_h >= 1 && d.out_h <= kGlyphSide);
    CHECK(d.off_x >= 0 && d.off_x + d.out_w <= kGlyphSide && d.off_y >= 0 && d.off_y + d.out_h <= kGlyphSide);
    if (d.flags & kGlyphBlank) { CHECK(square_blank && d.w == d.h); continue; }
    if (d.flags & kGlyphHorizontal) {
      CHECK(d.kh >= 0 && (size_t)d.kh + (size_t)d.out_w * d.ksize_h <= p.coef.size() && (size_t)d.bh + 2 * (size_t)d.out_w <= p.coef.size());
      for (int xx = 0; xx < d.out_w; xx++) {  // every tap the kernel reads lies inside the box
        const int xmin = p.coef[(size_t)d.bh + 2 * xx], taps = p.coef[(size_t)d.bh + 2 * xx + 1];
        CHECK(xmin >= 0 && taps >= 1 && taps <= d.ksize_h && xmin + taps <= d.w);
      }
    }
    if (d.flags & kGlyphVertical) {
      CHECK(d.kv >= 0 && (size_t)d.kv + (size_t)d.out_h * d.ksize_v <= p.coef.size() && (size_t)d.bv + 2 * (size_t)d.out_h <= p.coef.size());
      for (int yy = 0; yy < d.out_h; yy++) {
        const int ymin = p.coef[(size_t)d.bv + 2 * yy], taps = p.coef[(size_t)d.bv + 2 * yy + 1];
        CHECK(ymin >= 0 && taps >= 1 && taps <= d.ksize_v && ymin + taps <= d.h);
      }
    }
    if (d.flags & kGlyphGlobalMid) {
      CHECK((size_t)d.h * d.out_w > (size_t)kGlyphMidBytes && (size_t)d.tmp == tmp_end && d.tmp % 16 == 0);
      tmp_end = (size_t)d.tmp + (((size_t)d.h * d.out_w + 15) & ~(size_t)15);
    } else if ((d.flags & kGlyphHorizontal) && (d.flags & kGlyphVertical)) {
      CHECK((size_t)d.h * d.out_w <= (size_t)kGlyphMidBytes);
    }
  }
  CHECK(tmp_end == p.tmp_bytes);
  return 0;
}

static unsigned lcg(unsigned &s) { return (s = s * 1664525u + 1013904223u) >> 8; }

int main() {
  // the hand-worked cases of tests/test_page_lines.py
  CHECK(expect({{12, 28, 30, 50, 2812}, {15, 5, 25, 15, 515}, {0, 30, 8, 40, 3000}, {0, 0, 10, 20, 0}}, 0, {3, 1, 2, 0}, {0, 0, 1, 1}, {0, 0, 0, 0}) == 0);
  CHECK(expect({{0, 0, 10, 30, 0}, {0, 20, 10, 50, 2000}, {20, 22, 30, 36, 2220}, {40, 24, 50, 30, 2440}}, 0, {0, 3, 1, 2}, {0, 0, 1, 1}, {0, 0, 0, 0}) == 0);
  CHECK(expect({{0, 0, 10, 20, 0}, {20, 10, 30, 30, 1020}}, 0, {0, 1}, {0, 0}, {0, 0}) == 0);
  CHECK(expect({{0, 0, 10, 20, 0}, {20, 11, 30, 31, 1120}}, 0, {0, 1}, {0, 1}, {0, 0}) == 0);
  CHECK(expect({{0, 0, 10, 20, 0}, {20, 18, 30, 22, 1820}}, 0, {0, 1}, {0, 0}, {0, 0}) == 0);
  CHECK(expect({{0, 0, 10, 20, 0}, {20, 19, 30, 23, 1920}}, 0, {0, 1}, {0, 1}, {0, 0}) == 0);
  CHECK(expect({{5, 5, 10, 10, 30}, {5, 5, 10, 10, 10}, {5, 5, 10, 10, 20}}, 3, {1, 2, 0}, {0, 0, 0}, {0, 0, 0}) == 0);
  CHECK(expect({{3, 4, 5, 6, 7}}, 1, {0}, {0}, {0}) == 0);
  CHECK(expect({}, 0, {}, {}, {}) == 0);
  CHECK(expect({}, 5, {}, {}, {}) == 0);
  CHECK(expect({{0, 0, 10, 10, 0}, {15, 0, 20, 10, 15}}, 5, {0, 1}, {0, 0}, {0, 1}) == 0);
  CHECK(expect({{0, 0, 10, 10, 0}, {15, 0, 20, 10, 15}}, 6, {0, 1}, {0, 0}, {0, 0}) == 0);
  CHECK(expect({{0, 0, 10, 10, 0}, {15, 0, 20, 10, 15}}, 0, {0, 1}, {0, 0}, {0, 0}) == 0);
  CHECK(expect({{0, 0, 30, 10, 0}, {5, 2, 8, 9, 205}, {33, 0, 40, 10, 33}}, 3, {0, 1, 2}, {0, 0, 0}, {0, 0, 1}) == 0);
  CHECK(expect({{0, 0, 30, 10, 0}, {5, 2, 8, 9, 205}, {33, 0, 40, 10, 33}}, 4, {0, 1, 2}, {0, 0, 0}, {0, 0, 0}) == 0);
  // coordinates at the ends of int: the differences are taken in long
  CHECK(expect({{INT_MIN, INT_MIN, INT_MAX, INT_MAX, 0}, {INT_MAX - 1, INT_MAX - 1, INT_MAX, INT_MAX, 1}, {INT_MIN, INT_MIN, INT_MIN + 1, INT_MIN + 1, 2}},
               INT_MAX, {0, 2, 1}, {0, 0, 0}, {0, 0, 0}) == 0);
  // random box sets of at most 40 boxes, duplicates among them
  unsigned seed = 5;
  for (int round = 0; round < 300; round++) {
    std::vector<Box> boxes;
    const int n = (int)(lcg(seed) % 41u), rows = 1 + (int)(lcg(seed) % 4u);
    for (int i = 0; i < n; i++) {
      const int u = (int)(lcg(seed) % (unsigned)rows) * 40 + (int)(lcg(seed) % 25u), h = 1 + (int)(lcg(seed) % (lcg(seed) % 10u ? 30u : 60u));
      const int l = (int)(lcg(seed) % 300u), w = 1 + (int)(lcg(seed) % 40u);
      boxes.push_back(Box{l, u, l + w, u + h, u * 400 + l});
      if (round % 7 == 0 && i % 5 == 0) boxes.push_back(boxes.back());
    }
    std::vector<int32_t> o, l, g;
    CHECK(lines(boxes, (int)(lcg(seed) % 30u), o, l, g) == 0);
    std::vector<Component> chosen;
    for (int32_t i : o) chosen.push_back(components(boxes)[(size_t)i]);
    for (int filter : {0, 3})
      for (int square_blank : {0, 1}) CHECK(plan(chosen, filter, square_blank) == 0);
  }
  // the device path's sequence on the host: label noise, select_components without a cap, order_lines, the cap, plan_page
  for (int level : {128, 255})
    for (int min_pixels : {1, 3}) {
      const int w = 150, h = 90;
      std::vector<uint8_t> a((size_t)w * h);
      unsigned s = 11u + (unsigned)level;
      for (auto &v : a) v = lcg(s) % 1000u < 250u ? (uint8_t)(lcg(s) % 255u) : 255;
      FindOpts f;
      f.ink_level = level; f.min_pixels = min_pixels;
      std::vector<Component> all, kept;
      label_components(a.data(), w, h, 0, f, all, nullptr);
      const long total = select_components(all, f, INT_MAX, kept);
      CHECK(total == (long)kept.size() && total > 0);
      std::vector<int32_t> o, l, g;
      CHECK(order_lines(kept, 4, o, l, g).empty() && o.size() == kept.size());
      for (size_t cap : {(size_t)1, (size_t)7, kept.size()}) {
        std::vector<Component> chosen;
        for (size_t i = 0; i < std::min(cap, o.size()); i++) chosen.push_back(kept[(size_t)o[i]]);
        CHECK(plan(chosen, 3, 0) == 0);
      }
    }
  // glyphs of every route, too thin, and past the LDS budget (two of them: the temporaries lie apart)
  {
    std::vector<Component> c;
    const int sizes[][2] = {{28, 20}, {28, 28}, {5, 24}, {24, 5}, {1, 1}, {1, 40}, {40, 1}, {3, 5}, {1250, 1300}, {1300, 1300}, {1207, 1171}, {60, 80}};
    int id = 0;
    for (const auto &wh : sizes) c.push_back(Component{id * 7, 3, 2, 3 + wh[0], 2 + wh[1], wh[0] * wh[1], id++, 0});
    for (int filter : {0, 3})
      for (int square_blank : {0, 1}) CHECK(plan(c, filter, square_blank) == 0);
    GlyphPlan p;
    std::vector<int32_t> keys;
    CHECK(plan_page(c, 3, 0, p, keys).empty() && p.status[5] == kGlyphTooThin && p.status[6] == kGlyphTooThin && p.tmp_bytes > 2 * (size_t)kGlyphMidBytes);
    CHECK(p.desc[2].flags == kGlyphVertical && p.desc[3].flags == kGlyphHorizontal && p.desc[0].flags == 0 && p.desc[1].flags == 0);
  }
  // the limit: 65 536 components are ordered, one more is refused; and the validation
  {
    std::vector<Component> many((size_t)kMaxLineComponents + 1);
    for (size_t i = 0; i < many.size(); i++) many[i] = Component{(int32_t)i, (int32_t)(many.size() - i), 0, (int32_t)(many.size() - i) + 1, 5, 1, (int32_t)i, 0};
    std::vector<int32_t> o, l, g;
    CHECK(!order_lines(many, 0, o, l, g).empty() && o.empty() && l.empty() && g.empty());
    many.pop_back();
    CHECK(order_lines(many, 2, o, l, g).empty() && o.size() == many.size() && o[0] == kMaxLineComponents - 1 && l.back() == 0);
  }
  PageOpts g;
  CHECK(validate_page("t", &g).empty() && !validate_page("t", nullptr).empty());
  for (int field = 0; field < 3; field++)
    for (int bad : {-1, 0, 1, 2, INT_MAX, INT_MIN}) {
      PageOpts q;
      int *slot[] = {&q.mask, &q.line_order, &q.word_gap};
      *slot[field] = bad;
      const bool fine = field == 2 ? bad >= 0 : (bad == 0 || bad == 1);
      CHECK(validate_page("t", &q).empty() == fine);
    }
  g = PageOpts{1, 0, 1};
  CHECK(!validate_page("t", &g).empty());
  const int box[8] = {0, 0, 4, 4, 5, 3, 9, 3}, first[2] = {0, 5};
  int out[2];
  CHECK(validate_order_lines("t", box, first, 1, 0, out).empty() && validate_order_lines("t", box, first, 0, 0, out).empty());
  CHECK(!validate_order_lines("t", box, first, 2, 0, out).empty() && !validate_order_lines("t", box, first, -1, 0, out).empty());
  CHECK(!validate_order_lines("t", nullptr, first, 1, 0, out).empty() && !validate_order_lines("t", box, nullptr, 1, 0, out).empty());
  CHECK(!validate_order_lines("t", box, first, 1, 0, nullptr).empty() && !validate_order_lines("t", box, first, 1, -1, out).empty());
  CHECK(!validate_order_lines("t", box, first, kMaxLineComponents + 1, 0, out).empty());
  std::printf("page sanitize run ok\n");
  return 0;
}
