// Stand-alone driver for tests/test_host_sanitize_glyphs.py: the host-only code of enhance_picture / glyphs_to_mnist /
// classify_glyphs (csrc/glyphs.cpp on top of csrc/resample.cpp) under AddressSanitizer + UBSan.  The fit rule over a grid
// of ink boxes, both filters' tables for every (in, out) the fit can ask for up to 1300 (what the record kernel reads
// stays inside the ink box), validation on and off all four edges and for every option, and plans: no ink, too thin,
// square with and without square_blank, shared tables, glyphs on both sides of the LDS budget, 10^4 boxes.
#include <climits>
#include <cmath>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "glyphs.h"
#include "resample.h"

using namespace bnn;

#define CHECK(x) do { if (!(x)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

static int check_table(int filter, int in, int out) {
  std::vector<int32_t> kk, bounds;
  const int ksize = resample_coeffs(filter, in, out, kk, bounds);
  CHECK(ksize >= 1 && kk.size() == (size_t)out * ksize && bounds.size() == (size_t)out * 2);
  for (int xx = 0; xx < out; xx++) {
    const int xmin = bounds[2 * (size_t)xx], taps = bounds[2 * (size_t)xx + 1];
    CHECK(xmin >= 0 && taps >= 0 && taps <= ksize && xmin + taps <= in);
    long sum = 0;
    for (int x = 0; x < taps; x++) sum += kk[(size_t)xx * ksize + x];
    if (taps) CHECK(std::labs(sum - (1L << 22)) <= taps);  // normalised weights, each rounded once
  }
  return 0;
}

// what the record kernel relies on, for every glyph of a plan
static int check_plan(const std::vector<int> &boxes, const std::vector<int> &found, int filter, int square_blank, GlyphPlan &plan) {
  const int n = (int)boxes.size() / 4;
  CHECK(plan_glyphs(boxes.data(), found.data(), n, filter, square_blank, plan).empty());
  CHECK((int)plan.desc.size() == n && (int)plan.status.size() == n && (int)plan.ink_boxes.size() == 4 * n);
  size_t tmp_end = 0;
  for (int i = 0; i < n; i++) {
    const GlyphDesc &d = plan.desc[(size_t)i];
    const int *b = &boxes[4 * (size_t)i], *ib = &plan.ink_boxes[4 * (size_t)i];
    CHECK(ib[0] >= b[0] && ib[1] >= b[1] && ib[2] <= b[2] && ib[3] <= b[3] && ib[0] < ib[2] && ib[1] < ib[3]);
    CHECK(d.x0 == ib[0] && d.y0 == ib[1] && d.w == ib[2] - ib[0] && d.h == ib[3] - ib[1]);
    if (plan.status[(size_t)i] == kGlyphTooThin) { CHECK(d.flags == kGlyphSkip); continue; }
    CHECK(!(d.flags & kGlyphSkip));
    CHECK(d.out_w >= 1 && d.out_w <= 28 && d.out_h >= 1 && d.out_h <= 28 && (d.out_w == 28 || d.out_h == 28));
    CHECK(d.off_x >= 0 && d.off_x + d.out_w <= 28 && d.off_y >= 0 && d.off_y + d.out_h <= 28);
    if (plan.status[(size_t)i] == kGlyphNoInk) CHECK(d.flags == kGlyphBlank);
    if (d.flags & kGlyphBlank) continue;
    CHECK(((d.flags & kGlyphHorizontal) != 0) == (d.out_w != d.w) && ((d.flags & kGlyphVertical) != 0) == (d.out_h != d.h));
    if (d.flags & kGlyphHorizontal) {
      CHECK(d.kh >= 0 && d.bh == d.kh + d.out_w * d.ksize_h && (size_t)d.bh + 2 * (size_t)d.out_w <= plan.coef.size());
      for (int xx = 0; xx < d.out_w; xx++) CHECK(plan.coef[(size_t)d.bh + 2 * xx] >= 0 && plan.coef[(size_t)d.bh + 2 * xx + 1] <= d.ksize_h &&
                                                 plan.coef[(size_t)d.bh + 2 * xx] + plan.coef[(size_t)d.bh + 2 * xx + 1] <= d.w);
    }
    if (d.flags & kGlyphVertical) {
      CHECK(d.kv >= 0 && d.bv == d.kv + d.out_h * d.ksize_v && (size_t)d.bv + 2 * (size_t)d.out_h <= plan.coef.size());
      for (int yy = 0; yy < d.out_h; yy++) CHECK(plan.coef[(size_t)d.bv + 2 * yy] >= 0 && plan.coef[(size_t)d.bv + 2 * yy + 1] <= d.ksize_v &&
                                                 plan.coef[(size_t)d.bv + 2 * yy] + plan.coef[(size_t)d.bv + 2 * yy + 1] <= d.h);
    }
    const bool both = (d.flags & kGlyphHorizontal) && (d.flags & kGlyphVertical);
    const bool big = both && (size_t)d.h * d.out_w > (size_t)kGlyphMidBytes;
    CHECK(((d.flags & kGlyphGlobalMid) != 0) == big);
    if (big) {
      CHECK(d.tmp % 16 == 0 && (size_t)d.tmp >= tmp_end && (size_t)d.tmp + (size_t)d.h * d.out_w <= plan.tmp_bytes);
      tmp_end = (size_t)d.tmp + (size_t)d.h * d.out_w;
    } else if (d.flags & kGlyphHorizontal) {
      CHECK((size_t)(both ? d.h : d.out_h) * d.out_w <= (size_t)kGlyphMidBytes);
    }
  }
  return 0;
}

int main() {
  // the fit: targets inside the canvas, status 2 exactly where a dimension would be 0
  for (int w = 1; w <= 1300; w += (w < 64 ? 1 : 17))
    for (int h = 1; h <= 1300; h += (h < 64 ? 1 : 13)) {
      const GlyphFit f = glyph_fit(w, h);
      if (f.status == kGlyphTooThin) { CHECK(h > 28 * w || w > 28 * h); continue; }
      CHECK(f.out_w >= 1 && f.out_w <= 28 && f.out_h >= 1 && f.out_h <= 28 && f.off_x + f.out_w <= 28 && f.off_y + f.out_h <= 28);
      CHECK(w == h ? (f.out_w == 28 && f.out_h == 28) : h > w ? f.out_h == 28 : f.out_w == 28);
    }
  CHECK(glyph_fit(0, 3).status == kGlyphTooThin && glyph_fit(3, -1).status == kGlyphTooThin && glyph_fit(65535, 65535).out_w == 28);
  CHECK(glyph_fit(1, 28).status == kGlyphOk && glyph_fit(1, 29).status == kGlyphTooThin && glyph_fit(65535, 1).status == kGlyphTooThin);
  // the tables
  for (int filter : {kFilterNearest, kFilterBicubic})
    for (int in : {1, 2, 3, 5, 27, 28, 29, 56, 57, 100, 333, 1170, 1171, 1300, 65535})
      for (int out = 1; out <= 28; out++) CHECK(check_table(filter, in, out) == 0);
  {
    std::vector<int32_t> kk(3, 1), bounds(3, 1);
    CHECK(resample_coeffs(1, 5, 5, kk, bounds) == 0 && kk.empty() && bounds.empty());
    CHECK(resample_coeffs(3, 0, 5, kk, bounds) == 0 && resample_coeffs(0, 5, 0, kk, bounds) == 0 && resample_coeffs(3, -4, 5, kk, bounds) == 0);
  }
  // validation
  {
    const int W = 50, H = 40;
    uint8_t px = 0, out = 0;
    const GlyphOpts good;
    const std::vector<int> on_edges = {0, 0, 50, 40, 0, 0, 1, 1, 49, 39, 50, 40, 0, 5, 7, 40, 45, 0, 50, 9, 0, 39, 50, 40, 49, 0, 50, 40};
    CHECK(validate_glyphs("t", &px, W, H, 3, 0, on_edges.data(), (int)on_edges.size() / 4, &good, &out).empty());
    CHECK(validate_glyphs("t", &px, W, H, 1, 0, nullptr, 0, &good, &out).empty());   // the whole picture
    CHECK(validate_glyphs("t", &px, W, H, 1, 0, nullptr, 7, &good, &out).empty());   // (boxes == nullptr: likewise, whatever the count)
    const int bad[][4] = {{-1, 0, 5, 5}, {0, -1, 5, 5}, {46, 0, 51, 5}, {0, 36, 5, 41}, {5, 5, 5, 9}, {5, 5, 9, 5}, {9, 5, 5, 9}, {5, 9, 9, 5},
                          {INT_MAX, 0, INT_MIN, 5}};
    for (const auto &b : bad)
      for (int pos : {0, 3}) {
        std::vector<int> boxes;
        for (int k = 0; k < pos; k++) boxes.insert(boxes.end(), {0, 0, 50, 40});
        boxes.insert(boxes.end(), b, b + 4);
        const std::string e = validate_glyphs("t", &px, W, H, 3, 0, boxes.data(), pos + 1, &good, &out);
        CHECK(e.find("box " + std::to_string(pos) + " ") != std::string::npos);
      }
    CHECK(!validate_glyphs("t", &px, W, H, 2, 0, nullptr, 0, &good, &out).empty());
    CHECK(!validate_glyphs("t", &px, W, H, 3, 149, nullptr, 0, &good, &out).empty() && validate_glyphs("t", &px, W, H, 3, 150, nullptr, 0, &good, &out).empty());
    CHECK(!validate_glyphs("t", nullptr, W, H, 3, 0, nullptr, 0, &good, &out).empty() && !validate_glyphs("t", &px, W, H, 3, 0, nullptr, 0, nullptr, &out).empty());
    CHECK(!validate_glyphs("t", &px, W, H, 3, 0, nullptr, 0, &good, nullptr).empty() && !validate_glyphs("t", &px, W, H, 3, 0, on_edges.data(), -1, &good, &out).empty());
    CHECK(!validate_glyphs("t", &px, 65536, H, 3, 0, nullptr, 0, &good, &out).empty() && !validate_glyphs("t", &px, W, 0, 3, 0, nullptr, 0, &good, &out).empty());
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    for (float f : {-1.f, -1e-30f, inf, -inf, nan}) {
      GlyphOpts o;
      o.contrast = f;
      CHECK(validate_glyphs("t", &px, W, H, 3, 0, nullptr, 0, &o, &out).find("contrast") != std::string::npos);
      o = GlyphOpts();
      o.brightness = f;
      CHECK(validate_glyphs("t", &px, W, H, 3, 0, nullptr, 0, &o, &out).find("brightness") != std::string::npos);
    }
    for (int t : {-2, 256, INT_MAX, INT_MIN}) {
      GlyphOpts o;
      o.threshold = t;
      CHECK(validate_glyphs("t", &px, W, H, 3, 0, nullptr, 0, &o, &out).find("threshold") != std::string::npos);
    }
    for (int f : {-1, 1, 2, 4, 5, INT_MAX}) {
      GlyphOpts o;
      o.filter = f;
      CHECK(validate_glyphs("t", &px, W, H, 3, 0, nullptr, 0, &o, &out).find("filter") != std::string::npos);
    }
    GlyphOpts o;
    o.contrast = 0.f; o.brightness = 0.f; o.threshold = 255; o.filter = 0;
    CHECK(validate_glyphs("t", &px, W, H, 3, 0, nullptr, 0, &o, &out).empty());
  }
  // plans
  {
    GlyphPlan plan;
    CHECK(check_plan({}, {}, 3, 0, plan) == 0 && plan.coef.empty() && plan.tmp_bytes == 0);
    // no ink; one pixel; square; too thin; a glyph already 28 high; two glyphs that share an axis
    const std::vector<int> boxes = {0, 0, 10, 10, 0, 0, 10, 10, 0, 0, 40, 40, 0, 0, 10, 100, 0, 0, 30, 40, 5, 5, 65, 35, 0, 0, 65, 65, 0, 0, 9, 300};
    const std::vector<int> found = {INT_MAX, INT_MAX, -1, -1, 3, 4, 3, 4, 10, 10, 29, 29, 4, 0, 4, 99, 3, 2, 12, 29, 5, 5, 64, 24, 0, 0, 59, 39, INT_MAX, INT_MAX, -1, -1};
    for (int filter : {0, 3})
      for (int sb : {0, 1}) {
        CHECK(check_plan(boxes, found, filter, sb, plan) == 0);
        const std::vector<int32_t> want = {kGlyphNoInk, kGlyphOk, kGlyphOk, kGlyphTooThin, kGlyphOk, kGlyphOk, kGlyphOk, kGlyphTooThin};
        CHECK(plan.status == want);
        CHECK(((plan.desc[1].flags & kGlyphBlank) != 0) == (sb == 1) && ((plan.desc[2].flags & kGlyphBlank) != 0) == (sb == 1));
        CHECK(plan.desc[4].out_h == 28 && !(plan.desc[4].flags & kGlyphVertical));  // 10 x 28: the height stays
        // glyphs 5 (60 x 20 -> 28 x 9) and 6 (60 x 40 -> 28 x 18): one horizontal table between them
        CHECK(plan.desc[5].kh == plan.desc[6].kh && plan.desc[5].bh == plan.desc[6].bh && plan.desc[5].kv != plan.desc[6].kv);
        CHECK(plan.tables == (sb ? 3 : 5));  // 1->28 and 20->28 once each (both axes of a square); 60->28, 20->9, 40->18
      }
    // an ink box outside its box is an internal error, named
    CHECK(plan_glyphs(boxes.data(), std::vector<int>{0, 0, 10, 5, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}.data(), 8, 3, 0, plan)
              .find("box 0") != std::string::npos);
    // both sides of the LDS budget (h x out_w bytes): a 1170 x 1170 ink box leaves 28 x 1170 = 32760 bytes in LDS, 1171 x
    // 1171 does not fit; 1250 x 1300 (26 x 1300) neither, 50 x 1300 (1 x 1300) easily; tall glyphs get disjoint pieces
    const std::vector<int> tall = {0, 0, 1170, 1170, 0, 0, 1171, 1171, 10, 0, 1260, 1300, 0, 0, 1300, 50, 0, 0, 50, 1300};
    const std::vector<int> tall_found = {0, 0, 1169, 1169, 0, 0, 1170, 1170, 10, 0, 1259, 1299, 0, 0, 1299, 49, 0, 0, 49, 1299};
    CHECK(check_plan(tall, tall_found, 3, 0, plan) == 0);
    CHECK(!(plan.desc[0].flags & kGlyphGlobalMid) && (plan.desc[1].flags & kGlyphGlobalMid) && (plan.desc[2].flags & kGlyphGlobalMid) &&
          !(plan.desc[3].flags & kGlyphGlobalMid) && !(plan.desc[4].flags & kGlyphGlobalMid));
    CHECK(plan.desc[2].out_w == 26 && plan.desc[4].out_w == 1);
    CHECK(plan.tmp_bytes >= (size_t)1171 * 28 + (size_t)1300 * 26);
    // 10^4 boxes of 97 x 89 sizes
    std::vector<int> many, many_found;
    for (int i = 0; i < 10000; i++) {
      const int k = (int)(((long)i * 7919) % 10000);
      const int w = 1 + k % 97, h = 1 + (k / 97) % 89, x = k % 13, y = k % 11;
      many.insert(many.end(), {x, y, x + w + 2, y + h + 1});
      if (k % 7 == 0) many_found.insert(many_found.end(), {INT_MAX, INT_MAX, -1, -1});
      else many_found.insert(many_found.end(), {x + 1, y, x + w, y + h - 1});
    }
    CHECK(check_plan(many, many_found, 3, 0, plan) == 0 && check_plan(many, many_found, 0, 1, plan) == 0);
  }
  std::printf("glyphs sanitize run ok\n");
  return 0;
}
