// see glyphs.h.  Compiled with -ffp-contract=off like resample.cpp: the fit rule is the notebooks' double arithmetic.
#include "glyphs.h"

#include <cmath>
#include <map>
#include <tuple>

#include "resample.h"

namespace bnn {

GlyphFit glyph_fit(int w, int h) {
  GlyphFit f;
  if (w < 1 || h < 1) {
    f.status = kGlyphTooThin;
    return f;
  }
  const double rh = 28. / h, rw = 28. / w;
  const double ratio = rw < rh ? rw : rh;  // Python's min(28. / h, 28. / w): the second only when it is smaller
  if (h == w) {
    f.out_w = f.out_h = kGlyphSide;
  } else if (h > w) {
    f.out_w = (int)(w * ratio);
    f.out_h = kGlyphSide;
  } else {
    f.out_w = kGlyphSide;
    f.out_h = (int)(h * ratio);
  }
  if (f.out_w < 1 || f.out_h < 1) {
    f.status = kGlyphTooThin;
    return f;
  }
  f.off_x = (kGlyphSide - f.out_w) / 2;  // int((28 - size) / 2), size <= 28
  f.off_y = (kGlyphSide - f.out_h) / 2;
  return f;
}

std::string validate_glyphs(const char *what, const void *pixels, int width, int height, int bands, long row_stride, const int *boxes,
                            int n_boxes, const GlyphOpts *opts, const void *out) {
  const std::string name = std::string(what) + ": ";
  if (n_boxes < 0) return name + "negative number of boxes";
  if (!pixels || !opts || !out) return name + "bad arguments (null pointer)";
  if (bands != 1 && bands != 3 && bands != 4) return name + "bands must be 1 (L), 3 (RGB) or 4 (RGBA) bytes per pixel";
  if (width < 1 || height < 1 || width > 65535 || height > 65535) return name + "need a picture of 1..65535 x 1..65535 pixels";
  if (row_stride != 0 && row_stride < (long)width * bands) return name + "row stride shorter than a row";
  if (!std::isfinite(opts->contrast) || opts->contrast < 0.f) return name + "contrast must be a finite factor of 0 or more";
  if (!std::isfinite(opts->brightness) || opts->brightness < 0.f) return name + "brightness must be a finite factor of 0 or more";
  if (opts->threshold < -1 || opts->threshold > 255) return name + "threshold must be -1 (none) or 0..255";
  if (opts->filter != kFilterNearest && opts->filter != kFilterBicubic) return name + "filter must be 0 (NEAREST) or 3 (BICUBIC)";
  for (int i = 0; boxes && i < n_boxes; i++) {
    const int *b = boxes + 4 * (size_t)i;
    const std::string box = "box " + std::to_string(i) + " (" + std::to_string(b[0]) + ", " + std::to_string(b[1]) + ", " +
                            std::to_string(b[2]) + ", " + std::to_string(b[3]) + ")";
    if (b[2] <= b[0] || b[3] <= b[1]) return name + box + " is empty or inverted (need right > left and lower > upper)";
    if (b[0] < 0 || b[1] < 0 || b[2] > width || b[3] > height)
      return name + box + " leaves the " + std::to_string(width) + " x " + std::to_string(height) + " picture";
  }
  return "";
}

std::string plan_glyphs(const int *boxes, const int *found, int n, int filter, int square_blank, GlyphPlan &plan) {
  plan.desc.assign((size_t)(n > 0 ? n : 0), GlyphDesc{});
  plan.status.assign(plan.desc.size(), kGlyphOk);
  plan.ink_boxes.assign(plan.desc.size() * 4, 0);
  plan.coef.clear();
  plan.tmp_bytes = 0;
  plan.tables = 0;
  // (filter, in, out) -> {offset of kk, offset of bounds, ksize}: an axis of one glyph often is an axis of another
  std::map<std::tuple<int, int, int>, std::tuple<int32_t, int32_t, int32_t>> tables;
  auto table = [&](int in, int out, int32_t &off_k, int32_t &off_b, int32_t &ksize) {
    const auto key = std::make_tuple(filter, in, out);
    auto it = tables.find(key);
    if (it == tables.end()) {
      std::vector<int32_t> kk, bounds;
      const int ks = resample_coeffs(filter, in, out, kk, bounds);
      const int32_t ok = (int32_t)plan.coef.size(), ob = ok + (int32_t)kk.size();
      plan.coef.insert(plan.coef.end(), kk.begin(), kk.end());
      plan.coef.insert(plan.coef.end(), bounds.begin(), bounds.end());
      it = tables.emplace(key, std::make_tuple(ok, ob, (int32_t)ks)).first;
      plan.tables++;
    }
    std::tie(off_k, off_b, ksize) = it->second;
  };
  for (int i = 0; i < n; i++) {
    const int *b = boxes + 4 * (size_t)i, *f = found + 4 * (size_t)i;
    int x0 = b[0], y0 = b[1], x1 = b[2], y1 = b[3];
    GlyphDesc &d = plan.desc[(size_t)i];
    int32_t &st = plan.status[(size_t)i];
    const bool ink = f[2] >= 0;
    if (ink) {
      if (f[0] < x0 || f[1] < y0 || f[2] >= x1 || f[3] >= y1 || f[0] > f[2] || f[1] > f[3])
        return "internal: the ink box of box " + std::to_string(i) + " does not lie inside it";
      x0 = f[0]; y0 = f[1]; x1 = f[2] + 1; y1 = f[3] + 1;
    } else {
      st = kGlyphNoInk;  // the whole box is the ink box; the record comes out with no ink
    }
    int32_t *ib = &plan.ink_boxes[4 * (size_t)i];
    ib[0] = x0; ib[1] = y0; ib[2] = x1; ib[3] = y1;
    d.x0 = x0; d.y0 = y0; d.w = x1 - x0; d.h = y1 - y0;
    const GlyphFit fit = glyph_fit(d.w, d.h);
    if (fit.status == kGlyphTooThin) {  // (a box without ink that is too thin as well: Pillow raises before anything is pasted)
      st = kGlyphTooThin;
      d.flags = kGlyphSkip;
      continue;
    }
    d.out_w = fit.out_w; d.out_h = fit.out_h; d.off_x = fit.off_x; d.off_y = fit.off_y;
    // a box without ink holds 255 alone: whatever is pasted is white, so nothing needs to be
    if (!ink || (square_blank && d.w == d.h)) {
      d.flags = kGlyphBlank;
      continue;
    }
    // (Image.resize runs the vertical pass first when h > 100 w and the height shrinks -- never here: out_w >= 1 needs
    // h <= 28 w)
    if (d.out_w != d.w) {
      d.flags |= kGlyphHorizontal;
      table(d.w, d.out_w, d.kh, d.bh, d.ksize_h);
    }
    if (d.out_h != d.h) {
      d.flags |= kGlyphVertical;
      table(d.h, d.out_h, d.kv, d.bv, d.ksize_v);
    }
    if ((d.flags & kGlyphHorizontal) && (d.flags & kGlyphVertical) && (size_t)d.h * d.out_w > (size_t)kGlyphMidBytes) {
      d.flags |= kGlyphGlobalMid;
      d.tmp = (int32_t)plan.tmp_bytes;
      plan.tmp_bytes += ((size_t)d.h * d.out_w + 15) & ~(size_t)15;
      if (plan.tmp_bytes > ((size_t)1 << 30)) return "more than 1 GiB of tall glyphs in one call (box " + std::to_string(i) + ")";
    }
  }
  return "";
}

}  // namespace bnn
