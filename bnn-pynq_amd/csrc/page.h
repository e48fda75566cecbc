// Host half of bnn_mi355x_order_lines / bnn_mi355x_page_to_mnist / bnn_mi355x_read_page: a page is read line by line,
// and every glyph's record holds that glyph's own ink alone.  The reference has no segmentation (its notebooks hold one
// glyph in front of the camera), so -- like the labelling (components.h) -- the model is this project's own, stated
// here once:
//
// Masked record (mask = 1).  Glyph g is a component that select_components returned.  Its picture is the enhanced L plane
//   with every pixel that does not belong to component g replaced by 255: other components, filtered components,
//   components beyond the cap, and background -- grey values in [ink_level, 255) included.  Steps 5-8 of classify_glyphs
//   (ink box, fit, resize, paste, record rule; glyphs.h) run on that picture with g's box as the box.  Every member pixel
//   is < ink_level <= 255, so the ink box IS the component's box (no k_glyph_bbox, no second round trip); status 1 (no
//   ink) cannot occur; status 2 (aspect above 28) and square_blank work as before.  mask = 0 is read_glyphs' crop rule:
//   whatever lies inside the box is part of the record.
//
// Lines (line_order = 1).  The input is the components kept by min_pixels, before the cap; each has its box (l, u, r, b)
//   and its first pixel f.
//   1  They are visited in ascending (u, f).
//   2  Each line has a band [top, bottom).  For a visited component of height h = b - u and each existing line, ov =
//      min(b, bottom) - max(u, top).  The component joins the line with the largest ov among the lines with 2 ov >=
//      min(h, bottom - top); on a tie the line created first.  The band's bottom becomes max(bottom, b); the top never
//      moves, because of the visiting order.  If no line qualifies the component opens a new line [u, b).
//   3  Lines are numbered in creation order, which is ascending top.
//   4  Inside a line the glyphs go in ascending (l, u, f).
//   5  The output order is line 0, then line 1, and so on; line[i] is the line of output glyph i.
//   6  gap[i] is 1 iff word_gap > 0, glyph i is not the first of its line, and l_i - max(r of the earlier glyphs of its
//      line) >= word_gap; else 0.
//   7  The cap takes the first min(cap, total) in that order.
//   8  More than kMaxLineComponents kept components are refused (raise min_pixels): the clustering is written the plain
//      way, components x lines.
//   Known limit: a dot above a stem is a line of its own unless reach_y joins it to the stem.
//   line_order = 0 keeps find->order; every line[i] and gap[i] is 0 then, and a word_gap above 0 is refused.
//
// This file is host-only (no HIP): the validation, order_lines, and the masked route's plan -- the selected components
// straight into GlyphDescs (plan_glyphs of glyphs.h, given each component's box as its own ink box) plus the per-glyph
// owner key.  csrc/page_kernels.hip holds the kernel, csrc/runtime.hip the entry points.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "components.h"
#include "glyphs.h"

namespace bnn {

constexpr int kMaxLineComponents = 65536;

struct PageOpts {  // (bnn_mi355x_page_opts)
  int mask = 1;
  int line_order = 1;
  int word_gap = 0;
};

// Empty when acceptable, else the message for last_error, worded like validate_find (components.h), which the entry
// points call first.
std::string validate_page(const char *what, const PageOpts *page);

// Empty when acceptable: the arguments of bnn_mi355x_order_lines (boxes: n x 4, first: n, order: n; all non-null).
std::string validate_order_lines(const char *what, const int *boxes, const int *first, int n, int word_gap, const int *order);

// The line model on `kept` (any order): order[i] = the index in `kept` of output glyph i, line[i] and gap[i] as above,
// n entries each.  Returns the message for last_error when there are more than kMaxLineComponents, else empty.
std::string order_lines(const std::vector<Component> &kept, int word_gap, std::vector<int32_t> &order, std::vector<int32_t> &line,
                        std::vector<int32_t> &gap);

// The masked route's plan from the chosen components, in their order: plan as plan_glyphs makes it with every box its
// own ink box, and keys[2 i ..] = {first pixel, -2 - id}: the two values the label plane holds for the pixels of
// component i after launch_cc_collect (component_kernels.h).  Returns the message for last_error, else empty.
std::string plan_page(const std::vector<Component> &chosen, int filter, int square_blank, GlyphPlan &plan, std::vector<int32_t> &keys);

}  // namespace bnn
