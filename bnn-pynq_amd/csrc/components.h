// Host half of bnn_mi355x_find_glyphs_host / bnn_mi355x_find_glyphs / bnn_mi355x_read_glyphs: the glyphs of a picture are
// the connected components of its ink.  The reference has no segmentation (its notebooks hold one glyph in front of the
// camera), so the model is this project's own, stated here once:
//
//   ink        a pixel of the enhanced L plane is ink iff its value is below ink_level (1..255; at 255 this is
//              k_glyph_bbox's rule "!= 255").  The 255-valued padding of the device plane past `width` is never ink.
//   adjacency  two different ink pixels are adjacent iff |dx| <= reach_x and |dy| <= reach_y (1..16 each).  The glyphs are
//              the connected components of that graph; at reach (1, 1) it is the 8-connectivity of
//              scipy.ndimage.label(ink, structure=np.ones((3, 3))).
//   component  its first pixel (the smallest index y * width + x of its pixels), its box (left, upper, right, lower;
//              right and lower exclusive, as Image.crop and classify_glyphs take boxes), its number of ink pixels.
//   filter     components of fewer than min_pixels ink pixels are dropped.
//   order      0: ascending first pixel (raster order); 1: ascending (left, upper, first pixel), the reading order of
//              one line.
//   cap        the first min(cap, total) components in that order are returned, together with total.
//   labels     (optional) int32 height x width: the index of the pixel's component in the returned order; -1 for
//              background, for filtered components and for components beyond the cap.
//
// This file is host-only (no HIP): the validation, a plain two-pass union-find labelling of an L plane (the model's
// statement, bnn_mi355x_find_glyphs_host), and select_components -- filter, order and cap, which the device path runs on
// the list it reads back, so that they exist once.  csrc/component_kernels.hip holds the kernels, csrc/runtime.hip the
// entry points.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace bnn {

// The largest picture that is labelled, in pixels: the device keeps an int32 label per pixel (64 MiB here), a second
// plane of the same size when the label map is asked for, and two lists of 32 bytes per possible component (one per
// 2 x 2 cell: 8 bytes per pixel each).
constexpr long kMaxComponentPixels = 1L << 24;
constexpr int kMaxReach = 16;

struct FindOpts {  // (bnn_mi355x_find_opts)
  int ink_level = 255;
  int reach_x = 1, reach_y = 1;
  int min_pixels = 1;
  int order = 0;  // kOrderRaster or kOrderLeft
};
constexpr int kOrderRaster = 0, kOrderLeft = 1;

// one component, as the device's lists hold it: 8 ints, 32 bytes
struct Component {
  int32_t first;                       // y * width + x of its first pixel
  int32_t left, upper, right, lower;   // right and lower exclusive
  int32_t pixels;
  int32_t id;                          // the device's number of its root (arrival order: means nothing); host: as first
  int32_t pad;
};

// Components never outnumber the 2 x 2 cells of the picture: with a reach of 1 or more in both directions the ink pixels
// of one cell are mutually adjacent.  Isolated pixels on every second row and column reach the bound.
inline size_t max_components(int width, int height) { return (size_t)((width + 1) / 2) * (size_t)((height + 1) / 2); }

// Empty when the call is acceptable, else the message for last_error, worded like validate_glyphs (glyphs.h), which the
// entry points call first for the picture itself.  `boxes` is the caller's cap x 4 output.
std::string validate_find(const char *what, int width, int height, const FindOpts *find, const void *boxes, int cap);

// Two-pass union-find over the plane (rows `row_stride` bytes apart, 0: width): every component, in ascending order of
// its first pixel, id = first.  roots (may be null): width x height ints, the first pixel of the pixel's component, -1
// for background.
void label_components(const uint8_t *plane, int width, int height, long row_stride, const FindOpts &find, std::vector<Component> &all,
                      std::vector<int32_t> *roots);

// Filter, order and cap: `chosen` = the first min(cap, total) of the components of `all` (any order) with min_pixels or
// more pixels, in find.order; returns total.  The index of a component in `chosen` is its label.
long select_components(const std::vector<Component> &all, const FindOpts &find, int cap, std::vector<Component> &chosen);

// The whole of bnn_mi355x_find_glyphs_host behind its validation; boxes: cap x 4, pixel_counts (cap) and labels (width x
// height) may be null.  Returns total.
long find_components_host(const uint8_t *plane, int width, int height, long row_stride, const FindOpts &find, int *boxes, int *pixel_counts,
                          int32_t *labels, int cap);

}  // namespace bnn
