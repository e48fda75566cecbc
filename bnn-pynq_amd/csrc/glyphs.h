// Host half of bnn_mi355x_enhance_picture / bnn_mi355x_glyphs_to_mnist / bnn_mi355x_classify_glyphs: one picture and N
// boxes become N MNIST-format records (28 x 28 bytes) on the device.  The reference does this by hand, per camera frame,
// in LFC-BNN_MNIST_Webcam.ipynb and LFC-BNN_Chars_Webcam.ipynb (cells 9-13): greyscale, ImageEnhance.Contrast and
// .Brightness, an optional hard threshold, the bounding box of the ink, Image.resize of the crop into 28 x 28 keeping the
// aspect ratio, a centred paste on white, and 255 / 1 per pixel.  DESIGN.md 9 restates every step in integer / IEEE form.
//
// This file is host-only (no HIP): the validation of the caller's arguments, the fit rule, and the plan the one host
// round trip of a call builds from the ink boxes the device found -- one descriptor per glyph and the coefficient tables
// (resample.h: resample_coeffs), each (filter, in, out) table once however many glyphs and axes share it.
// csrc/glyph_kernels.hip holds the kernels, csrc/runtime.hip the entry points.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace bnn {

constexpr int kGlyphSide = 28;
constexpr int kGlyphRecord = kGlyphSide * kGlyphSide;  // 784 bytes, 49 x 16
// LDS budget of the record kernel: the horizontal pass's 8-bit output, h x out_w <= h x 28 bytes, stays in LDS for the
// vertical pass (the budget of the window kernel, windows.h).  Taller ink boxes (h > 1170 at out_w = 28) keep it in a
// global temporary.
constexpr int kGlyphMidBytes = 32768;

struct GlyphOpts {  // (bnn_mi355x_glyph_opts)
  float contrast = 3.f, brightness = 4.f;
  int threshold = -1;   // -1: none; else v > threshold ? 255 : 0
  int filter = 3;       // resample.h: kFilterBicubic (3) or kFilterNearest (0)
  int square_blank = 0; // 1: a square ink box gives a blank record, as the notebooks do (they forget the paste)
};

// status of a glyph
constexpr int kGlyphOk = 0, kGlyphNoInk = 1, kGlyphTooThin = 2;

struct GlyphFit {
  int out_w = 0, out_h = 0;  // Image.resize's target; 0 in a dimension: status 2
  int off_x = 0, off_y = 0;  // where the paste puts it on the 28 x 28 canvas
  int status = kGlyphOk;     // kGlyphOk or kGlyphTooThin
};

// Cell 11 for a (w, h) ink box: ratio = min(28. / h, 28. / w) in doubles, square -> (28, 28), taller -> (int(w * ratio),
// 28), wider -> (28, int(h * ratio)); paste at (int((28 - out_w) / 2), int((28 - out_h) / 2)).  An output dimension of 0
// (aspect above 28) is kGlyphTooThin: Pillow raises ValueError there.
GlyphFit glyph_fit(int w, int h);

// Empty when the call is acceptable, else the message for last_error, worded like validate_windows (windows.h).  n_boxes
// == 0 or boxes == nullptr: the whole picture is the one box.  `out` is the caller's output buffer (any non-null pointer
// for an entry point that has none).  Refused besides what validate_windows refuses: factors that are not finite or are
// negative, a threshold outside -1..255, a filter other than 0 / 3.
std::string validate_glyphs(const char *what, const void *pixels, int width, int height, int bands, long row_stride, const int *boxes,
                            int n_boxes, const GlyphOpts *opts, const void *out);

// one glyph as the record kernel reads it: 16 ints, 64 bytes
struct GlyphDesc {
  int32_t x0, y0, w, h;      // the ink box in the picture (left, upper, width, height)
  int32_t out_w, out_h;      // 1..28 each
  int32_t off_x, off_y;      // the paste
  int32_t kh, bh, ksize_h;   // horizontal tables: offsets into the coefficient buffer (int32 units), taps per row
  int32_t kv, bv, ksize_v;   // vertical
  int32_t flags;             // kGlyph* bits below
  int32_t tmp;               // kGlyphGlobalMid: this glyph's bytes in the global temporary (offset, 16-byte aligned)
};
constexpr int kGlyphHorizontal = 1, kGlyphVertical = 2;  // the passes Pillow runs (out_w != w, out_h != h)
constexpr int kGlyphBlank = 4;      // nothing is pasted: no ink, or a square ink box under square_blank
constexpr int kGlyphSkip = 8;       // status 2: the record is not written
constexpr int kGlyphGlobalMid = 16; // the horizontal pass's output exceeds kGlyphMidBytes

struct GlyphPlan {
  std::vector<GlyphDesc> desc;     // one per box, in the caller's order
  std::vector<int32_t> status;     // kGlyphOk / kGlyphNoInk / kGlyphTooThin
  std::vector<int32_t> ink_boxes;  // n x 4 (left, upper, right, lower) in picture coordinates, as Image.crop takes them
  std::vector<int32_t> coef;       // all tables, one upload
  size_t tmp_bytes = 0;            // the global temporary the call needs
  int tables = 0;                  // distinct (filter, in, out) tables in coef
};

// Builds the plan from the n boxes and what k_glyph_bbox found in them: found[4 i ..] = {min x, min y, max x, max y} of
// the pixels != 255 in picture coordinates, {INT_MAX, INT_MAX, -1, -1} for a box without ink.  Returns the message for
// last_error when a found box does not lie inside its box (nothing the caller can cause), else empty.
std::string plan_glyphs(const int *boxes, const int *found, int n, int filter, int square_blank, GlyphPlan &plan);

}  // namespace bnn
