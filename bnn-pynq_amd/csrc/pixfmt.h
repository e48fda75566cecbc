// Pixel formats of a clip's frames (bnn_mi355x_unpack_frames*, bnn_mi355x_*_clip_frames, bnn_mi355x_*_clip_device): frames as a
// camera or a decoder delivers them become the packed RGB frames the clip scan reads ("Camera frames").
//
//   RGB, L   the `bands` 3 and 1 of the older entry points.
//   BGR      3 bytes a pixel, reversed.
//   NV12     a Y plane of `height` rows at row_stride, then interleaved Cb Cr of height / 2 rows at the same stride.
//   I420     a Y plane, then a Cb plane of height / 2 rows at row_stride / 2, then a Cr plane likewise.
//   YUYV     Y0 Cb Y1 Cr, 2 bytes a pixel.
// Chroma is replicated to the 2 x 2 (NV12, I420) or 2 x 1 (YUYV) pixels it covers: no interpolation.
//
// Colour.  range 0 is JFIF full range, byte for byte Pillow's convert("RGB") from mode YCbCr: four tables
// T_c[i] = (int)(c * 64 * (i - 128) + 0.5) for c = 1.402, -0.34414, -0.71414, 1.772 and
//   R = clip8(Y + (T_1.402[Cr] >> 6)), G = clip8(Y + ((T_-.34414[Cb] + T_-.71414[Cr]) >> 6)), B = clip8(Y + (T_1.772[Cb] >> 6)).
// range 1 is BT.601 video range, the project's own statement (parity unpinned): with C = Y - 16, D = Cb - 128, E = Cr - 128
//   R = clip8((298 C + 409 E + 128) >> 8), G = clip8((298 C - 100 D - 208 E + 128) >> 8), B = clip8((298 C + 516 D + 128) >> 8).
// Every shift is arithmetic.  The model is pure integer, so the kernel (csrc/pixfmt_kernels.hip) is pinned to it byte for
// byte; tests/pixfmt_ref.py restates it in numpy.  Host-only but for the BNN_HD routines, which the kernel shares (as
// ecc.h and detect.h).  No HIP in this file.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>

#ifndef BNN_HD
#define BNN_HD
#endif

namespace bnn {

enum PixFormat : int { PIX_RGB = 0, PIX_L = 1, PIX_BGR = 2, PIX_NV12 = 3, PIX_I420 = 4, PIX_YUYV = 5, PIX_FORMATS = 6 };

// Limits (include/bnn_mi355x.h states them): a side, the frames of one call, and the bytes of the raw frames and of the
// RGB frames, each
constexpr int kPixMaxSide = 8192;
constexpr int kPixMaxFrames = 4096;
constexpr size_t kPixMaxBytes = (size_t)1 << 30;

struct Frames {  // (bnn_mi355x_frames)
  int format, range, width, height, n_frames;
  long row_stride, frame_stride;  // bytes; 0: packed
};

// Where the bytes of validated frames lie: a row of the first plane, the rows of one frame counted in strides (NV12 and
// I420: the chroma planes take height / 2 strides), and the strides with 0 resolved
struct PixLayout {
  int n_frames = 0, rows = 0;
  size_t row_bytes = 0, rows_apart = 0, frame_span = 0, frames_apart = 0;
  size_t total() const { return frames_apart * (size_t)(n_frames - 1) + frame_span; }  // bytes from the first frame to past the last
};

BNN_HD constexpr bool pix_is_yuv(int format) { return format == PIX_NV12 || format == PIX_I420 || format == PIX_YUYV; }
BNN_HD constexpr bool pix_is_420(int format) { return format == PIX_NV12 || format == PIX_I420; }
inline int pix_row_bytes(int format, int width) { return width * (format == PIX_L || pix_is_420(format) ? 1 : format == PIX_YUYV ? 2 : 3); }
const char *pix_format_name(int format);

// T_c[v] of the header comment in integers, c100k = c * 64 * 100000: c * 64 * (v - 128) + 0.5 is never closer than 1.6e-4 to
// an integer for the four coefficients, so the truncating division is the table's (int) cast (tests/test_pixfmt_host.py
// compares all 1024 entries with the floating-point statement)
BNN_HD inline int pix_jfif_term(int c100k, int v) { return (c100k * (v - 128) + 50000) / 100000; }

// what a chroma sample adds to each channel, before the luma
struct PixChroma { int r, g, b; };
BNN_HD inline PixChroma pix_chroma(int range, int cb, int cr) {
  PixChroma c;
  if (range == 0) {
    c.r = pix_jfif_term(8972800, cr) >> 6;
    c.g = (pix_jfif_term(-2202496, cb) + pix_jfif_term(-4570496, cr)) >> 6;
    c.b = pix_jfif_term(11340800, cb) >> 6;
  } else {
    const int d = cb - 128, e = cr - 128;
    c.r = 409 * e;
    c.g = -100 * d - 208 * e;
    c.b = 516 * d;
  }
  return c;
}
BNN_HD inline int pix_clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }
BNN_HD inline int pix_channel(int range, int y, int c) { return pix_clip8(range == 0 ? y + c : (298 * (y - 16) + c + 128) >> 8); }

// The RGB of pixel (x, y) of ONE frame that starts at f, byte by byte (the host loop, and the kernel's path for row
// tails and for bases and strides its wide accesses cannot take).  Reads only inside the planes' `width` columns.
BNN_HD inline void pix_unpack_one(int format, const uint8_t *f, size_t stride, int height, int range, int x, int y, uint8_t *rgb) {
  if (format == PIX_RGB || format == PIX_BGR) {
    const uint8_t *p = f + (size_t)y * stride + (size_t)x * 3;
    const int swap = format == PIX_BGR ? 2 : 0;
    rgb[0] = p[swap]; rgb[1] = p[1]; rgb[2] = p[2 - swap];
    return;
  }
  if (format == PIX_L) {
    rgb[0] = rgb[1] = rgb[2] = f[(size_t)y * stride + x];
    return;
  }
  int luma, cb, cr;
  if (format == PIX_YUYV) {
    const uint8_t *p = f + (size_t)y * stride + (size_t)(x & ~1) * 2;
    luma = p[(x & 1) * 2]; cb = p[1]; cr = p[3];
  } else {
    luma = f[(size_t)y * stride + x];
    if (format == PIX_NV12) {
      const uint8_t *p = f + (size_t)(height + (y >> 1)) * stride + (x & ~1);
      cb = p[0]; cr = p[1];
    } else {
      const size_t half = stride / 2;
      const uint8_t *p = f + (size_t)height * stride + (size_t)(y >> 1) * half + (x >> 1);
      cb = p[0]; cr = p[(size_t)(height / 2) * half];
    }
  }
  const PixChroma c = pix_chroma(range, cb, cr);
  rgb[0] = (uint8_t)pix_channel(range, luma, c.r);
  rgb[1] = (uint8_t)pix_channel(range, luma, c.g);
  rgb[2] = (uint8_t)pix_channel(range, luma, c.b);
}

// Empty when the frames can be unpacked, else the message for last_error (`what`: the entry point's name), naming the
// argument.  Refused, in this order: null pointers; an unknown format or range; a side outside 1 .. kPixMaxSide; an odd
// width (NV12, I420, YUYV) or height (NV12, I420); n_frames outside 1 .. kPixMaxFrames; a row stride shorter than a row
// or, for I420, odd; a frame stride shorter than a frame; raw or RGB bytes above kPixMaxBytes.  `layout` is set on success.
std::string validate_frames(const char *what, const Frames *frames, const void *pixels, PixLayout &layout);

// The model on validated frames: packed RGB [n_frames][height][width][3]
void unpack_frames(const Frames &frames, const PixLayout &layout, const uint8_t *pixels, uint8_t *rgb);

}  // namespace bnn
