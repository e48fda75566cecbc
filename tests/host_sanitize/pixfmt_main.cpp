// Stand-alone driver for tests/test_host_sanitize_pixfmt.py: the host-only code of the pixel formats (csrc/pixfmt.cpp:
// validation and the model's loop) under AddressSanitizer + UBSan.  The small frames of tests/test_pixfmt_host.py -- every
// format, widths 2, 4, 6, 34 and 66, heights 2 and 6, 3 frames, padded strides, both ranges -- with source and destination
// in heap blocks of exactly the bytes the layout states, so that a read or a write one byte outside is caught; every pixel
// is compared with a restatement of the header's words (the floating-point tables), then the refusals.
#include <cstdint>
#include <cstdio>
#include <memory>
#include <random>
#include <string>

#include "pixfmt.h"

using namespace bnn;

#define CHECK(x) do { if (!(x)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

static bool has(const std::string &s, const char *what) { return s.find(what) != std::string::npos; }
static int clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// the header's statement of one pixel, with the tables computed in floating point
static void expect(int range, int y, int cb, int cr, int *rgb) {
  if (range == 0) {
    const auto t = [](double c, int i) { return (int)(c * 64 * (i - 128) + 0.5); };
    rgb[0] = clip8(y + (t(1.402, cr) >> 6));
    rgb[1] = clip8(y + ((t(-0.34414, cb) + t(-0.71414, cr)) >> 6));
    rgb[2] = clip8(y + (t(1.772, cb) >> 6));
  } else {
    const int c = y - 16, d = cb - 128, e = cr - 128;
    rgb[0] = clip8((298 * c + 409 * e + 128) >> 8);
    rgb[1] = clip8((298 * c - 100 * d - 208 * e + 128) >> 8);
    rgb[2] = clip8((298 * c + 516 * d + 128) >> 8);
  }
}

static int run_case(std::mt19937 &rng, int format, int range, int w, int h, int frames, long row_stride, long frame_stride) {
  const Frames f{format, range, w, h, frames, row_stride, frame_stride};
  PixLayout l;
  int probe = 0;
  CHECK(validate_frames("t", &f, &probe, l).empty());
  const size_t total = l.total(), out_bytes = (size_t)w * h * 3 * frames;
  std::unique_ptr<uint8_t[]> src(new uint8_t[total]), out(new uint8_t[out_bytes]);
  for (size_t i = 0; i < total; i++) src[i] = (uint8_t)rng();
  for (size_t i = 0; i < out_bytes; i++) out[i] = 0x5A;
  unpack_frames(f, l, src.get(), out.get());
  const size_t S = l.rows_apart;
  for (int n = 0; n < frames; n++)
    for (int y = 0; y < h; y++)
      for (int x = 0; x < w; x++) {
        const uint8_t *p = src.get() + (size_t)n * l.frames_apart, *got = out.get() + (((size_t)n * h + y) * w + x) * 3;
        int want[3];
        if (format == PIX_RGB || format == PIX_BGR) {
          for (int c = 0; c < 3; c++) want[c] = p[(size_t)y * S + 3 * x + (format == PIX_BGR ? 2 - c : c)];
        } else if (format == PIX_L) {
          want[0] = want[1] = want[2] = p[(size_t)y * S + x];
        } else if (format == PIX_YUYV) {
          const uint8_t *q = p + (size_t)y * S + 4 * (x / 2);
          expect(range, q[2 * (x % 2)], q[1], q[3], want);
        } else if (format == PIX_NV12) {
          const uint8_t *q = p + (size_t)(h + y / 2) * S + 2 * (x / 2);
          expect(range, p[(size_t)y * S + x], q[0], q[1], want);
        } else {
          const uint8_t *cb = p + (size_t)h * S + (size_t)(y / 2) * (S / 2) + x / 2;
          expect(range, p[(size_t)y * S + x], cb[0], cb[(size_t)(h / 2) * (S / 2)], want);
        }
        CHECK(got[0] == want[0] && got[1] == want[1] && got[2] == want[2]);
      }
  return 0;
}

int main() {
  std::mt19937 rng(2025);
  // all 1024 table entries: the integer statement of pixfmt.h is the floating-point one
  const double coeffs[4] = {1.402, -0.34414, -0.71414, 1.772};
  const int c100k[4] = {8972800, -2202496, -4570496, 11340800};
  for (int k = 0; k < 4; k++)
    for (int i = 0; i < 256; i++) CHECK(pix_jfif_term(c100k[k], i) == (int)(coeffs[k] * 64 * (i - 128) + 0.5));

  const int widths[] = {2, 4, 6, 34, 66}, heights[] = {2, 6};
  int cases = 0;
  for (int format = 0; format < PIX_FORMATS; format++)
    for (int w : widths)
      for (int h : heights)
        for (int range = 0; range < 2; range++) {
          const long rb = pix_row_bytes(format, w);
          // packed; a wider row stride (odd where the format allows it) and a frame stride with a gap
          if (run_case(rng, format, range, w, h, 3, 0, 0)) return 1;
          const long stride = pix_is_420(format) ? rb + 6 : rb + 5 + (rb % 2);
          const long rows = pix_is_420(format) ? h / 2 * 3 : h;
          if (run_case(rng, format, range, w, h, 3, stride, stride * rows + 7)) return 1;
          if (run_case(rng, format, range, w, h, 1, stride, 0)) return 1;
          cases += 3;
        }

  // the refusals, each naming its argument
  PixLayout l;
  int probe = 0;
  const auto refused = [&](Frames f, const char *word) { return has(validate_frames("t", &f, &probe, l), word); };
  CHECK(has(validate_frames("t", nullptr, &probe, l), "frames is null"));
  {
    const Frames f{PIX_NV12, 0, 4, 4, 1, 0, 0};
    CHECK(has(validate_frames("t", &f, nullptr, l), "pixels is null"));
  }
  CHECK(refused(Frames{PIX_FORMATS, 0, 4, 4, 1, 0, 0}, "format") && refused(Frames{-1, 0, 4, 4, 1, 0, 0}, "format"));
  CHECK(refused(Frames{PIX_NV12, 2, 4, 4, 1, 0, 0}, "range"));
  CHECK(refused(Frames{PIX_NV12, 0, 5, 4, 1, 0, 0}, "width") && refused(Frames{PIX_I420, 0, 5, 4, 1, 0, 0}, "width") &&
        refused(Frames{PIX_YUYV, 0, 5, 4, 1, 0, 0}, "width"));
  CHECK(refused(Frames{PIX_NV12, 0, 4, 5, 1, 0, 0}, "height") && refused(Frames{PIX_I420, 0, 4, 5, 1, 0, 0}, "height"));
  CHECK(validate_frames("t", std::unique_ptr<Frames>(new Frames{PIX_YUYV, 0, 4, 5, 1, 0, 0}).get(), &probe, l).empty());
  CHECK(refused(Frames{PIX_I420, 0, 4, 4, 1, 7, 0}, "row_stride") && refused(Frames{PIX_NV12, 0, 4, 4, 1, 3, 0}, "row_stride") &&
        refused(Frames{PIX_BGR, 0, 4, 4, 1, -12, 0}, "row_stride"));
  CHECK(refused(Frames{PIX_NV12, 0, 4, 4, 2, 8, 47}, "frame_stride") && refused(Frames{PIX_NV12, 0, 4, 4, 2, 0, -1}, "frame_stride"));
  CHECK(refused(Frames{PIX_NV12, 0, 4, 4, 0, 0, 0}, "n_frames") && refused(Frames{PIX_NV12, 0, 4, 4, kPixMaxFrames + 1, 0, 0}, "n_frames"));
  CHECK(refused(Frames{PIX_NV12, 0, 0, 4, 1, 0, 0}, "width") && refused(Frames{PIX_NV12, 0, 4, kPixMaxSide + 2, 1, 0, 0}, "height"));
  // strides near the top of `long`: refused by the limit, no overflow on the way
  CHECK(refused(Frames{PIX_BGR, 0, 4, 4, 2, INT64_MAX, 0}, "limit") && refused(Frames{PIX_BGR, 0, 4, 4, 2, 0, INT64_MAX}, "limit"));
  CHECK(refused(Frames{PIX_RGB, 0, kPixMaxSide, kPixMaxSide, 6, 0, 0}, "limit"));
  std::printf("pixfmt sanitize run ok: %d cases\n", cases);
  return 0;
}
