// Host half of the pixel formats: see pixfmt.h.
#include "pixfmt.h"

namespace bnn {

const char *pix_format_name(int format) {
  static const char *const names[PIX_FORMATS] = {"RGB", "L", "BGR", "NV12", "I420", "YUYV"};
  return format >= 0 && format < PIX_FORMATS ? names[format] : "?";
}

std::string validate_frames(const char *what, const Frames *frames, const void *pixels, PixLayout &layout) {
  const std::string name = std::string(what) + ": ";
  layout = PixLayout{};
  if (!frames) return name + "frames is null";
  if (!pixels) return name + "pixels is null";
  const Frames &f = *frames;
  if (f.format < 0 || f.format >= PIX_FORMATS)
    return name + "format must be 0 (RGB), 1 (L), 2 (BGR), 3 (NV12), 4 (I420) or 5 (YUYV), got " + std::to_string(f.format);
  const std::string fmt = pix_format_name(f.format);
  if (f.range != 0 && f.range != 1) return name + "range must be 0 (JFIF full range) or 1 (BT.601 video range), got " + std::to_string(f.range);
  if (f.width < 1 || f.width > kPixMaxSide) return name + "width must be 1 to " + std::to_string(kPixMaxSide) + ", got " + std::to_string(f.width);
  if (f.height < 1 || f.height > kPixMaxSide) return name + "height must be 1 to " + std::to_string(kPixMaxSide) + ", got " + std::to_string(f.height);
  if (pix_is_yuv(f.format) && (f.width & 1)) return name + "width must be even for " + fmt + ", got " + std::to_string(f.width);
  if (pix_is_420(f.format) && (f.height & 1)) return name + "height must be even for " + fmt + ", got " + std::to_string(f.height);
  if (f.n_frames < 1 || f.n_frames > kPixMaxFrames)
    return name + "n_frames must be 1 to " + std::to_string(kPixMaxFrames) + ", got " + std::to_string(f.n_frames);
  PixLayout l;
  l.n_frames = f.n_frames;
  l.row_bytes = (size_t)pix_row_bytes(f.format, f.width);
  l.rows = pix_is_420(f.format) ? f.height / 2 * 3 : f.height;
  if (f.row_stride != 0 && (f.row_stride < 0 || (size_t)f.row_stride < l.row_bytes)) return name + "row_stride shorter than a row of " + fmt;
  l.rows_apart = f.row_stride ? (size_t)f.row_stride : l.row_bytes;
  if (f.format == PIX_I420 && (l.rows_apart & 1)) return name + "row_stride must be even for I420 (the chroma rows lie half of it apart)";
  // (the strides are bounded before they are multiplied: at most 2^30 x 12288 rows, 2^30 x 4096 frames)
  const std::string over = name + "the frames take more than the limit of " + std::to_string(kPixMaxBytes) + " bytes";
  if (l.rows_apart > kPixMaxBytes) return over;
  l.frame_span = l.rows_apart * (size_t)l.rows;
  if (f.frame_stride != 0 && (f.frame_stride < 0 || (size_t)f.frame_stride < l.frame_span)) return name + "frame_stride shorter than a frame";
  l.frames_apart = f.frame_stride ? (size_t)f.frame_stride : l.frame_span;
  if (l.frames_apart > kPixMaxBytes || l.total() > kPixMaxBytes) return over;
  const size_t rgb = (size_t)f.width * f.height * 3 * (size_t)f.n_frames;
  if (rgb > kPixMaxBytes) return name + "the RGB frames take " + std::to_string(rgb) + " bytes, more than the limit of " + std::to_string(kPixMaxBytes);
  layout = l;
  return "";
}

void unpack_frames(const Frames &f, const PixLayout &l, const uint8_t *pixels, uint8_t *rgb) {
  for (int n = 0; n < f.n_frames; n++) {
    const uint8_t *frame = pixels + (size_t)n * l.frames_apart;
    uint8_t *out = rgb + (size_t)n * f.width * f.height * 3;
    for (int y = 0; y < f.height; y++)
      for (int x = 0; x < f.width; x++) pix_unpack_one(f.format, frame, l.rows_apart, f.height, f.range, x, y, out + ((size_t)y * f.width + x) * 3);
  }
}

}  // namespace bnn
