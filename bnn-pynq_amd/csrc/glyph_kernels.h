// Device half of enhance_picture / glyphs_to_mnist / classify_glyphs (see glyphs.h): picture -> L plane and its pixel
// sum, contrast / brightness / threshold in place, the ink box of every box, and one MNIST-format record per glyph.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "glyphs.h"

namespace bnn {

// The picture on the device: rows `src_pitch` = bands * plane_pitch bytes apart; the L plane: rows `plane_pitch` bytes
// apart, plane_pitch = width rounded up to 16.  Both buffers 16-byte aligned, so that a thread's 16 pixels are whole
// 16-byte lanes of either.
inline long glyph_plane_pitch(int width) { return ((long)width + 15) & ~15L; }

struct GlyphPicture {
  const uint8_t *src;  // height x src_pitch (device)
  uint8_t *plane;      // height x plane_pitch (device)
  int width, height, bands;
  long plane_pitch;
  unsigned long long *sum;  // the sum of the L plane's width x height pixels (device; zeroed by the caller before k_glyph_luma)
};

// src -> plane (bytes past `width` in a row: 255), *sum += the pixels
hipError_t launch_glyph_luma(const GlyphPicture &p, hipStream_t s);
// steps 2-4 in place, m = floor((2 *sum + n) / (2 n)); the caller launches it only when a step is not the identity
hipError_t launch_glyph_enhance(const GlyphPicture &p, float contrast, float brightness, int threshold, hipStream_t s);
// found[4 i ..] = {min x, min y, max x, max y} over the pixels != 255 of box i; the caller has set them to {INT_MAX,
// INT_MAX, -1, -1}.  boxes: n x 4 ints, 16-byte aligned (device).
hipError_t launch_glyph_bbox(const GlyphPicture &p, const int32_t *boxes, int32_t *found, int n, int max_box_height, hipStream_t s);
// record i at records + i * 784 (16-byte aligned) from desc[i] and the tables in coef; tmp: plan.tmp_bytes (may be null
// when that is 0)
hipError_t launch_glyph_record(const GlyphPicture &p, const GlyphDesc *desc, const int32_t *coef, uint8_t *tmp, uint8_t *records, int n,
                               hipStream_t s);

}  // namespace bnn
