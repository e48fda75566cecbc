// Device half of find_glyphs_clip / clip_to_mnist / read_clip (see clip_glyphs.h): a clip of F frames as ONE tall L plane
// of width x (F * height) pixels -- frame f in rows [f * height, (f + 1) * height) -- enhanced frame by frame, and its
// ink labelled tile by tile in LDS, the tiles' borders merged afterwards.  Behind the labelling the tall plane and the
// tall label map go through launch_cc_collect / launch_cc_relabel (component_kernels.h) and the record kernels
// (glyph_kernels.h, page_kernels.h) unchanged: a component never spans two frames.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "clip_glyphs.h"
#include "component_kernels.h"
#include "glyph_kernels.h"

namespace bnn {

// k_clip_cc_tile: the tile's 2 048 labels and its 32 ink words
constexpr int kClipTileLdsBytes = kClipTileW * kClipTileH * 4 + kClipTileH * 8;

struct ClipGlyphPlane {
  GlyphPicture tall;   // src, plane and width as glyph_kernels.h; height = frames * frame_height; sum: one per FRAME
  int frames, frame_height;
};

struct ClipComponentPlane {
  ComponentPlane tall;  // as component_kernels.h with height = frames * frame_height; words_per_row = tiles_x
  int frames, frame_height;
  int tiles_x, tiles_y;  // tiles of ONE frame (clip_glyphs.h)
};

// k_clip_luma and -- when `enhance` -- k_clip_enhance: src -> plane (bytes past `width` in a row: 255), sum[f] += the
// pixels of frame f (zeroed by the caller), then contrast / brightness / threshold in place with frame f's own mean
// m = floor((2 sum[f] + n) / (2 n)), n = width * frame_height
hipError_t launch_clip_plane(const ClipGlyphPlane &p, bool enhance, float contrast, float brightness, int threshold, hipStream_t s);
// k_clip_cc_tile, then (more than one tile a frame) k_clip_cc_seams and k_clip_cc_flatten: afterwards bits[] holds the ink
// words and label[] satisfies launch_cc_collect's contract -- a component's pixels hold its first (smallest) pixel in
// tall coordinates, background -1 -- with no adjacency across a frame's first or last row
hipError_t launch_clip_cc_label(const ClipComponentPlane &c, int ink_level, int reach_x, int reach_y, hipStream_t s);

}  // namespace bnn
