// Host half of bnn_mi355x_find_glyphs_clip / bnn_mi355x_clip_to_mnist / bnn_mi355x_read_clip: the glyphs of every frame of
// a clip in one set of launches.  The model is find_glyphs' and read_page's (components.h, page.h) applied to each frame
// alone; what is stated here is how a clip becomes ONE picture:
//
//   tall plane  F frames of width x height become an L plane of width x (F * height), pitch glyph_plane_pitch(width);
//               frame f occupies rows [f * height, (f + 1) * height).  A pixel's label index is y * width + x with y the
//               tall row.
//   frames      three things know about them: the contrast step blends with the mean of the frame's own pixels; two ink
//               pixels of different frames are never adjacent, whatever reach_y; and the component list is split by
//               frame = first / (width * height).  A component never spans two frames, so its box and first pixel lie
//               inside one frame, and everything behind the labelling runs on the tall plane unchanged.
//   tiles       the labelling works on tiles of kClipTileW x kClipTileH pixels of one frame (clip_glyph_kernels.hip); the
//               last tile row of a frame is short, no tile straddles a frame.
//   per frame   filter, order (find->order, or the line model when line_order is set) and cap as for one picture; boxes
//               are returned in FRAME coordinates (rows minus f * height).  order_lines' limit of kMaxLineComponents
//               applies per frame.
//
// This file is host-only (no HIP): the geometry, the limits with their refusals, and the split of the compacted list.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "components.h"
#include "page.h"

namespace bnn {

constexpr int kClipGlyphMaxFrames = 4096;
constexpr int kClipTileW = 64, kClipTileH = 32;

struct ClipGlyphGeometry {
  int frames = 0, width = 0, height = 0;  // height of ONE frame
  long tall_height = 0;                   // frames * height
  long frame_pixels = 0;                  // width * height
  int tiles_x = 0, tiles_y = 0;           // tiles of one frame
  long tiles = 0;                         // of the clip
  size_t max_components = 0;              // frames * max_components(width, height): a frame's cells are its own
};
ClipGlyphGeometry clip_glyph_geometry(int n_frames, int width, int height);

// Empty when acceptable, else the message for last_error.  The entry points call validate_glyphs (one frame as the
// picture) and validate_find's option checks first.  row_bytes: the stride between rows in effect; frame_stride 0: the
// frames lie back to back.
std::string validate_clip_glyphs(const char *what, int n_frames, long frame_stride, int width, int height, long row_bytes, int cap);

// The split of the compacted component list (any order, tall coordinates) into frames.  Per frame: select_components with
// find's order and the cap, or -- page && page->line_order -- order_lines and then the cap.
struct ClipGlyphSplit {
  std::vector<Component> chosen;    // frame-major, tall coordinates: what the record kernels take
  std::vector<int32_t> line, gap;   // per chosen component (all 0 without line order)
  std::vector<int32_t> start;       // frames + 1 offsets into `chosen`
  std::vector<int32_t> total;       // per frame: components with min_pixels or more, before the cap
};
// Returns the message for last_error (a component that leaves its frame: nothing the caller can cause; too many components
// for the line model), else empty.
std::string split_clip_components(const std::vector<Component> &all, const ClipGlyphGeometry &g, const FindOpts &find, const PageOpts *page,
                                  int cap, ClipGlyphSplit &out);

// component k of the split (frame f) -> its box in frame coordinates
inline void clip_frame_box(const Component &c, int frame, int height, int32_t box[4]) {
  box[0] = c.left; box[1] = c.upper - frame * height; box[2] = c.right; box[3] = c.lower - frame * height;
}

}  // namespace bnn
