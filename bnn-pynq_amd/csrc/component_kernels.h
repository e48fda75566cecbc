// Device half of find_glyphs / read_glyphs (see components.h): the enhanced L plane that enqueue_glyph_plane left on the
// device -> the list of its connected components (first pixel, box, pixel count) and, when asked for, the label map.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "components.h"

namespace bnn {

// None of the kernels uses LDS: the ink words and the labels live in global memory (L2), the reductions are wave-level.
constexpr int kComponentLdsBytes = 0;
// ints in front of the compacted list: [0] roots numbered, [1] components kept; 32 bytes, zeroed by launch_cc_collect
constexpr int kComponentHead = 8;

inline int cc_words_per_row(int width) { return (width + 63) / 64; }

struct ComponentPlane {
  const uint8_t *plane;  // height x plane_pitch (device), bytes past `width` in a row: 255 (glyph_kernels.h)
  long plane_pitch;
  int width, height;
  int words_per_row;     // cc_words_per_row(width)
  uint64_t *bits;        // height x words_per_row ink words: bit b of word w of row y is pixel (64 w + b, y)
  int32_t *label;        // width x height, index y * width + x
};

// k_cc_bits, k_cc_merge, k_cc_flatten: afterwards label[p] is the first pixel of p's component, -1 for background
hipError_t launch_cc_label(const ComponentPlane &c, int ink_level, int reach_x, int reach_y, hipStream_t s);
// k_cc_roots, k_cc_stats, k_cc_compact: head (kComponentHead ints, then the list of up to `cap` components with
// min_pixels or more, in arrival order) and stat (cap components, by root number).  Afterwards label[root] is -2 - id.
// cap >= max_components(width, height).
hipError_t launch_cc_collect(const ComponentPlane &c, int32_t *head, Component *stat, int cap, int min_pixels, hipStream_t s);
// out[p] = index_of_id[id of p's component], -1 for background; index_of_id: one int per numbered root
hipError_t launch_cc_relabel(const ComponentPlane &c, const int32_t *index_of_id, int32_t *out, hipStream_t s);

}  // namespace bnn
