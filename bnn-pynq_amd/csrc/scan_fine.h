// Host half of the fine clip scan (bnn_mi355x_scan_clip_fine): every 32 x 32 window of every level at stride 2, from ONE pass
// over layers 0-3 and four passes, one per pool phase, over layers 4-8 ("Fine scan").
//
// A window at level offset (2I, 2J) sees the first pool's global cells as its own (2I is even), so stages 0-2 and the layer-3
// convolution are shared by all stride-2 windows.  Its layer-3 columns start at global column I: its second pool pairs the
// global columns (2X + px, 2X + px + 1) with px = I & 1, and the rows alike with py = J & 1.  Behind that pool, pixel (i, j)
// of PHASE (px, py) in stage 5 holds the 256 bits of the window at level position (4i + 2px, 4j + 2py); phase (0, 0) is the
// stride-4 scan.
//
// Host-only (no HIP), linked like scan_clip.o: the grid, the maps and where they lie, the tables of every stage's launch, the
// boxes, validation and limits.  csrc/scan_phase_kernels.hip holds the kernel of stages 2 and 3, csrc/runtime.hip the entry
// points; stages 0, 1, 4 and 5 run the clip scan's kernels on the tables they always read.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "scan_clip.h"

namespace bnn {

constexpr int kFineStride = 2, kFinePhases = 4;  // phase p = 2 py + px

// nx2 = (level_w - 32) / 2 + 1, ny2 alike; false for a side below 32
bool scan_fine_grid(int level_w, int level_h, int *nx2, int *ny2);

// The maps of one level along both axes.  Only the used extent 2 (n2 - 1) + 32 is read.
//   stage   0 (L0)       1 (L1 + pool)   2 (L2)     L3 conv   3 (L3 + pool)   4 (L4)    5 (L5)
//   width   2 nx2 + 28   nx2 + 13        nx2 + 11   nx2 + 9   nxp + 4         nxp + 2   nxp       nxp = ceil((nx2 - px) / 2)
// Stages 0-2 have one map a level, stages 3-5 one a phase; a phase with nxp = 0 or nyp = 0 has no maps and no windows.
struct FineLevel {
  int nx2 = 0, ny2 = 0;
  int w[3] = {}, h[3] = {};                    // stages 0-2
  int cw = 0, ch = 0;                          // the layer-3 convolution
  int nxp[kFinePhases] = {}, nyp[kFinePhases] = {};  // windows of phase p along each axis (stage 5's map)
  long windows = 0;                            // of all phases: nx2 * ny2
};
void fine_level(int level_w, int level_h, FineLevel &f);

// Returns the number of boxes of a size (result order: phase (py, then px), then raster) and writes the first `cap` of
// them, 4 ints each: window (I, J) = (2i + px, 2j + py) is (I s / 16, J s / 16, + s, + s), integer division -- for even I, J
// the stride-4 scan's i s / 8.  Such a box lies inside the picture: I <= (level_w - 32) / 2, so I s / 16 + s <= level_w s / 32
// <= width.  -1 when the size or the level is refused (scan_level).
long scan_fine_boxes(int width, int height, int size, int *boxes, long cap);

// A fine call as two clip plans, so that the clip scan's table builders (scan_clip.h) read each as they read any clip:
//   front  stages 0-2: map m = f * n_sizes + k is frame f at size k.  Its levels, planes and strides are plan_clip's; the
//          ScanPlans hold the fine extents of stages 0-2 and 0 x 0 maps behind (scan_clip.h, "Stages without maps").
//   back   stages 3-5: one map per (frame, size, non-empty phase) in result order, so that its stage-5 maps ARE the
//          stage-5 output of `windows` images (ClipMap::off[5] = first * 32).  Its "levels" are the (size, phase) pairs of
//          one frame, with 0 x 0 maps before stage 3.
// Stage s of either lies in buffer s & 1, each stage packed by itself.
struct FinePlan {
  ClipPlan front, back;
  std::vector<FineLevel> levels;  // of one frame, per size
  std::vector<int> back_map;      // [front map * 4 + phase]: its map in `back`, -1 for an empty phase
  std::vector<int> phase;         // of a back map: 2 py + px
  long windows = 0;
  size_t buf0 = 0, buf1 = 0;      // also front.buf0 / buf1: the workspace of the whole call
};
// Empty when the clip can be scanned at stride 2, else the message for last_error.  Refused: what plan_clip refuses, in its
// words; then windows and map bytes over their limits once all phases are counted.
std::string plan_fine(const char *what, const void *pixels, int n_frames, long frame_stride, int width, int height, int bands, long row_stride,
                      const int *sizes, int n_sizes, const void *boxes_out, FinePlan &plan);

// ---- stages 2 and 3: k_clip_conv_phase (scan_phase_kernels.hip) ---------------------------------------------------------------
// A block owns a BAND of one map's convolution: up to kPhaseRows conv rows x up to two tiles of 32 conv columns.
//   stage 2 (no pool)  tiles 32 columns apart: a band is 16 x 64 outputs, bands 16 rows and 64 columns apart.
//   stage 3 (phases)   a pooled pixel of any phase is the 2 x 2 block of conv outputs that STARTS at (r, c), for every r, c
//                      with r + 1 < oh and c + 1 < ow: phase (c & 1, r & 1), pixel (c >> 1, r >> 1).  A tile of 32 columns
//                      owns its first 31 starts and a band of 16 rows its first 15, so tiles lie 31 columns and bands 15 rows
//                      and 62 columns apart: one conv row and one conv column in 16 x 31 are computed twice.
constexpr int kPhaseRows = 16, kPhaseTile = 32;
constexpr int phase_band_rows(bool phases) { return phases ? kPhaseRows - 1 : kPhaseRows; }
constexpr int phase_tile_step(bool phases) { return phases ? kPhaseTile - 1 : kPhaseTile; }
constexpr int phase_band_cols(bool phases) { return 2 * phase_tile_step(phases); }
// conv columns a band computes, at most: its two tiles
constexpr int phase_band_span(bool phases) { return phase_tile_step(phases) + kPhaseTile; }
struct ClipPhaseMap {
  long long in_off;      // bytes into the launch's input buffer: the stage before's map
  long long out_off[4];  // bytes into the output buffer.  Stage 2: [0] alone.  Stage 3: phase p's map, -1 for an empty phase
  int iw;                // width of the input map, pixels
  int ow, oh;            // the convolution: iw - 2 columns, any parity
  int pad;
};
static_assert(sizeof(ClipPhaseMap) == 56, "14 dwords");
struct ClipPhaseBand {
  int map, y0, x0;  // first conv row and column of the band
  int pad;
};
static_assert(sizeof(ClipPhaseBand) == 16, "4 dwords");
// One int32 array: for stage s = 2, 3 the ClipPhaseMap of all front maps at maps[s - 2], then the ClipPhaseBand of all blocks
// of the stage's launch at bands[s - 2] (offsets in int32 units; maps 8-byte, bands 16-byte aligned when the array is).
struct ClipPhaseTables {
  std::vector<int32_t> words;
  size_t maps[2] = {}, bands[2] = {};
  long blocks[2] = {};
};
void clip_phase_tables(const FinePlan &plan, ClipPhaseTables &t);

// Stage 1 of the front maps in the clip scan's matrix form: the ClipMfmaMap of all maps, then the ClipMfmaBand of all blocks
// (scan_clip.h; offsets in int32 units, 16-byte aligned).  The conv width 2 nx2 + 26 and height are even: whole quads.
struct FineStage1Tables {
  std::vector<int32_t> words;
  size_t maps = 0, bands = 0;
  long blocks = 0;
};
void fine_stage1_tables(const FinePlan &plan, FineStage1Tables &t);

}  // namespace bnn
