// Host half of the clip scan (bnn_mi355x_scan_clip*): F frames of one size and n_sizes window sizes, every (frame, level)
// map through ONE launch per stage of layers 0-5, layers 6-8 and the decode once on all windows ("Clip scan").
//
// The levels, the grids and the boxes are the dense scan's (scan.h: plan_scene, scan_level); this file adds what a clip
// adds to them: the order of the maps, where each map of each stage lies, the work items and blocks of a merged launch,
// the tables its kernels look their map up in, the limits and the capacity.  Host-only (no HIP), linked like scan.o;
// csrc/scan_clip_kernels.hip holds the kernels, csrc/runtime.hip the entry points.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "scan.h"

namespace bnn {

// Limits (include/bnn_mi355x.h states them), next to the scan's per-picture ones, which every frame and level keeps:
// the frames of one call, and the bytes of the uploaded clip.  kScanMaxWindows bounds the windows of ALL maps and
// kScanMaxMapBytes EACH of the two map buffers.
constexpr int kScanClipMaxFrames = 4096;
constexpr size_t kScanClipMaxBytes = (size_t)1 << 30;
constexpr int kScanClipBlock = 256;  // work items of one block of a stage launch

// Map m = f * n_sizes + k is frame f at size k.  Results are frame-major, then size-major, then raster: the windows of
// map m are [first, first + nx_k * ny_k), `first` the running sum in map order.
struct ClipMap {
  int frame = 0, level = 0;
  long first = 0;
  size_t off[kScanStages] = {};  // byte offset of its stage-s map in buffer s & 1
  size_t planes = 0;             // byte offset of its level's planar picture [3][level_h][level_w] among the call's planes
};
// Stage s of map m lies at off[s] of buffer s & 1, off[s] the sum of scan_stage_bytes of the earlier maps of that stage:
// every stage is packed by itself, and stages of equal parity overlay one another as they do in a single scan.  For
// stage 5 (32 bytes a window) that makes off[5] = first * 32: the layer-5 maps of all maps ARE the stage-5 output of
// `windows` images in result order, and run_cnv with first_stage = 6 runs once on the whole clip.
struct ClipPlan {
  ScenePlan scene;  // one frame's levels (plan_scene)
  int frames = 0, width = 0, height = 0, bands = 0;
  long row_stride = 0, frame_stride = 0;  // of the caller's clip, bytes, as given (0 = packed)
  long windows = 0;                       // of all maps
  std::vector<ClipMap> maps;
  size_t stage_bytes[kScanStages] = {};   // of all maps of a stage
  long blocks[kScanStages] = {};          // of a stage's launch
  size_t buf0 = 0, buf1 = 0;              // bytes: the stages of their parity, and layers 6 / 7 at 64 bytes a window
  size_t planes_bytes = 0;                // all levels' planes of all frames, level-major then frame
  std::vector<size_t> level_planes;       // where level k's planes start; frame f's lie 3 * level_w * level_h * f on
};

// Work items of a stage of one map, as run_scan counts them: output pixels for stages 0, 4 and 5, 2 x 2 quads of conv
// outputs for stages 1-3.  Each map gets ceil(items / 256) blocks of its own: a block never straddles two maps.
int scan_clip_items(const ScanPlan &p, int stage);
inline long scan_clip_blocks(const ScanPlan &p, int stage) { return ((long)scan_clip_items(p, stage) + kScanClipBlock - 1) / kScanClipBlock; }

// Empty when the clip can be scanned, else the message for last_error (`what`: the entry point's name).  Refused, in this
// order: what plan_scene refuses for one frame, in its words; n_frames outside 1 .. kScanClipMaxFrames; a frame stride
// shorter than a frame (height rows at the row stride); windows, map bytes and clip bytes over their limits.
std::string plan_clip(const char *what, const void *pixels, int n_frames, long frame_stride, int width, int height, int bands, long row_stride,
                      const int *sizes, int n_sizes, const void *boxes_out, ClipPlan &plan);

// The largest n_frames plan_clip accepts for RGB frames (bands = 3: the clip-bytes limit at its tightest) of this size
// with these window sizes; 0 with the message in `why` when even one frame is refused.
int scan_clip_capacity(const char *what, int width, int height, const int *sizes, int n_sizes, std::string &why);

// What a block of a merged stage launch looks up (device copy: read through scalar loads).  Offsets are bytes into the
// launch's input and output buffers (stage 0: the input is the call's planes and row / plane strides are the level's).
struct ClipMapDesc {
  long long in_off, out_off, row_stride, plane_stride;
  int iw;           // width of the input map (stages 1-5)
  int ow;           // output width (stages 0, 4, 5) or quads per row (stages 1-3)
  int n_items;      // scan_clip_items
  int first_block;  // the map's blocks are [first_block, first_block + ceil(n_items / 256))
};
static_assert(sizeof(ClipMapDesc) == 48, "12 dwords");
// One int32 array for the whole call: per stage the descriptors of all maps, then block -> map for every block of the
// stage's launch.  desc[s] / block_map[s]: offsets in int32 units (descriptors 8-byte aligned).
struct ClipTables {
  std::vector<int32_t> words;
  size_t desc[kScanStages] = {}, block_map[kScanStages] = {};
};
void clip_tables(const ClipPlan &plan, ClipTables &t);
// Stages without maps.  A plan may leave a run of stages empty -- every level's ScanPlan 0 x 0 there, so that the stage has no
// items, no blocks and no bytes (the fine scan's two plans, scan_fine.h: one holds stages 0-2, the other stages 3-5).
// clip_tables writes descriptors with no blocks for such a stage; clip_l0_tables reads stage 0 alone and clip_tail_tables
// stages 3-5 alone, and may be given a plan whose other stages are empty.  clip_mfma_tables needs stages 0-3.  A launch of a
// stage without blocks is refused (run_scan_clip): whoever builds such a plan runs its own stages only.

// ---- the matrix-core form of stages 1-3 (k_clip_conv_mfma, scan_mfma_kernels.hip; DESIGN.md 9 "Clip scan") ------------
// A block owns a BAND of one map: kClipMfmaRowPairs output row pairs x kClipMfmaChunk conv-output columns (less at the
// map's bottom and right edges).  Its input patch is (2 row pairs + 2) rows x (columns + 2) columns of the map before.
constexpr int kClipMfmaRowPairs = 8, kClipMfmaChunk = 64;
// What a block looks up, through scalar loads like ClipMapDesc: its map's descriptor and its own band.
struct ClipMfmaMap {
  long long in_off, out_off;  // bytes into the launch's input and output buffers (ClipMap::off of stages s - 1 and s)
  int iw;                     // width of the input map, pixels
  int ow;                     // conv-output width (even; the pooled stages store ow / 2 columns)
  int row_pairs;              // conv-output rows / 2
  int first_block;
};
static_assert(sizeof(ClipMfmaMap) == 32, "8 dwords");
struct ClipMfmaBand {
  int map, rp0, x0;  // first row pair and first conv-output column (a multiple of kClipMfmaChunk) of the band
  int pad;
};
static_assert(sizeof(ClipMfmaBand) == 16, "4 dwords");
// One int32 array: for stage s = 1..3 the ClipMfmaMap of all maps at maps[s], then the ClipMfmaBand of all blocks of the
// stage's launch at bands[s] (offsets in int32 units, both 16-byte aligned).  Entry 0 of the arrays is unused.
struct ClipMfmaTables {
  std::vector<int32_t> words;
  size_t maps[4] = {}, bands[4] = {};
  long blocks[4] = {};
};
void clip_mfma_tables(const ClipPlan &plan, ClipMfmaTables &t);

// ---- the matrix-core form of stages 4 and 5 (k_clip_tail_mfma, scan_tail_mfma_kernels.hip; DESIGN.md 9 "Clip scan") ----
// Layers 4 and 5 have no pool and small ragged maps.  A block owns a BAND of one map: up to kClipTailRowPairs pairs of
// output rows x up to kClipTailCols output columns.  A map's bands are equal shares, not full bands and a remainder: a map of
// ow columns has ceil(ow / kClipTailCols) band columns of ceil(ow / that) columns each (the last may be narrower), and its
// ceil(oh / 2) row pairs are shared out likewise; an odd oh leaves the last row pair with one row.  The band's input patch is
// (2 row pairs + 2) rows x (columns + 2) columns of the stage before's map, less the row past its end when oh is odd.
constexpr int kClipTailRowPairs = 4, kClipTailCols = 64;
struct ClipTailMap {
  long long in_off, out_off;  // bytes into the launch's input and output buffers (ClipMap::off of stages s - 1 and s)
  int ow, oh;                 // the output map; the input map is (ow + 2) x (oh + 2)
  int band_cols, band_rps;    // the map's share sizes: columns and row pairs of all its bands but the last of a row / column
  int first_block;
  int pad[3];
};
static_assert(sizeof(ClipTailMap) == 48, "12 dwords");
struct ClipTailBand {
  int map, rp0, x0;  // first row pair (a multiple of band_rps) and first output column (a multiple of band_cols)
  int pad;
};
static_assert(sizeof(ClipTailBand) == 16, "4 dwords");
// One int32 array: for stage s = 4, 5 the ClipTailMap of all maps at maps[s - 4], then the ClipTailBand of all blocks of
// the stage's launch at bands[s - 4] (offsets in int32 units, both 16-byte aligned).
struct ClipTailTables {
  std::vector<int32_t> words;
  size_t maps[2] = {}, bands[2] = {};
  long blocks[2] = {};
};
void clip_tail_tables(const ClipPlan &plan, ClipTailTables &t);

// ---- the matrix-core form of stage 0 (k_clip_conv0_mfma, scan_l0_mfma_kernels.hip; DESIGN.md 9 "Clip scan") ------------
// A block owns a BAND of one map: kClipL0Rows output rows x kClipL0Cols output columns (less at the map's bottom and right
// edges).  Its input patch is 3 planes x (rows + 2) rows x (columns + 2) bytes of the level's planar picture, whose rows
// start at any byte address: the kernel stages a patch row with the aligned dwords around it, dword d of a row being the
// two aligned dwords at and behind (row start rounded down to 4) + 4 d, for d < ceil((columns + 2) / 4).
constexpr int kClipL0Rows = 16, kClipL0Cols = 128;
struct ClipL0Map {
  long long in_off, out_off;  // bytes: the level's planes among the call's planes (ClipMap::planes), ClipMap::off[0] in buffer 0
  long long plane_stride;     // bytes between the three planes
  int row_stride;             // bytes between the rows of a plane (the level's width)
  int ow, oh;                 // the stage-0 map
  int first_block;
};
static_assert(sizeof(ClipL0Map) == 40, "10 dwords");
// (a band is a ClipMfmaBand whose rp0 is the band's first output ROW and x0 its first output column)
// One int32 array: the ClipL0Map of all maps at `maps`, then the ClipMfmaBand of all blocks of the launch at `bands`
// (offsets in int32 units; maps 8-byte, bands 16-byte aligned when the array is).
struct ClipL0Tables {
  std::vector<int32_t> words;
  size_t maps = 0, bands = 0;
  long blocks = 0;
  // One past the highest byte a staging load of the launch touches, from the start of the call's planes (which is 4-byte
  // aligned): up to 7 bytes past ClipPlan::planes_bytes.  The planes' allocation must hold that many bytes.
  size_t planes_top = 0;
};
void clip_l0_tables(const ClipPlan &plan, ClipL0Tables &t);
// One past the highest byte the staging of patch row `row` (0 .. rows + 1) of plane `plane` of a band touches; the lowest is
// clip_l0_row_first.  `rows`, `cols`: the band's output rows and columns.  The kernel's loads, stated once for the plan and its test.
inline size_t clip_l0_row_first(const ClipL0Map &m, int y0, int x0, int plane, int row) {
  return ((size_t)m.in_off + (size_t)plane * (size_t)m.plane_stride + (size_t)(y0 + row) * (size_t)m.row_stride + (size_t)x0) & ~(size_t)3;
}
inline size_t clip_l0_row_top(const ClipL0Map &m, int y0, int x0, int cols, int plane, int row) {
  return clip_l0_row_first(m, y0, x0, plane, row) + 4 * (size_t)((cols + 2 + 3) / 4) + 4;
}

}  // namespace bnn
