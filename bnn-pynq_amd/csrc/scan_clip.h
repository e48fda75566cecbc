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

}  // namespace bnn
