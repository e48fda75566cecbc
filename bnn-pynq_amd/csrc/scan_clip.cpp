// Host half of the clip scan: see scan_clip.h.
#include "scan_clip.h"

#include <cassert>
#include <cstring>

namespace bnn {

int scan_clip_items(const ScanPlan &p, int stage) {
  if (stage < 0 || stage >= kScanStages) return 0;
  // output pixels; a pooled pixel of stages 1 and 3 is one 2 x 2 quad of conv outputs; stage 2's map is even: whole quads
  return stage == 2 ? (p.w[2] / 2) * (p.h[2] / 2) : p.w[stage] * p.h[stage];
}

namespace {

// what one frame adds to a call: windows, bytes of each stage, bytes of the two buffers per frame
struct PerFrame {
  long windows = 0;
  size_t stage[kScanStages] = {};
  size_t buf0 = 0, buf1 = 0;
};
PerFrame per_frame(const ScenePlan &scene) {
  PerFrame f;
  f.windows = scene.windows;
  for (const ScanLevel &lv : scene.levels)
    for (int s = 0; s < kScanStages; s++) f.stage[s] += scan_stage_bytes(lv.plan, s);
  const size_t tail = (size_t)f.windows * 64;  // layers 6 and 7: 512 bits per window
  f.buf0 = f.buf1 = tail;
  for (int s = 0; s < kScanStages; s++) {
    size_t &b = (s & 1) ? f.buf1 : f.buf0;
    if (f.stage[s] > b) b = f.stage[s];
  }
  return f;
}

// Empty when F frames stay inside the clip's own limits.  Everything grows linearly with F: the check of F frames is the
// check of F times one frame's figures.  (The windows are compared by division: with very many sizes their product could
// pass 2^63.  Behind that check there are at most 2^20 levels of at most 2^27 bytes a stage and F is at most 4096, and a
// frame has at most 2^26 x 3 bytes: the other products fit 64 bits.)
std::string over_limits(const std::string &name, const PerFrame &f, size_t frame_bytes, long frames) {
  const std::string clip = "a clip of " + std::to_string(frames) + " frames ";
  if (f.windows > kScanMaxWindows / frames)
    return name + clip + "has " + std::to_string(f.windows * frames) + " windows, more than the limit of " + std::to_string(kScanMaxWindows);
  const size_t b0 = f.buf0 * (size_t)frames, b1 = f.buf1 * (size_t)frames;
  if (b0 > kScanMaxMapBytes || b1 > kScanMaxMapBytes)
    return name + "the maps of " + clip + "take " + std::to_string(b0 > b1 ? b0 : b1) + " bytes in one buffer, more than the limit of " +
           std::to_string(kScanMaxMapBytes);
  if (frame_bytes * (size_t)frames > kScanClipMaxBytes)
    return name + clip + "takes " + std::to_string(frame_bytes * (size_t)frames) + " bytes, more than the limit of " + std::to_string(kScanClipMaxBytes);
  return "";
}

}  // namespace

std::string plan_clip(const char *what, const void *pixels, int n_frames, long frame_stride, int width, int height, int bands, long row_stride,
                      const int *sizes, int n_sizes, const void *boxes_out, ClipPlan &plan) {
  const std::string name = std::string(what) + ": ";
  plan = ClipPlan{};
  const std::string bad = plan_scene(what, pixels, width, height, bands, row_stride, sizes, n_sizes, boxes_out, plan.scene);
  if (!bad.empty()) return bad;
  if (n_frames < 1 || n_frames > kScanClipMaxFrames)
    return name + "need 1 to " + std::to_string(kScanClipMaxFrames) + " frames (got " + std::to_string(n_frames) + ")";
  const size_t row_bytes = (size_t)width * bands, frame_bytes = row_bytes * height;
  const size_t rows_apart = row_stride ? (size_t)row_stride : row_bytes;
  if (frame_stride != 0 && (frame_stride < 0 || (size_t)frame_stride < rows_apart * height)) return name + "frame stride shorter than a frame";
  const PerFrame f = per_frame(plan.scene);
  const std::string over = over_limits(name, f, frame_bytes, n_frames);
  if (!over.empty()) return over;

  plan.frames = n_frames; plan.width = width; plan.height = height; plan.bands = bands;
  plan.row_stride = row_stride; plan.frame_stride = frame_stride;
  const size_t n_levels = plan.scene.levels.size();
  for (const ScanLevel &lv : plan.scene.levels) {
    plan.level_planes.push_back(plan.planes_bytes);
    plan.planes_bytes += (size_t)3 * lv.level_w * lv.level_h * n_frames;
  }
  plan.maps.reserve((size_t)n_frames * n_levels);
  for (int fr = 0; fr < n_frames; fr++)
    for (size_t k = 0; k < n_levels; k++) {
      const ScanLevel &lv = plan.scene.levels[k];
      ClipMap m;
      m.frame = fr; m.level = (int)k;
      m.first = plan.windows;
      m.planes = plan.level_planes[k] + (size_t)3 * lv.level_w * lv.level_h * fr;
      for (int s = 0; s < kScanStages; s++) {
        m.off[s] = plan.stage_bytes[s];
        plan.stage_bytes[s] += scan_stage_bytes(lv.plan, s);
        plan.blocks[s] += scan_clip_blocks(lv.plan, s);
      }
      assert(m.off[5] == (size_t)m.first * 32);
      plan.windows += (long)lv.plan.nx * lv.plan.ny;
      plan.maps.push_back(m);
    }
  plan.buf0 = f.buf0 * (size_t)n_frames;
  plan.buf1 = f.buf1 * (size_t)n_frames;
  assert(plan.windows == f.windows * n_frames);
  for (int s = 0; s < kScanStages; s++) assert(plan.stage_bytes[s] == f.stage[s] * (size_t)n_frames && plan.stage_bytes[s] <= ((s & 1) ? plan.buf1 : plan.buf0));
  return "";
}

int scan_clip_capacity(const char *what, int width, int height, const int *sizes, int n_sizes, std::string &why) {
  // (plan_scene with a stand-in for the pointers it checks, as scan_boxes does)
  ScenePlan scene;
  why = plan_scene(what, sizes ? (const void *)&scene : nullptr, width, height, 3, 0, sizes, n_sizes, &scene, scene);
  if (!why.empty()) return 0;
  const std::string name = std::string(what) + ": ";
  const PerFrame f = per_frame(scene);
  const size_t frame_bytes = (size_t)width * height * 3;
  why = over_limits(name, f, frame_bytes, 1);
  if (!why.empty()) return 0;
  long cap = kScanClipMaxFrames;
  const auto at_most = [&](size_t limit, size_t per) { if (per > 0 && (long)(limit / per) < cap) cap = (long)(limit / per); };
  at_most((size_t)kScanMaxWindows, (size_t)f.windows);
  at_most(kScanMaxMapBytes, f.buf0);
  at_most(kScanMaxMapBytes, f.buf1);
  at_most(kScanClipMaxBytes, frame_bytes);
  assert(cap >= 1 && over_limits(name, f, frame_bytes, cap).empty() && (cap == kScanClipMaxFrames || !over_limits(name, f, frame_bytes, cap + 1).empty()));
  return (int)cap;
}

void clip_tables(const ClipPlan &plan, ClipTables &t) {
  const size_t n_maps = plan.maps.size();
  constexpr size_t kDescWords = sizeof(ClipMapDesc) / sizeof(int32_t);
  size_t total = 0;
  for (int s = 0; s < kScanStages; s++) {
    t.desc[s] = total;
    total += n_maps * kDescWords;
    t.block_map[s] = total;
    total += ((size_t)plan.blocks[s] + 1) & ~(size_t)1;  // the next stage's descriptors stay 8-byte aligned
  }
  t.words.assign(total, 0);
  for (int s = 0; s < kScanStages; s++) {
    long block = 0;
    for (size_t m = 0; m < n_maps; m++) {
      const ClipMap &cm = plan.maps[m];
      const ScanLevel &lv = plan.scene.levels[(size_t)cm.level];
      const ScanPlan &p = lv.plan;
      ClipMapDesc d{};
      d.in_off = (long long)(s == 0 ? cm.planes : cm.off[s - 1]);
      d.out_off = (long long)cm.off[s];
      d.row_stride = s == 0 ? lv.level_w : 0;
      d.plane_stride = s == 0 ? (long long)lv.level_w * lv.level_h : 0;
      d.iw = s == 0 ? lv.level_w : p.w[s - 1];
      d.ow = s == 2 ? p.w[2] / 2 : p.w[s];
      d.n_items = scan_clip_items(p, s);
      d.first_block = (int)block;
      std::memcpy(&t.words[t.desc[s] + m * kDescWords], &d, sizeof(d));
      const long nb = scan_clip_blocks(p, s);
      for (long b = 0; b < nb; b++) t.words[t.block_map[s] + (size_t)(block + b)] = (int32_t)m;
      block += nb;
    }
    assert(block == plan.blocks[s]);
  }
}

}  // namespace bnn
