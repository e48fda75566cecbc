// Host half of the fine clip scan: see scan_fine.h.
#include "scan_fine.h"

#include <algorithm>
#include <cassert>
#include <cstring>

namespace bnn {

bool scan_fine_grid(int level_w, int level_h, int *nx2, int *ny2) {
  if (level_w < kScanWindow || level_h < kScanWindow) return false;
  if (nx2) *nx2 = (level_w - kScanWindow) / kFineStride + 1;
  if (ny2) *ny2 = (level_h - kScanWindow) / kFineStride + 1;
  return true;
}

namespace {

// one axis: the maps of stages 0-2, the layer-3 convolution and the windows of phase bit 0 and 1, from n2 windows at stride 2
void fine_axis(int n2, int (&s)[3], int &conv, int (&np)[2]) {
  const int u = kScanWindow + kFineStride * (n2 - 1);  // the used extent: even
  s[0] = u - 2;
  s[1] = (u - 4) / 2;
  s[2] = s[1] - 2;
  conv = s[2] - 2;
  for (int b = 0; b < 2; b++) {
    np[b] = (n2 - b + 1) / 2;  // ceil((n2 - b) / 2)
    // behind the phase's pool and layers 4 and 5 the map is the phase's windows
    assert((conv - b) / 2 - 4 == np[b]);
  }
  assert(s[1] == n2 + 13 && conv == n2 + 9 && (u - 4) % 2 == 0);
}

template <typename T>
void append(std::vector<int32_t> &words, const T &v) {
  constexpr size_t n = sizeof(T) / sizeof(int32_t);
  words.resize(words.size() + n);
  std::memcpy(&words[words.size() - n], &v, sizeof(T));
}

}  // namespace

void fine_level(int level_w, int level_h, FineLevel &f) {
  f = FineLevel{};
  if (!scan_fine_grid(level_w, level_h, &f.nx2, &f.ny2)) return;
  int px[2], py[2];
  fine_axis(f.nx2, f.w, f.cw, px);
  fine_axis(f.ny2, f.h, f.ch, py);
  for (int p = 0; p < kFinePhases; p++) {
    f.nxp[p] = px[p & 1];
    f.nyp[p] = py[p >> 1];
    f.windows += (long)f.nxp[p] * f.nyp[p];
  }
  assert(f.windows == (long)f.nx2 * f.ny2);
}

long scan_fine_boxes(int width, int height, int size, int *boxes, long cap) {
  int lw = 0, lh = 0;
  if (!scan_level(width, height, size, &lw, &lh)) return -1;
  FineLevel f;
  fine_level(lw, lh, f);
  long n = 0;
  for (int p = 0; p < kFinePhases; p++)
    for (int j = 0; j < f.nyp[p]; j++)
      for (int i = 0; i < f.nxp[p]; i++, n++) {
        const int l = (2 * i + (p & 1)) * size / 16, u = (2 * j + (p >> 1)) * size / 16;
        assert(l + size <= width && u + size <= height);
        if (boxes && n < cap) {
          int *b = boxes + 4 * n;
          b[0] = l; b[1] = u; b[2] = l + size; b[3] = u + size;
        }
      }
  return n;
}

std::string plan_fine(const char *what, const void *pixels, int n_frames, long frame_stride, int width, int height, int bands, long row_stride,
                      const int *sizes, int n_sizes, const void *boxes_out, FinePlan &plan) {
  const std::string name = std::string(what) + ": ";
  plan = FinePlan{};
  ClipPlan &front = plan.front, &back = plan.back;
  const std::string bad = plan_clip(what, pixels, n_frames, frame_stride, width, height, bands, row_stride, sizes, n_sizes, boxes_out, front);
  if (!bad.empty()) return bad;
  // one frame's levels at stride 2; the (size, phase) pairs that have windows become the levels of `back`
  const size_t n_levels = front.scene.levels.size();
  std::vector<int> back_level(n_levels * kFinePhases, -1), level_phase;  // [size * 4 + phase] -> level of `back`; its phase
  long per_frame = 0;
  for (size_t k = 0; k < n_levels; k++) {
    ScanLevel &lv = front.scene.levels[k];
    FineLevel f;
    fine_level(lv.level_w, lv.level_h, f);
    plan.levels.push_back(f);
    ScanPlan p;
    p.nx = f.nx2; p.ny = f.ny2;
    p.wu = f.w[0] + 2; p.hu = f.h[0] + 2;
    for (int s = 0; s < 3; s++) { p.w[s] = f.w[s]; p.h[s] = f.h[s]; }
    lv.plan = p;
    lv.first = per_frame;
    for (int ph = 0; ph < kFinePhases; ph++) {
      if (f.nxp[ph] == 0 || f.nyp[ph] == 0) continue;
      ScanLevel b;
      b.size = lv.size; b.level_w = lv.level_w; b.level_h = lv.level_h;
      b.plan.nx = f.nxp[ph]; b.plan.ny = f.nyp[ph];
      for (int s = 3; s < kScanStages; s++) { b.plan.w[s] = f.nxp[ph] + 2 * (5 - s); b.plan.h[s] = f.nyp[ph] + 2 * (5 - s); }
      assert(b.plan.w[3] == (f.cw - (ph & 1)) / 2 && b.plan.h[3] == (f.ch - (ph >> 1)) / 2);
      b.first = per_frame;
      per_frame += (long)f.nxp[ph] * f.nyp[ph];
      back_level[k * kFinePhases + ph] = (int)back.scene.levels.size();
      back.scene.levels.push_back(b);
      level_phase.push_back(ph);
    }
  }
  front.scene.windows = back.scene.windows = per_frame;
  const std::string clip = "a clip of " + std::to_string(n_frames) + " frames ";
  if (per_frame > kScanMaxWindows / n_frames)
    return name + clip + "has " + std::to_string(per_frame * n_frames) + " windows at stride 2, more than the limit of " + std::to_string(kScanMaxWindows);

  // where every map lies: each stage packed by itself, in map order
  back.frames = front.frames; back.width = width; back.height = height; back.bands = bands;
  for (int s = 0; s < kScanStages; s++) front.stage_bytes[s] = front.blocks[s] = 0;
  plan.back_map.assign(front.maps.size() * kFinePhases, -1);
  for (size_t m = 0; m < front.maps.size(); m++) {
    ClipMap &cm = front.maps[m];
    const ScanLevel &lv = front.scene.levels[(size_t)cm.level];
    cm.first = back.windows;
    for (int s = 0; s < kScanStages; s++) {
      cm.off[s] = front.stage_bytes[s];
      front.stage_bytes[s] += scan_stage_bytes(lv.plan, s);
      front.blocks[s] += scan_clip_blocks(lv.plan, s);
    }
    for (int ph = 0; ph < kFinePhases; ph++) {
      const int bl = back_level[(size_t)cm.level * kFinePhases + ph];
      if (bl < 0) continue;
      const ScanLevel &b = back.scene.levels[(size_t)bl];
      ClipMap bm;
      bm.frame = cm.frame; bm.level = bl;
      bm.first = back.windows;
      for (int s = 0; s < kScanStages; s++) {
        bm.off[s] = back.stage_bytes[s];
        back.stage_bytes[s] += scan_stage_bytes(b.plan, s);
        back.blocks[s] += scan_clip_blocks(b.plan, s);
      }
      assert(bm.off[5] == (size_t)bm.first * 32 && level_phase[(size_t)bl] == ph);
      back.windows += (long)b.plan.nx * b.plan.ny;
      plan.back_map[m * kFinePhases + ph] = (int)back.maps.size();
      plan.phase.push_back(ph);
      back.maps.push_back(bm);
    }
  }
  assert(back.windows == per_frame * n_frames);
  plan.windows = front.windows = back.windows;
  const size_t tail = (size_t)plan.windows * 64;  // layers 6 and 7: 512 bits per window
  plan.buf0 = std::max({tail, front.stage_bytes[0], front.stage_bytes[2], back.stage_bytes[4]});
  plan.buf1 = std::max({tail, front.stage_bytes[1], back.stage_bytes[3], back.stage_bytes[5]});
  front.buf0 = back.buf0 = plan.buf0;
  front.buf1 = back.buf1 = plan.buf1;
  if (plan.buf0 > kScanMaxMapBytes || plan.buf1 > kScanMaxMapBytes)
    return name + "the maps of " + clip + "take " + std::to_string(std::max(plan.buf0, plan.buf1)) + " bytes in one buffer at stride 2, more than the limit of " +
           std::to_string(kScanMaxMapBytes);
  return "";
}

void clip_phase_tables(const FinePlan &plan, ClipPhaseTables &t) {
  constexpr size_t kMapWords = sizeof(ClipPhaseMap) / sizeof(int32_t);
  const size_t n_maps = plan.front.maps.size();
  t = ClipPhaseTables{};
  for (int s = 2; s <= 3; s++) {
    const bool phases = s == 3;
    t.maps[s - 2] = t.words.size();
    t.words.resize((t.words.size() + n_maps * kMapWords + 3) & ~(size_t)3, 0);
    t.bands[s - 2] = t.words.size();
    long block = 0;
    for (size_t m = 0; m < n_maps; m++) {
      const ClipMap &cm = plan.front.maps[m];
      const FineLevel &f = plan.levels[(size_t)cm.level];
      ClipPhaseMap d{};
      d.in_off = (long long)cm.off[s - 1];
      d.iw = f.w[s - 1];
      d.ow = phases ? f.cw : f.w[2];
      d.oh = phases ? f.ch : f.h[2];
      assert(d.ow == d.iw - 2 && d.oh == f.h[s - 1] - 2 && d.ow > 1 && d.oh > 1);
      for (int ph = 0; ph < kFinePhases; ph++) {
        const int bm = plan.back_map[m * kFinePhases + ph];
        d.out_off[ph] = !phases ? (ph == 0 ? (long long)cm.off[2] : -1) : bm < 0 ? -1 : (long long)plan.back.maps[(size_t)bm].off[3];
      }
      std::memcpy(&t.words[t.maps[s - 2] + m * kMapWords], &d, sizeof(d));
      // a band of the pooled stage needs a row and a column behind its first: the last start is (oh - 2, ow - 2)
      const int need = phases ? 1 : 0;
      for (int y0 = 0; y0 + need < d.oh; y0 += phase_band_rows(phases))
        for (int x0 = 0; x0 + need < d.ow; x0 += phase_band_cols(phases), block++) append(t.words, ClipPhaseBand{(int)m, y0, x0, 0});
    }
    t.blocks[s - 2] = block;
  }
}

void fine_stage1_tables(const FinePlan &plan, FineStage1Tables &t) {
  constexpr size_t kMapWords = sizeof(ClipMfmaMap) / sizeof(int32_t);
  const size_t n_maps = plan.front.maps.size();
  t = FineStage1Tables{};
  t.words.resize(n_maps * kMapWords, 0);
  t.bands = t.words.size();
  for (size_t m = 0; m < n_maps; m++) {
    const ClipMap &cm = plan.front.maps[m];
    const FineLevel &f = plan.levels[(size_t)cm.level];
    ClipMfmaMap d{};
    d.in_off = (long long)cm.off[0];
    d.out_off = (long long)cm.off[1];
    d.iw = f.w[0];
    d.ow = f.w[0] - 2;
    d.row_pairs = (f.h[0] - 2) / 2;
    d.first_block = (int)t.blocks;
    assert(d.ow == 2 * f.w[1] && d.row_pairs == f.h[1]);
    std::memcpy(&t.words[m * kMapWords], &d, sizeof(d));
    for (int rp0 = 0; rp0 < d.row_pairs; rp0 += kClipMfmaRowPairs)
      for (int x0 = 0; x0 < d.ow; x0 += kClipMfmaChunk, t.blocks++) append(t.words, ClipMfmaBand{(int)m, rp0, x0, 0});
  }
}

}  // namespace bnn
