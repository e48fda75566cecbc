// component_kernels.hip -- connected components of the ink of an L plane (see components.h, component_kernels.h).
//
// A wave owns 64 consecutive pixels of one row (a "unit": row y, ink word w); a block is four such waves.
//   k_cc_bits     __ballot(value < ink_level) is the unit's 64-bit ink word; every neighbour test afterwards is bit
//                 arithmetic on these words.  label[p] = the start of p's run of ink inside its word (consecutive ink of
//                 a row is connected at any reach, so this is a parent of p already), -1 for background.
//   k_cc_merge    every ink pixel visits the forward half of its neighbourhood: the nearest ink to its right within
//                 reach_x, and in each of the rows y + 1 .. y + reach_y the window x - reach_x .. x + reach_x, where one
//                 join per run of set bits is enough.  A pixel whose left neighbour is ink looks at the window's last
//                 column only: the rest lies in the neighbour's window.
//   k_cc_flatten  label[p] = root of p.
//   k_cc_roots    roots get numbers (arrival order: the host sorts) and an empty entry each; label[root] = -2 - number.
//   k_cc_stats    box and pixel count per root.  The lanes of a unit that share a root are one bit mask: its lowest and
//                 highest bit, the row and its popcount go into five atomics per (unit, root), not per pixel.
//   k_cc_compact  the entries with min_pixels or more, behind one counter.
//   k_cc_relabel  (only when the label map is asked for) root number -> returned index, per pixel.
//
// Why the merge is correct and cannot hang.  label[] is a forest: label[i] <= i always (a root points at itself), and
// the only write of the merge launch is atomicMin(label + a, b) with b < a, so entries only ever decrease and a walk
// towards a root strictly descends: every loop is bounded by the index it starts from.  join(a, b) finds both roots,
// hangs the larger under the smaller with that atomicMin, and goes on from the value the atomic RETURNED until the
// atomic returns the root itself: if another workgroup got there first, the returned value is the parent it wrote, a
// member of the same set, and the join goes on with it.  NO WORKGROUP EVER WAITS FOR ANOTHER: no spin, no flag, no
// ticket; the progress of a join depends on nothing but what its own atomics returned.
// Visibility (8 XCDs with private L2s, an L1 per CU that other CUs' stores never refresh): every read of a label in the
// merge launch is an agent-scope atomic load (it bypasses the L1), and the decisive values are the atomics' return
// values, which are made at the memory side.  Even a stale value would be harmless -- it is an earlier parent, still a
// member of the same set and never smaller than the current one, so a walk through it still descends to the set's
// root or to an entry whose atomicMin then returns the newer parent -- but nothing relies on that.  Everything that
// must see FINAL labels runs in a later launch: flatten after merge, roots after flatten, stats after roots.
#include "component_kernels.h"

#include <limits.h>

namespace bnn {
namespace {

constexpr int kThreads = 256;
constexpr int kWave = 64;
constexpr int kUnitsPerBlock = kThreads / kWave;

__device__ __forceinline__ int32_t load_label(const int32_t *label, int32_t i) {
  return __hip_atomic_load(label + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ int32_t root_of(const int32_t *label, int32_t i) {
  for (;;) {
    const int32_t parent = load_label(label, i);  // parent <= i
    if (parent == i) return i;
    i = parent;
  }
}

__device__ __forceinline__ void join(int32_t *label, int32_t a, int32_t b) {
  for (;;) {
    a = root_of(label, a);
    b = root_of(label, b);
    if (a == b) return;
    if (a < b) { const int32_t t = a; a = b; b = t; }
    const int32_t old = atomicMin(label + a, b);  // b < a
    if (old == a) return;  // a was a root still: it hangs under b now
    a = old;               // another join hung a under `old` first: old < a, and old and b are still to be joined
  }
}

// the bits of columns lane - rx .. lane + rx of a row whose words around the unit are prev, cur, next: bit j is column
// lane - rx + j
__device__ __forceinline__ uint64_t window(uint64_t prev, uint64_t cur, uint64_t next, int lane, int rx) {
  const int t = lane - rx + 64;  // 48 .. 126: the first column in the 192-bit string prev : cur : next
  uint64_t v;
  if (t < 64) v = (prev >> t) | (cur << (64 - t));
  else if (t == 64) v = cur;
  else v = (cur >> (t - 64)) | (next << (128 - t));
  return v & ((2ull << (2 * rx)) - 1);
}

// unit -> (y, w); false past the last one (wave-uniform)
__device__ __forceinline__ bool unit_of(const ComponentPlane &c, long &unit, int &y, int &w) {
  unit = (long)blockIdx.x * kUnitsPerBlock + (threadIdx.x / kWave);
  if (unit >= (long)c.height * c.words_per_row) return false;
  y = (int)(unit / c.words_per_row);
  w = (int)(unit - (long)y * c.words_per_row);
  return true;
}

__global__ __launch_bounds__(kThreads) void k_cc_bits(const ComponentPlane c, int ink_level) {
  long unit; int y, w;
  if (!unit_of(c, unit, y, w)) return;
  const int lane = threadIdx.x & (kWave - 1);
  const int x = w * kWave + lane;
  int v = 255;
  if (x < c.plane_pitch) v = c.plane[(size_t)y * (size_t)c.plane_pitch + (size_t)x];
  const bool ink = x < c.width && v < ink_level;
  const uint64_t word = __ballot(ink);
  if (lane == 0) c.bits[unit] = word;
  if (x < c.width) {
    const uint64_t below = ~word & ((1ull << lane) - 1);  // background to the left of this lane, inside the word
    const int start = below ? 64 - __builtin_clzll(below) : 0;
    c.label[(size_t)y * c.width + x] = ink ? (int32_t)((size_t)y * c.width + (size_t)(w * kWave + start)) : -1;
  }
}

__global__ __launch_bounds__(kThreads) void k_cc_merge(const ComponentPlane c, int rx, int ry) {
  long unit; int y, w;
  if (!unit_of(c, unit, y, w)) return;
  const uint64_t cur = c.bits[unit];  // (the ink words are the previous launch's: plain loads)
  if (cur == 0) return;
  const int lane = threadIdx.x & (kWave - 1);
  const bool has_prev = w > 0, has_next = w + 1 < c.words_per_row;
  const uint64_t prev = has_prev ? c.bits[unit - 1] : 0, next = has_next ? c.bits[unit + 1] : 0;
  const bool ink = (cur >> lane) & 1;
  const int x = w * kWave + lane;
  const int32_t p = (int32_t)((size_t)y * c.width + x);
  const bool left_ink = lane > 0 ? (cur >> (lane - 1)) & 1 : (prev >> 63) & 1;
  if (ink) {
    // the nearest ink to the right within reach; at distance 1 inside the word k_cc_bits has joined them already
    const uint64_t right = window(prev, cur, next, lane, rx) >> (rx + 1);
    if (right) {
      const int d = __builtin_ctzll(right);
      if (d > 0 || lane == kWave - 1) join(c.label, p, p + 1 + d);
    }
  }
  for (int dy = 1; dy <= ry && y + dy < c.height; dy++) {
    const long below = unit + (long)dy * c.words_per_row;
    const uint64_t cu = c.bits[below], pr = has_prev ? c.bits[below - 1] : 0, nx = has_next ? c.bits[below + 1] : 0;
    if ((cu | pr | nx) == 0 || !ink) continue;
    const uint64_t v = window(pr, cu, nx, lane, rx);
    uint64_t starts = v & ~(v << 1);               // one join per run of set bits: a run is connected in its own row
    if (left_ink) starts &= 1ull << (2 * rx);      // the other columns are in the left neighbour's window
    const int32_t row = (int32_t)((size_t)(y + dy) * c.width) + x - rx;
    while (starts) {
      const int j = __builtin_ctzll(starts);
      starts &= starts - 1;
      join(c.label, p, row + j);
    }
  }
}

__global__ __launch_bounds__(kThreads) void k_cc_flatten(const ComponentPlane c) {
  long unit; int y, w;
  if (!unit_of(c, unit, y, w)) return;
  const uint64_t cur = c.bits[unit];
  const int lane = threadIdx.x & (kWave - 1);
  if (!((cur >> lane) & 1)) return;
  const size_t p = (size_t)y * c.width + (size_t)(w * kWave + lane);
  // Other threads of this launch replace entries by their roots meanwhile: whichever of the two a walk reads, it is an
  // ancestor of the entry, and the walk descends to the same root (the sets are final since the merge launch ended).
  c.label[p] = root_of(c.label, (int32_t)p);
}

__global__ __launch_bounds__(kThreads) void k_cc_roots(int32_t *label, long n_pixels, int32_t *head, Component *stat, int cap) {
  const long i = (long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n_pixels || label[i] != (int32_t)i) return;  // (nobody else writes a root's own entry in this launch)
  const int id = atomicAdd(head, 1);
  if (id >= cap) return;  // (never: cap >= the 2 x 2 cells of the picture)
  stat[id] = Component{(int32_t)i, INT_MAX, INT_MAX, -1, -1, 0, id, 0};
  label[i] = -2 - id;
}

// label -> root number; -1 for background (and for a root beyond the list, which does not happen)
__device__ __forceinline__ int id_of(const int32_t *label, size_t p) {
  const int32_t l = label[p];
  if (l <= -2) return -2 - l;
  if (l < 0) return -1;
  const int32_t r = label[l];
  return r <= -2 ? -2 - r : -1;
}

__global__ __launch_bounds__(kThreads) void k_cc_stats(const ComponentPlane c, Component *stat) {
  long unit; int y, w;
  if (!unit_of(c, unit, y, w)) return;
  const uint64_t cur = c.bits[unit];
  if (cur == 0) return;
  const int lane = threadIdx.x & (kWave - 1);
  int id = -1;
  if ((cur >> lane) & 1) id = id_of(c.label, (size_t)y * c.width + (size_t)(w * kWave + lane));
  uint64_t remaining = __ballot(id >= 0);
  while (remaining) {  // once per root of the unit; `remaining` is the same in every lane
    const int leader = __builtin_ctzll(remaining);
    const int lid = __shfl(id, leader, kWave);
    const uint64_t mask = __ballot(id == lid);
    if (lane == leader) {
      Component *e = stat + lid;
      atomicMin(&e->left, w * kWave + __builtin_ctzll(mask));
      atomicMax(&e->right, w * kWave + 63 - __builtin_clzll(mask));  // inclusive until k_cc_compact
      atomicMin(&e->upper, y);
      atomicMax(&e->lower, y);
      atomicAdd(&e->pixels, __popcll(mask));
    }
    remaining &= ~mask;
  }
}

__global__ __launch_bounds__(kThreads) void k_cc_compact(int32_t *head, const Component *__restrict__ stat, int cap, int min_pixels) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  const int n = min(head[0], cap);
  if (i >= n) return;
  Component e = stat[i];
  if (e.pixels < min_pixels) return;
  e.right++;
  e.lower++;
  const int k = atomicAdd(head + 1, 1);  // k < n <= cap
  reinterpret_cast<Component *>(head + kComponentHead)[k] = e;
}

__global__ __launch_bounds__(kThreads) void k_cc_relabel(const int32_t *__restrict__ label, long n_pixels, const int32_t *__restrict__ index_of_id,
                                                         int32_t *__restrict__ out) {
  const long i = (long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n_pixels) return;
  const int id = id_of(label, (size_t)i);
  out[i] = id >= 0 ? index_of_id[id] : -1;
}

unsigned blocks_for(long n, int per_block) { return (unsigned)((n + per_block - 1) / per_block); }

}  // namespace

hipError_t launch_cc_label(const ComponentPlane &c, int ink_level, int reach_x, int reach_y, hipStream_t s) {
  const dim3 grid(blocks_for((long)c.height * c.words_per_row, kUnitsPerBlock)), block(kThreads);
  hipLaunchKernelGGL(k_cc_bits, grid, block, 0, s, c, ink_level);
  hipLaunchKernelGGL(k_cc_merge, grid, block, 0, s, c, reach_x, reach_y);
  hipLaunchKernelGGL(k_cc_flatten, grid, block, 0, s, c);
  return hipGetLastError();
}

hipError_t launch_cc_collect(const ComponentPlane &c, int32_t *head, Component *stat, int cap, int min_pixels, hipStream_t s) {
  const long n_pixels = (long)c.width * c.height;
  const hipError_t e = hipMemsetAsync(head, 0, kComponentHead * sizeof(int32_t), s);
  if (e != hipSuccess) return e;
  const dim3 block(kThreads);
  hipLaunchKernelGGL(k_cc_roots, dim3(blocks_for(n_pixels, kThreads)), block, 0, s, c.label, n_pixels, head, stat, cap);
  hipLaunchKernelGGL(k_cc_stats, dim3(blocks_for((long)c.height * c.words_per_row, kUnitsPerBlock)), block, 0, s, c, stat);
  hipLaunchKernelGGL(k_cc_compact, dim3(blocks_for(cap, kThreads)), block, 0, s, head, stat, cap, min_pixels);
  return hipGetLastError();
}

hipError_t launch_cc_relabel(const ComponentPlane &c, const int32_t *index_of_id, int32_t *out, hipStream_t s) {
  const long n_pixels = (long)c.width * c.height;
  hipLaunchKernelGGL(k_cc_relabel, dim3(blocks_for(n_pixels, kThreads)), dim3(kThreads), 0, s, c.label, n_pixels, index_of_id, out);
  return hipGetLastError();
}

}  // namespace bnn
