// clip_glyph_kernels.hip -- a clip as one tall L plane: its frames enhanced each by its own mean, its ink labelled tile by
// tile in LDS (see clip_glyphs.h, clip_glyph_kernels.h).
//
//   k_clip_luma      k_glyph_luma's body (glyph_kernels.hip) with a frame axis: a thread per 16 pixels of a row, 16-byte
//                    lanes in and out, bytes past `width` 255; blockIdx.y is the frame, and the block's pixel sum goes into
//                    sum[frame] with one 64-bit atomic.
//   k_clip_enhance   the enhance kernel's body, likewise: the mean it blends with is the frame's own.
//   k_clip_cc_tile   a block of four waves owns a tile of 64 columns x 32 rows of one frame (the last tile row of a frame is
//                    short; no tile straddles a frame).  Each wave takes rows in turn: __ballot(value < ink_level) is the
//                    row's ink word, kept in LDS and written to bits[] for the later launches.  The tile's 2 048 labels live
//                    in LDS, local index ly * 64 + lx -- ascending local index is ascending tall index -- and start at the
//                    start of the pixel's run inside its word, as k_cc_bits does.  Behind a barrier every ink pixel visits
//                    the forward half of its neighbourhood INSIDE THE TILE (k_cc_merge's rule with every word outside the
//                    tile read as 0; one join per run of set bits; a pixel whose left neighbour is ink looks at the window's
//                    last column only) and joins with atomicMin on LDS.  Behind a second barrier every pixel walks to its
//                    local root and stores label[p] = the tall index of that root's pixel, -1 for background.  Both
//                    barriers stand outside the loops, where every thread of the block reaches them.  No global atomic.
//   k_clip_cc_seams  a wave per (tall row, ink word), as k_cc_merge -- and exactly the joins of k_cc_merge whose two pixels
//                    lie in DIFFERENT tiles of the SAME frame: the right-neighbour join that leaves the word, and in the
//                    rows y + 1 .. y + reach_y (up to the frame's last row) the run starts of the window that fall into a
//                    neighbouring word or into the tile row below.  A wave whose unit has no ink within reach of a tile
//                    border leaves at once.
//   k_clip_cc_flatten  label[p] = root of p, as k_cc_flatten.
//
// Why the result is k_cc_merge's.  The tile launch leaves the connected components of the ink inside each tile (every join
// is between adjacent pixels of the tile, and the visit is k_cc_merge's on a picture that ends at the tile's border).  Every
// join of k_cc_merge inside one tile joins two pixels those components already hold together; every other join of
// k_cc_merge on the frame is a seam join.  So the sets after the seams are k_cc_merge's sets on the frame alone, and since
// the larger root always hangs under the smaller, each set's root is its first pixel: the label map is launch_cc_label's
// on each frame, shifted by f * width * height.
//
// Why no launch can hang (the argument of component_kernels.hip, for LDS and for global labels alike).  A label array is a
// forest: label[i] <= i always, a root points at itself.  The only write of a merge phase is atomicMin(label + a, b) with
// b < a, so ENTRIES ONLY DECREASE; a WALK towards a root STRICTLY DESCENDS and is bounded by the index it starts from; a
// join goes on from the value its atomic RETURNED until the atomic returns the root itself.  NO THREAD WAITS FOR ANOTHER:
// no spin, no flag, no ticket; the barriers of the tile kernel are reached by every thread unconditionally.
// Visibility: the tile kernel's labels are LDS, read with workgroup-scope atomic loads.  The seams' reads of global labels
// are agent-scope atomic loads (they bypass the CU's L1), the decisive values are the atomics' return values, and
// everything that must see FINAL labels runs in a later launch: seams after tiles, flatten after seams, collect after that.
#include "clip_glyph_kernels.h"

namespace bnn {
namespace {

constexpr int kThreads = 256;
constexpr int kWave = 64;
constexpr int kWaves = kThreads / kWave;
static_assert(kClipTileW == kWave && kClipTileH % kWaves == 0, "a wave is a tile row; the waves share the rows evenly");

__device__ __forceinline__ uint32_t byte_of(const uint32_t *raw, int k) { return (raw[k >> 2] >> (8 * (k & 3))) & 0xFF; }

template <int BANDS>
__global__ __launch_bounds__(kThreads) void k_clip_luma(const ClipGlyphPlane p) {
  __shared__ uint32_t wave_sum[kWaves];
  const long lanes_per_row = p.tall.plane_pitch / 16;
  const long lane = (long)blockIdx.x * kThreads + threadIdx.x;  // inside the frame
  const int frame = blockIdx.y;
  uint32_t sum = 0;
  if (lane < lanes_per_row * p.frame_height) {
    const long yf = lane / lanes_per_row, c = lane - yf * lanes_per_row;
    const size_t y = (size_t)frame * (size_t)p.frame_height + (size_t)yf;
    const uint4 *__restrict__ in =
        reinterpret_cast<const uint4 *>(p.tall.src + y * (size_t)(p.tall.plane_pitch * BANDS) + (size_t)c * 16 * BANDS);
    uint32_t raw[4 * BANDS];
#pragma unroll
    for (int q = 0; q < BANDS; q++) {
      const uint4 v = in[q];
      raw[4 * q] = v.x; raw[4 * q + 1] = v.y; raw[4 * q + 2] = v.z; raw[4 * q + 3] = v.w;
    }
    const int valid = p.tall.width - (int)(c * 16);
    uint32_t out[4] = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 16; j++) {
      uint32_t L;
      if constexpr (BANDS == 1) {
        L = byte_of(raw, j);
      } else {
        const uint32_t r = byte_of(raw, BANDS * j), g = byte_of(raw, BANDS * j + 1), b = byte_of(raw, BANDS * j + 2);
        L = (r * 19595u + g * 38470u + b * 7471u + 0x8000u) >> 16;  // Pillow's rgb2l; alpha is ignored
      }
      if (j < valid) sum += L;
      else L = 255;
      out[j >> 2] |= L << (8 * (j & 3));
    }
    *reinterpret_cast<uint4 *>(p.tall.plane + y * (size_t)p.tall.plane_pitch + (size_t)c * 16) = make_uint4(out[0], out[1], out[2], out[3]);
  }
#pragma unroll
  for (int d = kWave / 2; d > 0; d >>= 1) sum += __shfl_down(sum, d, kWave);
  if ((threadIdx.x & (kWave - 1)) == 0) wave_sum[threadIdx.x / kWave] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long total = 0;
#pragma unroll
    for (int w = 0; w < kWaves; w++) total += wave_sum[w];
    if (total) atomicAdd(p.tall.sum + frame, total);
  }
}

// Pillow's ImagingBlend on one 8-bit sample, multiply and add rounded separately (glyph_kernels.hip: never an FMA)
__device__ __forceinline__ uint32_t blend(int a, int b, float alpha) {
#pragma clang fp contract(off)
  const float scaled = alpha * (float)(b - a);
  const float t = (float)a + scaled;
  return t <= 0.f ? 0u : t >= 255.f ? 255u : (uint32_t)(int)t;
}

__global__ __launch_bounds__(kThreads) void k_clip_enhance(const ClipGlyphPlane p, float contrast, float brightness, int threshold) {
  const long lanes = p.tall.plane_pitch / 16 * p.frame_height;  // of one frame
  const long lane = (long)blockIdx.x * kThreads + threadIdx.x;
  if (lane >= lanes) return;
  const int frame = blockIdx.y;
  const unsigned long long n = (unsigned long long)p.tall.width * (unsigned long long)p.frame_height;
  const int m = (int)((2 * p.tall.sum[frame] + n) / (2 * n));  // int(ImageStat.mean + 0.5) of this frame
  uint4 *q = reinterpret_cast<uint4 *>(p.tall.plane) + ((size_t)frame * (size_t)lanes + (size_t)lane);
  const uint4 v = *q;
  uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int i = 0; i < 4; i++) {
    uint32_t o = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      uint32_t x = (w[i] >> (8 * j)) & 0xFF;
      if (contrast != 1.0f) x = blend(m, (int)x, contrast);
      if (brightness != 1.0f) x = blend(0, (int)x, brightness);
      if (threshold >= 0) x = (int)x > threshold ? 255u : 0u;
      o |= x << (8 * j);
    }
    w[i] = o;
  }
  *q = make_uint4(w[0], w[1], w[2], w[3]);
}

// the bits of columns lane - rx .. lane + rx of a row whose words around the unit are prev, cur, next: bit j is column
// lane - rx + j (component_kernels.hip)
__device__ __forceinline__ uint64_t window(uint64_t prev, uint64_t cur, uint64_t next, int lane, int rx) {
  const int t = lane - rx + 64;  // 48 .. 126
  uint64_t v;
  if (t < 64) v = (prev >> t) | (cur << (64 - t));
  else if (t == 64) v = cur;
  else v = (cur >> (t - 64)) | (next << (128 - t));
  return v & ((2ull << (2 * rx)) - 1);
}

// ---- the union-find, once for the tile's labels in LDS (workgroup scope) and once for the global ones (agent scope) ----
template <int SCOPE>
__device__ __forceinline__ int32_t root_of(const int32_t *label, int32_t i) {
  for (;;) {
    const int32_t parent = __hip_atomic_load(label + i, __ATOMIC_RELAXED, SCOPE);  // parent <= i
    if (parent == i) return i;
    i = parent;
  }
}

template <int SCOPE>
__device__ __forceinline__ void join(int32_t *label, int32_t a, int32_t b) {
  for (;;) {
    a = root_of<SCOPE>(label, a);
    b = root_of<SCOPE>(label, b);
    if (a == b) return;
    if (a < b) { const int32_t t = a; a = b; b = t; }
    const int32_t old = atomicMin(label + a, b);  // b < a
    if (old == a) return;  // a was a root still: it hangs under b now
    a = old;               // another join hung a under `old` first: old < a, and old and b are still to be joined
  }
}

constexpr int kTile = __HIP_MEMORY_SCOPE_WORKGROUP, kPlane = __HIP_MEMORY_SCOPE_AGENT;

__global__ __launch_bounds__(kThreads) void k_clip_cc_tile(const ClipComponentPlane c, int ink_level, int rx, int ry) {
  __shared__ uint64_t word[kClipTileH];
  __shared__ int32_t lab[kClipTileW * kClipTileH];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int tx = blockIdx.x, ty = blockIdx.y, frame = blockIdx.z;
  const int x = tx * kClipTileW + lane;
  const int y0 = ty * kClipTileH;                                       // the tile's first row inside the frame
  const size_t row0 = (size_t)frame * (size_t)c.frame_height + (size_t)y0;  // ... and in the tall plane
  // 1  ink words and the labels' first state
  for (int ly = wave; ly < kClipTileH; ly += kWaves) {
    const bool row = y0 + ly < c.frame_height;  // (wave-uniform: the last tile row of a frame is short)
    int v = 255;
    if (row && x < c.tall.plane_pitch) v = c.tall.plane[(row0 + ly) * (size_t)c.tall.plane_pitch + (size_t)x];
    const bool ink = row && x < c.tall.width && v < ink_level;
    const uint64_t w = __ballot(ink);
    if (lane == 0) {
      word[ly] = w;
      if (row) c.tall.bits[(row0 + ly) * (size_t)c.tall.words_per_row + tx] = w;
    }
    const uint64_t below = ~w & ((1ull << lane) - 1);  // background to the left of this lane
    const int start = below ? 64 - __builtin_clzll(below) : 0;
    lab[ly * kClipTileW + lane] = ink ? ly * kClipTileW + start : -1;
  }
  __syncthreads();
  // 2  the forward half of every ink pixel's neighbourhood inside the tile
  for (int ly = wave; ly < kClipTileH; ly += kWaves) {
    const uint64_t cur = word[ly];
    if (cur == 0 || !((cur >> lane) & 1)) continue;
    const int32_t p = ly * kClipTileW + lane;
    const bool left_ink = lane > 0 && ((cur >> (lane - 1)) & 1);
    const uint64_t right = window(0, cur, 0, lane, rx) >> (rx + 1);
    if (right) {
      const int d = __builtin_ctzll(right);
      if (d > 0) join<kTile>(lab, p, p + 1 + d);  // (at distance 1 the first state has joined them already)
    }
    for (int dy = 1; dy <= ry && ly + dy < kClipTileH; dy++) {
      const uint64_t cu = word[ly + dy];  // (0 for the rows past the frame's last)
      if (cu == 0) continue;
      const uint64_t v = window(0, cu, 0, lane, rx);
      uint64_t starts = v & ~(v << 1);
      if (left_ink) starts &= 1ull << (2 * rx);
      const int32_t row = (ly + dy) * kClipTileW + lane - rx;
      while (starts) {
        const int j = __builtin_ctzll(starts);
        starts &= starts - 1;
        join<kTile>(lab, p, row + j);  // (a set bit is a column of the tile: 0 <= lane - rx + j < 64)
      }
    }
  }
  __syncthreads();
  // 3  local root -> tall index (nothing writes lab[] any more)
  for (int ly = wave; ly < kClipTileH; ly += kWaves) {
    if (y0 + ly >= c.frame_height || x >= c.tall.width) continue;
    const int32_t l = lab[ly * kClipTileW + lane];
    int32_t out = -1;
    if (l >= 0) {
      const int32_t r = root_of<kTile>(lab, l);
      out = (int32_t)((row0 + (size_t)(r / kClipTileW)) * (size_t)c.tall.width + (size_t)(tx * kClipTileW + (r & (kClipTileW - 1))));
    }
    c.tall.label[(row0 + ly) * (size_t)c.tall.width + (size_t)x] = out;
  }
}

// unit -> (tall row y, word w); false past the last one (wave-uniform)
__device__ __forceinline__ bool unit_of(const ComponentPlane &c, long &unit, int &y, int &w) {
  unit = (long)blockIdx.x * kWaves + (threadIdx.x / kWave);
  if (unit >= (long)c.height * c.words_per_row) return false;
  y = (int)(unit / c.words_per_row);
  w = (int)(unit - (long)y * c.words_per_row);
  return true;
}

__global__ __launch_bounds__(kThreads) void k_clip_cc_seams(const ClipComponentPlane cp, int rx, int ry) {
  const ComponentPlane &c = cp.tall;
  long unit; int y, w;
  if (!unit_of(c, unit, y, w)) return;
  const uint64_t cur = c.bits[unit];  // (the ink words are the tile launch's: plain loads)
  if (cur == 0) return;
  const int yf = y % cp.frame_height;       // the row inside its frame
  const int ly = yf % kClipTileH;           // ... and inside its tile
  const int rows = min(ry, cp.frame_height - 1 - yf);  // rows below that belong to the frame
  const bool has_prev = w > 0, has_next = w + 1 < c.words_per_row;
  // interior: no row below lies in another tile row, and no ink within reach_x of a neighbouring word
  const bool crosses_down = ly + rows >= kClipTileH;
  const uint64_t near_edge = (has_prev ? (1ull << rx) - 1 : 0) | (has_next ? ~0ull << (kWave - rx) : 0);
  if (!crosses_down && (cur & near_edge) == 0) return;
  const int lane = threadIdx.x & (kWave - 1);
  if (!((cur >> lane) & 1)) return;
  const uint64_t prev = has_prev ? c.bits[unit - 1] : 0, next = has_next ? c.bits[unit + 1] : 0;
  const int x = w * kWave + lane;
  const int32_t p = (int32_t)((size_t)y * c.width + x);
  const bool left_ink = lane > 0 ? (cur >> (lane - 1)) & 1 : (prev >> 63) & 1;
  const uint64_t right = window(prev, cur, next, lane, rx) >> (rx + 1);
  if (right) {
    const int d = __builtin_ctzll(right);
    if (lane + 1 + d >= kWave) join<kPlane>(c.label, p, p + 1 + d);  // the nearest ink to the right lies in the next word
  }
  // the columns of a window that belong to this unit's word: bits rx - lane .. rx - lane + 63
  const int lo = rx - lane, hi = rx - lane + kWave;  // (hi >= 1)
  const uint64_t own_word = (hi >= 64 ? ~0ull : (1ull << hi) - 1) & (lo > 0 ? ~0ull << lo : ~0ull);
  for (int dy = 1; dy <= rows; dy++) {
    const long below = unit + (long)dy * c.words_per_row;
    const uint64_t cu = c.bits[below], pr = has_prev ? c.bits[below - 1] : 0, nx = has_next ? c.bits[below + 1] : 0;
    if ((cu | pr | nx) == 0) continue;
    const uint64_t v = window(pr, cu, nx, lane, rx);
    uint64_t starts = v & ~(v << 1);
    if (left_ink) starts &= 1ull << (2 * rx);
    if (ly + dy < kClipTileH) starts &= ~own_word;  // same tile row: the tile launch made the joins inside the word
    const int32_t row = (int32_t)((size_t)(y + dy) * c.width) + x - rx;
    while (starts) {
      const int j = __builtin_ctzll(starts);
      starts &= starts - 1;
      join<kPlane>(c.label, p, row + j);
    }
  }
}

__global__ __launch_bounds__(kThreads) void k_clip_cc_flatten(const ComponentPlane c) {
  long unit; int y, w;
  if (!unit_of(c, unit, y, w)) return;
  const uint64_t cur = c.bits[unit];
  const int lane = threadIdx.x & (kWave - 1);
  if (!((cur >> lane) & 1)) return;
  const size_t p = (size_t)y * c.width + (size_t)(w * kWave + lane);
  // (entries other threads replace by their roots meanwhile are ancestors still: the sets are final since the seams ended)
  c.label[p] = root_of<kPlane>(c.label, (int32_t)p);
}

unsigned blocks_for(long n, int per_block) { return (unsigned)((n + per_block - 1) / per_block); }

}  // namespace

hipError_t launch_clip_plane(const ClipGlyphPlane &p, bool enhance, float contrast, float brightness, int threshold, hipStream_t s) {
  const long lanes = p.tall.plane_pitch / 16 * p.frame_height;
  const dim3 grid(blocks_for(lanes, kThreads), (unsigned)p.frames), block(kThreads);
  if (p.tall.bands == 3) hipLaunchKernelGGL(k_clip_luma<3>, grid, block, 0, s, p);
  else if (p.tall.bands == 4) hipLaunchKernelGGL(k_clip_luma<4>, grid, block, 0, s, p);
  else hipLaunchKernelGGL(k_clip_luma<1>, grid, block, 0, s, p);
  if (enhance) hipLaunchKernelGGL(k_clip_enhance, grid, block, 0, s, p, contrast, brightness, threshold);
  return hipGetLastError();
}

hipError_t launch_clip_cc_label(const ClipComponentPlane &c, int ink_level, int reach_x, int reach_y, hipStream_t s) {
  const dim3 block(kThreads);
  hipLaunchKernelGGL(k_clip_cc_tile, dim3((unsigned)c.tiles_x, (unsigned)c.tiles_y, (unsigned)c.frames), block, 0, s, c, ink_level, reach_x, reach_y);
  if (c.tiles_x * c.tiles_y > 1) {  // (a frame of one tile has no seam, and its roots are final)
    const dim3 grid(blocks_for((long)c.tall.height * c.tall.words_per_row, kWaves));
    hipLaunchKernelGGL(k_clip_cc_seams, grid, block, 0, s, c, reach_x, reach_y);
    hipLaunchKernelGGL(k_clip_cc_flatten, grid, block, 0, s, c.tall);
  }
  return hipGetLastError();
}

}  // namespace bnn
