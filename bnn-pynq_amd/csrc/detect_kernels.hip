// The detections' kernels (detect_kernels.h; the model: detect.h; DESIGN.md 9, "Detections").
//
// A window's key is ((score + 32768) << 6 | class) + 1, or 0 when it is no candidate: the score as an unsigned 16-bit
// number u orders the candidates, and the two histogram passes of k_detect_frame run over its high and its low byte.
// A sort entry is (65535 - u) << 26 | index << 6 | class: ascending entries are score descending, then index ascending.
#define BNN_HD __host__ __device__
#include "detect_kernels.h"

namespace bnn {
namespace {

constexpr int kB = kDetectFrameBlock, kWaves = kB / 64, kCap = kDetectMaxCandidates;
static_assert(kCap == 4 * kB && kCap / 32 <= kB, "the sort and the alive bits are laid out for 4096 entries and 1024 threads");

__global__ __launch_bounds__(kDetectKeyBlock) void k_detect_keys(const int16_t *__restrict__ scores, const int32_t *__restrict__ classes,
                                                                  uint32_t *__restrict__ keys, int total, int number_class,
                                                                  unsigned long long class_mask, int only, int min_score) {
  const int g = blockIdx.x * kDetectKeyBlock + threadIdx.x;
  if (g >= total) return;
  const int16_t *__restrict__ row = scores + (size_t)g * 64;
  int cls;
  if (only >= 0) {
    cls = only;
  } else if (classes) {
    cls = classes[g];
  } else {  // the decode restated: first strict maximum, floored at 0
    int bestv = 0;
    cls = 0;
    for (int c = 0; c < number_class; c++) {
      const int s = row[c];
      if (s > bestv) { bestv = s; cls = c; }
    }
  }
  cls &= 63;  // (a class is 0 .. 63: the read below stays inside the row whatever `classes` holds)
  const int s = row[cls];
  const bool cand = ((class_mask >> cls) & 1ull) && s > min_score;
  keys[g] = cand ? ((((uint32_t)(s + 32768)) << 6 | (uint32_t)cls) + 1u) : 0u;
}

// exclusive prefix of `flag` over the block in thread order and the block's total; tot[kWaves] is this call's own LDS row
__device__ __forceinline__ int block_rank(bool flag, uint32_t *tot, int &total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long b = __ballot(flag);
  if (lane == 0) tot[wave] = (uint32_t)__popcll(b);
  __syncthreads();
  int before = 0;
  total = 0;
#pragma unroll
  for (int w = 0; w < kWaves; w++) {
    const int t = (int)tot[w];
    before += w < wave ? t : 0;
    total += t;
  }
  return before + __popcll(b & ((1ull << lane) - 1ull));
}

__global__ __launch_bounds__(kDetectFrameBlock) void k_detect_frame(const uint32_t *__restrict__ keys, const uint64_t *__restrict__ boxes,
                                                                     int32_t *__restrict__ dets, int32_t *__restrict__ counts,
                                                                     int32_t *__restrict__ n_candidates, int n, int max_candidates, int max_det,
                                                                     int iou_num, int iou_den) {
  __shared__ uint64_t s_key[kCap];
  __shared__ uint64_t s_box[kCap];
  __shared__ uint32_t s_hist[256];
  __shared__ uint32_t s_alive[kCap / 32];
  __shared__ uint32_t s_tot[4][kWaves];
  __shared__ int s_cut[6];  // total, cut score u, entries wanted at the cut, entries taken m
  const int tid = threadIdx.x, f = blockIdx.x;
  keys += (size_t)f * n;

  // ---- the cut score: the high byte, then the low byte among the keys of that high byte
  if (tid < 256) s_hist[tid] = 0;
  __syncthreads();
  for (int base = 0; base < n; base += kB) {
    const int i = base + tid;
    const uint32_t k = i < n ? keys[i] : 0u;
    if (k) atomicAdd(&s_hist[(k - 1u) >> 14], 1u);
  }
  __syncthreads();
  if (tid == 0) {
    int total = 0;
    for (int b = 0; b < 256; b++) total += (int)s_hist[b];
    int above = 0, b1 = 0;
    if (total > max_candidates) {
      for (b1 = 255; b1 > 0; b1--) {
        if (above + (int)s_hist[b1] >= max_candidates) break;
        above += (int)s_hist[b1];
      }
    }
    s_cut[0] = total; s_cut[4] = b1; s_cut[5] = above;
  }
  __syncthreads();
  const int total = s_cut[0];
  if (total == 0) {  // (uniform)
    if (tid == 0) { counts[f] = 0; n_candidates[f] = 0; }
    return;
  }
  if (total > max_candidates) {  // (uniform)
    const uint32_t b1 = (uint32_t)s_cut[4];
    if (tid < 256) s_hist[tid] = 0;  // (thread 0 read the first histogram before the barrier above)
    __syncthreads();
    for (int base = 0; base < n; base += kB) {
      const int i = base + tid;
      const uint32_t k = i < n ? keys[i] : 0u;
      if (k && ((k - 1u) >> 14) == b1) atomicAdd(&s_hist[((k - 1u) >> 6) & 255u], 1u);
    }
    __syncthreads();
    if (tid == 0) {
      int above = s_cut[5], b2;
      for (b2 = 255; b2 > 0; b2--) {
        if (above + (int)s_hist[b2] >= max_candidates) break;
        above += (int)s_hist[b2];
      }
      s_cut[1] = (int)(b1 << 8) | b2; s_cut[2] = max_candidates - above; s_cut[3] = max_candidates;
    }
  } else if (tid == 0) {  // everything takes part: nothing lies below u = 0
    s_cut[1] = 0; s_cut[2] = max_candidates; s_cut[3] = total;
  }
  __syncthreads();
  const uint32_t cut = (uint32_t)s_cut[1];
  const int want_eq = s_cut[2], m = s_cut[3];

  // ---- ordered compaction: what lies above the cut, and the first want_eq at the cut by index
  int run_eq = 0, run_take = 0;
  for (int base = 0, c = 0; base < n && run_take < m; base += kB, c ^= 2) {
    const int i = base + tid;
    const uint32_t k = i < n ? keys[i] : 0u;
    const uint32_t u = (k - 1u) >> 6;
    const bool eq = k && u == cut;
    int chunk_eq, chunk_take;
    const int eq_rank = run_eq + block_rank(eq, s_tot[c], chunk_eq);
    const bool take = k && (u > cut || (eq && eq_rank < want_eq));
    const int pos = run_take + block_rank(take, s_tot[c + 1], chunk_take);
    if (take && pos < kCap) s_key[pos] = (uint64_t)(65535u - u) << 26 | (uint64_t)(uint32_t)i << 6 | (uint64_t)((k - 1u) & 63u);
    run_eq += chunk_eq;
    run_take += chunk_take;
  }
  int P = 1;
  while (P < m) P <<= 1;
  for (int t = m + tid; t < P; t += kB) s_key[t] = ~0ull;
  __syncthreads();

  // ---- bitonic sort of the P entries, ascending
  for (int k2 = 2; k2 <= P; k2 <<= 1) {
    for (int j = k2 >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < (P >> 1); t += kB) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), ixj = i | j;
        const uint64_t a = s_key[i], b = s_key[ixj];
        const bool up = (i & k2) == 0;
        if ((a > b) == up) { s_key[i] = b; s_key[ixj] = a; }
      }
      __syncthreads();
    }
  }

  // ---- the greedy pass: the block keeps the next entry alive, all lanes mark its later overlappers of its class dead
  for (int t = tid; t < m; t += kB) s_box[t] = boxes[(s_key[t] >> 6) & 0xFFFFFu];
  if (tid < kCap / 32) {
    const int left = m - tid * 32;
    s_alive[tid] = left >= 32 ? ~0u : (left > 0 ? (1u << left) - 1u : 0u);
  }
  __syncthreads();
  const int words = (m + 31) >> 5;
  int kept = 0, next = 0;  // next: the first entry not yet passed
  while (kept < max_det) {
    int i = -1;
    for (int w = next >> 5; w < words; w++) {
      uint32_t bits = s_alive[w];
      if (w == (next >> 5)) bits &= ~0u << (next & 31);
      if (bits) { i = w * 32 + __ffs((int)bits) - 1; break; }
    }
    if (i < 0) break;  // (uniform: bits at and below the entry found are never cleared while it is looked for)
    const uint64_t ke = s_key[i], bx = s_box[i];
    const int cls = (int)(ke & 63u);
    const int al = (int)(bx & 0xFFFFu), au = (int)((bx >> 16) & 0xFFFFu), ar = (int)((bx >> 32) & 0xFFFFu), ab = (int)(bx >> 48);
    if (tid == 0) {
      int32_t *d = dets + ((size_t)f * max_det + kept) * kDetectFields;
      d[0] = al; d[1] = au; d[2] = ar; d[3] = ab;
      d[4] = cls; d[5] = 32767 - (int)(ke >> 26); d[6] = (int)((ke >> 6) & 0xFFFFFu); d[7] = ar - al;
    }
    for (int j = i + 1 + tid; j < m; j += kB) {
      if (!((s_alive[j >> 5] >> (j & 31)) & 1u) || (int)(s_key[j] & 63u) != cls) continue;
      const uint64_t bj = s_box[j];
      if (detect_suppresses(al, au, ar, ab, (int)(bj & 0xFFFFu), (int)((bj >> 16) & 0xFFFFu), (int)((bj >> 32) & 0xFFFFu), (int)(bj >> 48), iou_num,
                            iou_den))
        atomicAnd(&s_alive[j >> 5], ~(1u << (j & 31)));
    }
    kept++;
    next = i + 1;
    __syncthreads();
  }
  if (tid == 0) { counts[f] = kept; n_candidates[f] = total; }
}

}  // namespace

hipError_t run_detect(const DetectLaunch &a) {
  const DetectOpts &o = a.opts;
  if (a.n < 1 || a.frames < 1 || (long)a.n * a.frames > kDetectMaxWindows || o.max_candidates < 1 || o.max_candidates > kDetectMaxCandidates ||
      o.max_det < 1 || o.max_det > o.max_candidates || a.number_class < 1 || a.number_class > 64)
    return hipErrorInvalidValue;
  int only = -1;
  if (o.by_score)
    for (only = 0; only < 63 && !((o.class_mask >> only) & 1); only++) {}
  const int total = a.n * a.frames;
  hipError_t e = hipMemsetAsync(a.dets, 0, (size_t)a.frames * o.max_det * kDetectFields * sizeof(int32_t), a.stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_detect_keys, dim3((unsigned)((total + kDetectKeyBlock - 1) / kDetectKeyBlock)), dim3(kDetectKeyBlock), 0, a.stream, a.scores,
                     a.classes, a.keys, total, a.number_class, (unsigned long long)o.class_mask, only, o.min_score);
  hipLaunchKernelGGL(k_detect_frame, dim3((unsigned)a.frames), dim3(kDetectFrameBlock), 0, a.stream, a.keys, a.boxes, a.dets, a.counts, a.n_candidates,
                     a.n, o.max_candidates, o.max_det, o.iou_num, o.iou_den);
  return hipGetLastError();
}

}  // namespace bnn
