// iwecc.h -- the bit exchange of the column-interleaved coded weight memories (the model: mem_org.h, "column-interleaved
// code words"; the kernels: iwecc_kernels.hip).
//
// A group of D = 2^LOGD code words lies on D adjacent lanes; lane i holds the 64 PHYSICAL bits at offsets [64 i, 64 i + 64)
// of the group, and offset p is data bit p / D of code word p % D.  So code word c's
//     bit i * (64 / D) + j  is  lane i's bit j * D + c:
// a local UNZIP of each lane's word into D sub-words of 64 / D bits (sub-word c = the lane's bits c, D + c, 2 D + c, ...),
// then a D x D TRANSPOSE of sub-words across the lanes (lane c's sub-word i <- lane i's sub-word c).  The way back is the
// transpose (an involution) and the zip.
//   The unzip moves the bit at index x = j * D + c to index c * (64 / D) + j: a rotation of the six index bits by LOGD.  A
//   permutation of index bits is a product of at most five transpositions, and swapping index bits a > b of every position
//   is one delta swap (mask: positions with bit b set and bit a clear; distance 2^a - 2^b).  The steps are worked out at
//   compile time.
//   The transpose is the usual butterfly: stage s trades, between lanes l and l ^ 2^s, the sub-words whose index differs
//   from the lane's own in bit s.  iwecc_stage is one lane's side of a stage, given the partner's word -- on the device a
//   __shfl_xor delivers it, on the host (tests/host_sanitize_iwecc) an array of lanes does.
// Everything here is plain integer code for host and device.
#pragma once
#include <stdint.h>

#ifndef BNN_HD
#define BNN_HD
#endif

namespace bnn {

// positions whose index has bit i set
constexpr uint64_t kIwIndexBit[6] = {0xAAAAAAAAAAAAAAAAull, 0xCCCCCCCCCCCCCCCCull, 0xF0F0F0F0F0F0F0F0ull,
                                     0xFF00FF00FF00FF00ull, 0xFFFF0000FFFF0000ull, 0xFFFFFFFF00000000ull};

struct IwSteps {
  uint64_t m[5];
  int sh[5];
  int n;
};

// the delta swaps of the unzip at depth 2^logd, in order (the zip applies them in reverse)
constexpr IwSteps iwecc_unzip_steps(int logd) {
  IwSteps u{};
  int cur[6] = {0, 1, 2, 3, 4, 5};  // cur[pos]: the original index bit that sits at index-bit position pos
  for (int pos = 0; pos < 6; pos++) {
    const int want = (pos + logd) % 6;
    if (cur[pos] == want) continue;
    int from = pos + 1;
    while (cur[from] != want) from++;
    u.m[u.n] = kIwIndexBit[pos] & ~kIwIndexBit[from];
    u.sh[u.n] = (1 << from) - (1 << pos);
    u.n++;
    cur[from] = cur[pos];
    cur[pos] = want;
  }
  return u;
}

template <int LOGD>
BNN_HD inline uint64_t iwecc_unzip(uint64_t x) {
  constexpr IwSteps u = iwecc_unzip_steps(LOGD);
#pragma unroll
  for (int i = 0; i < u.n; i++) {
    const uint64_t t = ((x >> u.sh[i]) ^ x) & u.m[i];
    x ^= t | (t << u.sh[i]);
  }
  return x;
}

template <int LOGD>
BNN_HD inline uint64_t iwecc_zip(uint64_t x) {
  constexpr IwSteps u = iwecc_unzip_steps(LOGD);
#pragma unroll
  for (int i = u.n - 1; i >= 0; i--) {
    const uint64_t t = ((x >> u.sh[i]) ^ x) & u.m[i];
    x ^= t | (t << u.sh[i]);
  }
  return x;
}

// stage s (0 ... LOGD - 1) of the transpose for a lane whose index has bit s = lane_bit: own sub-words whose index agrees
// with the lane in bit s stay; the others come from the partner's sub-word 2^s away
template <int LOGD, int S>
BNN_HD inline uint64_t iwecc_stage(uint64_t own, uint64_t partner, unsigned lane_bit) {
  static_assert(S >= 0 && S < LOGD && LOGD <= 4, "a stage per bit of the depth");
  constexpr uint64_t hi = kIwIndexBit[6 - LOGD + S];  // the bits of the sub-words whose index has bit S set
  constexpr int sh = 1 << (6 - LOGD + S);
  return lane_bit ? (own & hi) | ((partner & hi) >> sh) : (own & ~hi) | ((partner & ~hi) << sh);
}

// The check memory by offsets (8 / D may be half a bit, so no sub-words): code word c of a group takes its check bit k
// from offset r = k * D + c, that is element r >> 3, bit r & 7; element i's bit b (r = 8 i + b) is check bit r / D of code
// word r % D.
BNN_HD inline void iwecc_check_source(unsigned depth, unsigned word, unsigned k, unsigned *element, unsigned *bit) {
  const unsigned r = k * depth + word;
  *element = r >> 3;
  *bit = r & 7;
}
BNN_HD inline void iwecc_check_target(unsigned depth, unsigned element, unsigned b, unsigned *word, unsigned *k) {
  const unsigned r = 8 * element + b;
  *word = r % depth;
  *k = r / depth;
}

}  // namespace bnn
