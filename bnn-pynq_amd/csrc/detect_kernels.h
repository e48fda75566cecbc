// Device half of the detections (detect.h states the model; DESIGN.md 9, "Detections"): two launches on one stream.
//   k_detect_keys   a thread per window of every frame: (class, score) -> one 32-bit key, 0 for "not a candidate"
//   k_detect_frame  a block per frame: the first max_candidates keys in order (two histogram passes find the cut score,
//                   an ordered compaction takes what lies above it and the first at it by index), a bitonic sort of at
//                   most 4096 entries in LDS, and the greedy pass
// No block waits for another; every loop is bounded by n, by 4096 or by max_det.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "detect.h"

namespace bnn {

constexpr int kDetectKeyBlock = 256;     // threads of a k_detect_keys block
constexpr int kDetectFrameBlock = 1024;  // threads of a k_detect_frame block: 16 waves
// static LDS of k_detect_frame: 4096 x (8-byte sort entry + 8-byte box), the histogram, the alive bits, the wave totals, the cut
constexpr int kDetectLdsBytes = kDetectMaxCandidates * 16 + 256 * 4 + (kDetectMaxCandidates / 32) * 4 + 4 * 16 * 4 + 6 * 4;

// a box as the kernels hold it: left | upper << 16 | right << 32 | lower << 48 (every coordinate is 0 .. 65535)
inline uint64_t detect_pack_box(const int *b) {
  return (uint64_t)(uint16_t)b[0] | (uint64_t)(uint16_t)b[1] << 16 | (uint64_t)(uint16_t)b[2] << 32 | (uint64_t)(uint16_t)b[3] << 48;
}

struct DetectLaunch {
  const int16_t *scores;   // [frames * n][64], frame-major: what the decode kernels write
  const int32_t *classes;  // [frames * n] the decode's classes, or null: the key kernel restates the decode
  const uint64_t *boxes;   // [n] one frame's boxes (detect_pack_box)
  uint32_t *keys;          // [frames * n] workspace
  int32_t *dets;           // [frames][max_det][8], zeroed by run_detect
  int32_t *counts, *n_candidates;  // [frames]
  int n, frames, number_class;
  DetectOpts opts;
  hipStream_t stream;
};
// Enqueues the zeroing of dets and the two launches on a.stream.  The caller has validated (validate_detect*).
hipError_t run_detect(const DetectLaunch &a);

}  // namespace bnn
