// The matrix-core form of the clip scan's stages 4 and 5 (scan_clip.h, ClipTailTables; DESIGN.md 9 "Clip scan"): layers 4
// and 5 of cnvW1A1 over all (frame, level) maps of a clip as exact FP4 GEMMs, one launch per stage, writing the maps
// k_clip_vec<2> and k_clip_vec<4> write, byte for byte.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "scan_clip.h"

namespace bnn {

// static LDS of k_clip_tail_mfma<CD>: the band's FP4 patch [CD 32-channel blocks][10 rows][66 columns] x 16 bytes and the
// 256-entry expansion table: 43 264 bytes (stage 4, CD = 4), 85 504 (stage 5, CD = 8).  One block of eight waves is
// resident on a CU (two waves a SIMD, by registers), so either fits the CU's 160 KiB.
constexpr int clip_tail_lds_bytes(int cd) { return cd * (2 * kClipTailRowPairs + 2) * (kClipTailCols + 2) * 16 + 256 * 4; }

struct ClipTailLaunch {
  const uint8_t *in;    // device: the buffer holding stage - 1's maps
  uint8_t *out;         // device: the buffer stage's maps go to
  const uint8_t *tab;   // device: the layer's operand table (kernels.h, conv_mfma_table at kTailMfmaL4Off / L5Off: weights, then seeds)
  const int32_t *maps;  // device copy of ClipTailTables::words at maps[stage - 4] (16-byte aligned)
  const int32_t *bands; // ... at bands[stage - 4]
  long blocks;          // ClipTailTables::blocks[stage - 4]
  hipStream_t stream;
};
// stage 4 or 5; anything else is hipErrorInvalidValue
hipError_t launch_clip_tail_mfma(int stage, const ClipTailLaunch &a);

}  // namespace bnn
