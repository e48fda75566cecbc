// The matrix-core form of the clip scan's stages 1-3 (scan_clip.h, ClipMfmaTables; DESIGN.md 9 "Clip scan"): layers 1-3 of
// cnvW1A1 over all (frame, level) maps of a clip as exact FP4 GEMMs, one launch per stage, writing the maps k_clip_quad
// writes, byte for byte.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "scan_clip.h"

namespace bnn {

// static LDS of k_clip_conv_mfma<CD, ..>: the band's FP4 patch [CD 32-channel blocks][18 rows][66 columns] x 16 bytes and
// the 256-entry expansion table: 39 040 bytes (layers 1 and 2), 77 056 (layer 3: two blocks fit the 160 KiB of a CU)
constexpr int clip_mfma_lds_bytes(int cd) { return cd * (2 * kClipMfmaRowPairs + 2) * (kClipMfmaChunk + 2) * 16 + 256 * 4; }

struct ClipMfmaLaunch {
  const uint8_t *in;    // device: the buffer holding stage - 1's maps
  uint8_t *out;         // device: the buffer stage's maps go to
  const uint8_t *tab;   // device: the layer's operand table (kernels.h, conv_mfma_table: weights, then seeds)
  const int32_t *maps;  // device copy of ClipMfmaTables::words at maps[stage] (16-byte aligned)
  const int32_t *bands; // ... at bands[stage]
  long blocks;          // ClipMfmaTables::blocks[stage]
  hipStream_t stream;
};
// stage 1, 2 or 3; anything else is hipErrorInvalidValue
hipError_t launch_clip_conv_mfma(int stage, const ClipMfmaLaunch &a);

}  // namespace bnn
