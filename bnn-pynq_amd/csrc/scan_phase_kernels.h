// Stages 2 and 3 of the fine clip scan on the matrix cores (scan_fine.h, ClipPhaseTables; DESIGN.md 9 "Fine scan"): layers 2
// and 3 of cnvW1A1 over maps of ANY extents, layer 3 leaving the four pool phases of one evaluation of its convolution.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "scan_fine.h"

namespace bnn {

// static LDS of k_clip_conv_phase<CD, ..>: the band's FP4 patch [CD 32-channel blocks][18 rows][66 columns] x 16 bytes and the
// 256-entry expansion table: 39 040 bytes (stage 2), 77 056 (stage 3: two blocks fit the 160 KiB of a CU)
constexpr int clip_phase_lds_bytes(int cd) { return cd * (kPhaseRows + 2) * (2 * kPhaseTile + 2) * 16 + 256 * 4; }

struct ClipPhaseLaunch {
  const uint8_t *in;    // device: the buffer holding stage - 1's maps
  uint8_t *out;         // device: the buffer stage's maps go to
  const uint8_t *tab;   // device: the layer's operand table (kernels.h, conv_mfma_table: weights, then seeds)
  const int32_t *maps;  // device copy of ClipPhaseTables::words at maps[stage - 2] (8-byte aligned)
  const int32_t *bands; // ... at bands[stage - 2]
  long blocks;          // ClipPhaseTables::blocks[stage - 2]
  hipStream_t stream;
};
// stage 2 or 3; anything else is hipErrorInvalidValue
hipError_t launch_clip_conv_phase(int stage, const ClipPhaseLaunch &a);

}  // namespace bnn
