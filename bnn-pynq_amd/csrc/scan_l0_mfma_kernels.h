// The matrix-core form of the clip scan's stage 0 (scan_clip.h, ClipL0Tables; DESIGN.md 9 "Clip scan"): layer 0 of cnvW1A1
// over all (frame, level) maps of a clip as int8 MFMAs, one launch, writing the maps k_clip_conv0 writes, byte for byte.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "scan_clip.h"

namespace bnn {

// LDS of k_clip_conv0_mfma: the band's quantised patch, 3 planes x (kClipL0Rows + 2) rows at a pitch of kClipL0Pitch bytes,
// and one more row, which the unused fifth fetch of lane half 1 reads behind the last plane.
// The pitch holds the 130 bytes of a patch row rounded up to dwords (132; the fetches of the last tile's lanes end there too)
// and is 32 mod 64: two rows are then 64 mod 128 bytes apart and so is a plane of 18 rows (2 880), which puts the two lane
// halves of every fetch -- a plane or two rows apart -- 16 banks apart, on 32 banks and on 64; a half touches at most ten
// consecutive banks (32 pixels + 7 bytes), so the halves never meet.
constexpr int kClipL0Pitch = 160, kClipL0Plane = (kClipL0Rows + 2) * kClipL0Pitch;
constexpr int kClipL0LdsBytes = 3 * kClipL0Plane + kClipL0Pitch;
static_assert(kClipL0Pitch % 64 == 32 && kClipL0Plane % 128 == 64 && kClipL0Pitch >= (kClipL0Cols + 2 + 3) / 4 * 4, "see above");

struct ClipL0Launch {
  const uint8_t *planes;  // device, 4-byte aligned: the call's planes, ClipL0Tables::planes_top bytes or more reserved
  uint8_t *out;           // device: buffer 0
  const uint8_t *tab;     // device: layer 0's MFMA table (packed_params.h, from l0_mfma_offset; the tile operands lie kL0MfmaTileOffset in)
  const int32_t *maps;    // device copy of ClipL0Tables::words at maps (8-byte aligned)
  const int32_t *bands;   // ... at bands
  long blocks;            // ClipL0Tables::blocks
  hipStream_t stream;
};
hipError_t launch_clip_conv0_mfma(const ClipL0Launch &a);

}  // namespace bnn
