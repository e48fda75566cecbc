// Device half of the pixel formats (pixfmt.h states the model; DESIGN.md 9, "Camera frames"): one streaming launch.
//   k_unpack_frames<FORMAT>  blockIdx.y is the frame; a lane takes 8 pixels of one row -- of two rows for NV12 and I420,
//                            whose 8 chroma bytes are read once for both -- with 8- or 16-byte loads and writes the 24 RGB
//                            bytes of each row with 8-byte stores.  Row tails, and bases or strides those accesses cannot
//                            take, go byte by byte through pix_unpack_one, the host loop's own routine.
// No LDS, no scratch; every byte of the RGB frames is written and nothing outside them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pixfmt.h"

namespace bnn {

constexpr int kUnpackBlock = 256;  // threads of a k_unpack_frames block
constexpr int kUnpackPixels = 8;   // pixels of one row a lane takes

struct UnpackLaunch {
  const uint8_t *src;  // device: the frames as validate_frames accepted them; read only
  uint8_t *dst;        // device: [n_frames][height][width][3]
  Frames frames;
  PixLayout layout;
  hipStream_t stream;
};
// Enqueues the launch on a.stream.  The caller has validated (validate_frames).
hipError_t run_unpack_frames(const UnpackLaunch &a);

}  // namespace bnn
