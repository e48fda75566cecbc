// The matrix-core form of the four LFC layers (lfcW1A1, lfcW1A2; DESIGN.md 5 "The matrix pipe", "LFC"): every layer an exact
// FP4 GEMM, n images x 1024 (last layer: 64) neurons x 832 or 1024 synapses, one launch per layer, writing the words k_vec_x
// and k_vec write, byte for byte.  run_lfc (kernels.hip) takes it where lfc_mfma_for() says so: BNN_MI355X_LFC=mfma, from
// BNN_MI355X_LFC_MFMA_MIN images on.  Nothing selects it by default.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "topology.h"

namespace bnn {

// The tiling (lfc_mfma_kernels.hip).  A block of kLfcMfmaWaves waves takes kLfcMfmaGroup images at a time, 32 of them (the
// MFMA's item tile) per accumulator tile; a wave keeps kLfcMfmaTilesPerWave 32-neuron tiles of weights in VGPRs, so a block
// covers 16 of a hidden layer's 32 tiles and two blocks (blockIdx & 1) share a group of images.  At most kLfcMfmaGrid groups
// are in flight per layer; a block takes groups kLfcMfmaGrid apart (in a launch of more than that many groups) one after
// the other, the next one's words on their way while this one's MFMAs run.
constexpr int kLfcMfmaWaves = 8, kLfcMfmaGroup = 128, kLfcMfmaItemTile = 32, kLfcMfmaTilesPerWave = 2;
constexpr int kLfcMfmaGrid = 128;  // 2 x 128 blocks of the hidden layers: one per CU (a wave holds up to 256 VGPRs)

// k steps (64 synapses each) and neuron tiles of layer l: 784 inputs padded to 832 (the reference's padding: 48 inputs of
// bit 0 = -1 against the weight memories' own bits, which its thresholds count: real synapses, not zeros), 1024 hidden
// neurons, 64 output rows (10 classes and padding)
constexpr int lfc_mfma_ksteps(int l) { return l == 0 ? 13 : 16; }
constexpr int lfc_mfma_tiles(int l) { return l == 3 ? 2 : 32; }

// The operand tables (made on the device by lfc_mfma_table, kernels.hip, with the table kernels of k_tail_mfma): per layer
// the weights [k step][neuron tile][lane 0..63] x 16 bytes of FP4 (+1 = 0x2, -1 = 0xA; lane (r, h) holds synapses 32h ..
// 32h + 31 of the step for neuron 32 * tile + r), then the seeds [tile][h][16] floats, then -- lfcW1A2 (`two`) -- the second
// threshold's distance from the first, [tile][h][16] floats.
constexpr size_t lfc_mfma_layer_bytes(int l, bool two) {
  return (size_t)lfc_mfma_ksteps(l) * lfc_mfma_tiles(l) * 64 * 16 + (size_t)lfc_mfma_tiles(l) * 32 * 4 * (two ? 2 : 1);
}
constexpr size_t lfc_mfma_offset(int l, bool two) { return l == 0 ? 0 : lfc_mfma_offset(l - 1, two) + lfc_mfma_layer_bytes(l - 1, two); }
constexpr size_t lfc_mfma_bytes(bool two) { return lfc_mfma_offset(4, two); }

// Layer `layer` (0..3) of `net` over n images on stream s.  in: layer 0 the 13 binarised u64 of every image, else the
// previous layer's words; out: [image][32] dwords (lfcW1A1), [image][16][plane] u64 (lfcW1A2), last layer [image] u64;
// tab: the net's table (all layers).  hipErrorInvalidValue for another net or layer.
hipError_t launch_lfc_mfma(NetId net, int layer, const void *in, void *out, const uint8_t *tab, int n, hipStream_t s);

}  // namespace bnn
