// The matrix-core form of the single-fault sweeps (fault_sweep, act_fault_sweep, input_fault_sweep; DESIGN.md 9 "Sweeps on
// the matrix cores"): layers 1-7 of the three CNV nets as the exact FP4 GEMMs of k_conv_mfma / k_conv_mfma_a2 / k_tail_mfma,
// with the work split by a LIST OF ALIVE SLOTS instead of by batch or by segment record.
//
// Why a form of its own: a sweep is a run per fault, and pruning cuts its segments short -- three survivors of a record
// would fill 3 of the 128 rows of a layer-6 tile of the segment kernels (multi_mfma_kernels.h) and reload the weights for
// them.  But in almost every stage of a sweep all runs read the SAME parameters: the activation and input sweeps read the
// loaded blob, and in the parameter sweep every layer behind the faulted one holds the loaded rows in every copy.  So the
// tables load_parameters made serve all surviving pairs of the stage at once, and a tile can be packed from survivors
// wherever their slots lie.
//
// Split of a launch: grid min(ceil(count / G), resident blocks), nothing in y.  A block loads its wave's neuron tile(s) of
// the tables into VGPRs once and walks tiles t = blockIdx.x, t += gridDim.x.  Tile t is list entries [t G, t G + G) (G = 2
// for layer 1, 8 for layers 2-3, 32 / 32 / 128 / 128 for layers 4-7); its slots go to LDS once per tile, a step ahead of
// the tile's source loads.  Image i of the tile reads in + slot_i * (an image's input) and writes out + slot_i * (an
// image's output): the slots run_cnv_multi's integer kernels read and write, byte for byte.  Entries past `count` in the
// last tile repeat the last slot and store nothing; a slot that is not on the list is never touched.
//
// Built figures (gfx950, tests/test_list_matrix_build.py holds them to the occupancy the launch bounds claim; no scratch,
// no spills) -- VGPRs / static LDS bytes:
//   k_list_conv_mfma     layer 1: 173 / 58 640    layer 2: 166 / 51 264    layer 3: 217 / 81 216
//   k_list_conv_mfma_a2  layer 1: 209 / 59 664    layer 2: 222 / 52 288    layer 3: 254 / 75 840
//   k_list_tail_mfma     1-bit  layers 4-7: 163 / 53 504, 211 / 40 320, 196 / 20 608, 178 / 37 120
//                        2-bit  layers 4-7: 187 / 55 552, 220 / 42 368, 234 / 23 680, 207 / 40 192
// Every one stays within 256 VGPRs (two waves per SIMD) and within half a CU's 160 KiB of LDS where two blocks share a CU
// (the 4-wave kernels: layers 1-3 and 6).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "topology.h"

namespace bnn {

struct ListLaunch {
  const uint32_t *list;   // device, the alive slots of this stage in ascending order
  int count;              // entries of the list (>= 1)
  void *buf0, *buf1;      // the activation buffers (odd layers read buf0 and write buf1, even layers the other way round)
  const uint8_t *tables;  // device, the operand tables of layers 1-7 (conv_mfma_table / conv_mfma_a2_table)
  hipStream_t stream;
};

// Layer `layer` (1 ... 7) of the slots on the list on the matrix cores.  hipErrorInvalidValue: another layer, an LFC net,
// no tables, no list.
hipError_t run_cnv_list_mfma(NetId net, int layer, const ListLaunch &a);

}  // namespace bnn
