// The matrix-core form of the campaign launches (kernels.h, MultiLaunch; DESIGN.md 5 "The matrix pipe", 9 "Campaigns on the
// matrix cores"): layers 1-7 of the three CNV nets as the exact FP4 GEMMs of k_conv_mfma / k_conv_mfma_a2 / k_tail_mfma, with
// the work split by SEGMENT RECORD instead of by batch.  Every run of a campaign has its own (faulted) copy of the blob, so
// every run has its own operand tables, made on the device from its copy; a block takes its run's tables from its record.
//
// Which paths take it: fault_campaigns, act_noise_campaigns, mem_noise_campaigns and its hardened, exposure, ecc, repair,
// wecc and iwecc successors -- everything that goes through run_cnv_multi with MultiLaunch::multi_mfma set.  Which keep the
// integer pipe whatever the form: act_window, input_noise_campaigns (it classifies by the fault-free pass), the LFC nets, layers 0
// and 8 of every net, and every call under BNN_MI355X_CONV=valu.  The single-fault sweeps (a run per fault, segments pruned
// short) take neither these kernels nor the integer pipe under form 1 but the slot-list kernels of list_mfma_kernels.h.
//
// Split of a launch: grid (bx, nsegs).  Block (x, y) reads record y with scalar loads, loads its wave's neuron tile(s) of
// run `run`'s tables into VGPRs once, and walks the record's image groups x, x + bx, ... (G images each: 2 for layer 1, 8
// for layers 2-3, 32 / 32 / 128 / 128 for layers 4-7).  bx = multi_mfma_bx(groups of the longest record, nsegs, resident
// blocks of the kernel): the groups of the longest record dealt evenly over at most max(1, resident / nsegs) blocks.  Few
// long records: as many blocks per record as keep the chip full, each reloading its weights once per resident / nsegs
// groups at worst.  Many short records (nsegs >= resident): one block per record, weights loaded once per record.  Blocks
// with no group in their record (a record shorter than the longest) exit before touching LDS.
//
// Built figures (gfx950, tests/test_campaign_matrix_build.py holds them to the occupancy the launch bounds claim; no
// scratch, no spills) -- VGPRs / static LDS bytes:
//   k_seg_conv_mfma     layer 1: 194 / 58 624    layer 2: 181 / 51 200    layer 3: 245 / 81 152
//   k_seg_conv_mfma_a2  layer 1: 195 / 59 648    layer 2: 214 / 52 224    layer 3: 245 / 75 776
//   k_seg_tail_mfma     1-bit  layers 4-7: 164 / 53 248, 202 / 40 064, 189 / 19 584, 175 / 36 096
//                       2-bit  layers 4-7: 182 / 55 296, 216 / 42 112, 234 / 22 656, 206 / 39 168
// Every one stays within 256 VGPRs (two waves per SIMD) and within half a CU's 160 KiB of LDS where two blocks share a CU
// (the 4-wave kernels: layers 1-3 and 6).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"

namespace bnn {

// the stages the form covers (bit k: stage k = layer k)
constexpr int kCampaignMatrixStages = 0xFE;
// table memory of one call, runs x multi_mfma_bytes: above it the call runs the integer pipe (1 GiB: 1 390 runs of cnvW1A1)
constexpr size_t kCampaignTableCap = (size_t)1 << 30;

// bytes of one run's tables: kConvMfmaBytes (cnvW1A1) or kConvMfmaA2Bytes (cnvW1A2, cnvW2A2), a multiple of 256; 0: an LFC net
size_t multi_mfma_bytes(NetId net);

// grid.x of a segment launch (see above)
inline unsigned multi_mfma_bx(long long groups, int nsegs, long long resident) {
  const long long cap = resident / (nsegs > 0 ? nsegs : 1) > 1 ? resident / nsegs : 1;
  const long long per = (groups + cap - 1) / cap;
  return (unsigned)(per > 0 ? (groups + per - 1) / per : 1);
}

// The tables of `runs` runs, one launch per layer (blockIdx.y = run): run q's from the packed rows rows[l] + q * stride / 4
// (stride: bytes between two runs' copies of the blob) to dst + q * tab_stride, in the layouts of conv_mfma_table
// (cnvW1A1) / conv_mfma_a2_table (the 2-bit nets; cnvW2A2's -2 from the row's "weight is -2" plane).  Enqueued on s.
hipError_t multi_mfma_tables(NetId net, const uint32_t *const rows[9], size_t stride, int runs, uint8_t *dst, size_t tab_stride, hipStream_t s);

// Layer `layer` (1 ... 7) of the records of `a` on the matrix cores: a.multi_mfma is run 0's tables, run q's a.mfma_stride
// bytes behind (0: every run reads the same ones).  Reads and writes the activation slots run_cnv_multi's integer kernels
// do, byte for byte.  hipErrorInvalidValue: another layer, an LFC net, no tables.
hipError_t run_cnv_multi_mfma(NetId net, int layer, const MultiLaunch &a);

}  // namespace bnn
