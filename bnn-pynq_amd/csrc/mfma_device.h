// The device helpers the matrix forms of the fault launches are written with (multi_mfma_kernels.hip: by segment record;
// list_mfma_kernels.hip: by slot list): the FP4 encodings, the sign-bit epilogues and the LDS strides of k_conv_mfma,
// k_conv_mfma_a2 and k_tail_mfma (kernels.hip, whose comments derive them; that file's own are in its anonymous namespace).
// Device code only: include from a .hip file, inside no namespace.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bnn {
namespace {

typedef int v8i __attribute__((ext_vector_type(8)));
typedef float v16f __attribute__((ext_vector_type(16)));
typedef const uint32_t __attribute__((address_space(4))) *kptr32;  // scalar (constant) address space: uniform loads become s_load_*

// bits = (bits << 1) | (v < 0)
__device__ __forceinline__ uint32_t shift_in_sign(uint32_t bits, int v) {
  asm("" : "+v"(v));
  return __builtin_amdgcn_alignbit(bits, (uint32_t)v, 31);
}
// sign bits of the 16 accumulators of one lane -> bits 8g + 4h + q of a dword (other bits 0)
__device__ __forceinline__ uint32_t sign_nibbles(const int (&v)[16], int h) {
  uint32_t x = 0;
#pragma unroll
  for (int g = 3; g >= 0; g--) {
#pragma unroll
    for (int q = 3; q >= 0; q--) x = shift_in_sign(x, v[4 * g + q]);
    if (g) x <<= 4;
  }
  return x << (4 * h);
}
// OR with the partner lane l ^ 32
__device__ __forceinline__ uint32_t or_halves(uint32_t x) {
  const auto sw = __builtin_amdgcn_permlane32_swap(x, x, false, false);
  return sw[0] | sw[1];
}
// 8 bits -> 8 FP4 nibbles, bit i -> nibble i: 1 -> 0x2 (+1.0), 0 -> 0xA (-1.0)
__device__ __forceinline__ uint32_t fp4_pm1(uint32_t byte) {
  uint32_t t = ~byte & 0xFFu;
  t = (t | (t << 12)) & 0x000F000Fu;
  t = (t | (t << 6)) & 0x03030303u;
  t = (t | (t << 3)) & 0x11111111u;
  return (t << 3) + 0x22222222u;
}
// bit i of a byte -> 0x1 in nibble i
__device__ __forceinline__ uint32_t nibble_spread(uint32_t byte) {
  uint32_t t = byte & 0xFFu;
  t = (t | (t << 12)) & 0x000F000Fu;
  t = (t | (t << 6)) & 0x03030303u;
  return (t | (t << 3)) & 0x11111111u;
}
// 32 channels (non-zero bits nz, sign bits sg) -> 32 FP4 nibbles through the two tables (lutz: 0x2 per bit, luts: 0x8)
__device__ __forceinline__ uint4 fp4_planes(const uint32_t *lutz, const uint32_t *luts, uint32_t sg, uint32_t nz) {
  const uint32_t m = sg & nz;
  return make_uint4(lutz[nz & 255] | luts[m & 255], lutz[(nz >> 8) & 255] | luts[(m >> 8) & 255],
                    lutz[(nz >> 16) & 255] | luts[(m >> 16) & 255], lutz[nz >> 24] | luts[m >> 24]);
}
// !fire0 and !fire1 words (32 neurons, both lane halves) of 16 pooled or plain accumulators
__device__ __forceinline__ void not_fired(const v16f &acc, const v16f &dt, int h, uint32_t &n0, uint32_t &n1) {
  int v[16], u[16];
#pragma unroll
  for (int k = 0; k < 16; k++) {
    v[k] = __float_as_int(acc[k]);
    u[k] = __float_as_int(acc[k] - dt[k]);
  }
  n0 = or_halves(sign_nibbles(v, h));
  n1 = or_halves(sign_nibbles(u, h));
}
// the LDS row and image strides of k_conv_mfma's planes (kernels.hip derives them)
constexpr int conv_mfma_row_stride(int win) {
  int ws = win;
  while ((2 * ws - (win - 2)) % 16) ws++;
  return ws;
}
constexpr int conv_mfma_img_stride(int win, int cd) {
  const int ws = conv_mfma_row_stride(win);
  int s = cd * win * ws;
  while ((s - 2 * ((win - 2) / 2 - 1) * ws - (win - 2)) % 16) s++;
  return s;
}

}  // namespace
}  // namespace bnn
