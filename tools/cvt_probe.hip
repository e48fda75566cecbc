// tools/cvt_probe.hip -- what the two sign collections of the matrix-form conv kernels cost to issue ("The
// matrix pipe"): SIMD-cycles per instruction of
//   stream 0: a dependent v_alignbit_b32 chain (sign_nibbles: one per accumulator),
//   stream 1: v_cvt_scalef32_pk_fp4_f32 as a packed collection issues it (built and not kept, CHANGELOG) -- eight read-modify-write conversions into two
//             destinations, byte selects 0..3,
// each with the wave alone on its SIMD (256-thread blocks, one per CU) and with a second resident wave on the SIMD that
// issues v_mfma_scale_f32_32x32x64_f8f6f4 back to back (512-thread blocks: waves w and w + 4 share a SIMD; waves 4-7
// run the MFMAs and outlast the measured waves).  Cycles from s_memtime around the loop, the clock from s_memtime /
// s_memrealtime (100 MHz).  A second entry converts given values once, so that the driver can show which nibble a source
// lands in and what the sign bit of -0, of values that round to zero and of saturating values becomes.
// Not part of the product libraries.
//
//   hipcc -O3 -std=c++17 -fPIC -shared --offload-arch=gfx950 tools/cvt_probe.hip -o tools/libcvt_probe.so
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace {
constexpr int ITERS = 2000, PER_ITER = 16;  // 32 000 measured instructions per wave
constexpr int MFMAS = 24000;                // the partner wave: 24 000 x 32 cycles, longer than 32 000 instructions at 16 cycles each

typedef int v8i __attribute__((ext_vector_type(8)));
typedef float v16f __attribute__((ext_vector_type(16)));

#define AB(i) "v_alignbit_b32 %0, %0, %" #i ", 31\n\t"
#define CV(d, a, b, sel) "v_cvt_scalef32_pk_fp4_f32 %" #d ", %" #a ", %" #b ", 1.0" sel "\n\t"

template <int STREAM>
__global__ __launch_bounds__(512) void k_cvt_probe(uint32_t *out, unsigned long long *stamps, int with_mfma) {
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (wave >= 4) {  // the partner: MFMAs back to back (two accumulators, so no MFMA waits for the one before)
    if (!with_mfma) return;
    const v8i a = {0x22222222, 0x2A2A2A2A, (int)threadIdx.x, 0x22222222, 0, 0, 0, 0};
    v16f acc0 = {0}, acc1 = {0};
    const unsigned long long c0 = __builtin_amdgcn_s_memtime();
    for (int i = 0; i < MFMAS / 2; i++) {
      acc0 = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, a, acc0, 4, 4, 0, 0x7F7F7F7F, 0, 0x7F7F7F7F);
      acc1 = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, a, acc1, 4, 4, 0, 0x7F7F7F7F, 0, 0x7F7F7F7F);
    }
    const unsigned long long c1 = __builtin_amdgcn_s_memtime();
    out[blockIdx.x * 512 + threadIdx.x] = (uint32_t)(acc0[0] + acc1[5]);
    if (threadIdx.x == 256) stamps[blockIdx.x * 3 + 2] = c1 - c0;
    return;
  }
  float f[16];
  for (int i = 0; i < 16; i++) f[i] = (float)((int)(threadIdx.x * 7 + i * 13) % 19 - 9);
  uint32_t x = threadIdx.x, d0 = 0, d1 = 0;
  const unsigned long long c0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
  for (int it = 0; it < ITERS; it++) {
    if constexpr (STREAM == 0)
      asm volatile(AB(1) AB(2) AB(3) AB(4) AB(5) AB(6) AB(7) AB(8) AB(9) AB(10) AB(11) AB(12) AB(13) AB(14) AB(15) AB(16)
                   : "+v"(x)
                   : "v"(f[0]), "v"(f[1]), "v"(f[2]), "v"(f[3]), "v"(f[4]), "v"(f[5]), "v"(f[6]), "v"(f[7]), "v"(f[8]), "v"(f[9]), "v"(f[10]), "v"(f[11]),
                     "v"(f[12]), "v"(f[13]), "v"(f[14]), "v"(f[15]));
    else  // two collections of eight conversions, the two destinations alternating as the compiler emits them
      asm volatile(CV(0, 2, 3, "") CV(1, 10, 11, "") CV(0, 4, 5, " op_sel:[0,0,1,0]") CV(1, 12, 13, " op_sel:[0,0,1,0]")
                       CV(0, 6, 7, " op_sel:[0,0,0,1]") CV(1, 14, 15, " op_sel:[0,0,0,1]") CV(0, 8, 9, " op_sel:[0,0,1,1]")
                           CV(1, 16, 17, " op_sel:[0,0,1,1]") CV(0, 2, 3, "") CV(1, 10, 11, "") CV(0, 4, 5, " op_sel:[0,0,1,0]")
                               CV(1, 12, 13, " op_sel:[0,0,1,0]") CV(0, 6, 7, " op_sel:[0,0,0,1]") CV(1, 14, 15, " op_sel:[0,0,0,1]")
                                   CV(0, 8, 9, " op_sel:[0,0,1,1]") CV(1, 16, 17, " op_sel:[0,0,1,1]")
                   : "+v"(d0), "+v"(d1)
                   : "v"(f[0]), "v"(f[1]), "v"(f[2]), "v"(f[3]), "v"(f[4]), "v"(f[5]), "v"(f[6]), "v"(f[7]), "v"(f[8]), "v"(f[9]), "v"(f[10]), "v"(f[11]),
                     "v"(f[12]), "v"(f[13]), "v"(f[14]), "v"(f[15]));
  }
  const unsigned long long c1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
  out[blockIdx.x * 512 + threadIdx.x] = x + d0 + d1;
  if (threadIdx.x == 0) {
    stamps[blockIdx.x * 3] = c1 - c0;
    stamps[blockIdx.x * 3 + 1] = r1 - r0;
  }
}

__global__ void k_cvt_values(const float *in, uint32_t *out, int pairs) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= pairs) return;
  uint32_t d = 0;
  d = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(d, in[2 * i], in[2 * i + 1], 1.0f, 1);  // byte 1: bits 8..11 first source, 12..15 second
  out[i] = d;
}
}  // namespace

// stream 0 / 1 as above; with_mfma 0 / 1.  Out: SIMD-cycles per instruction (the median block's wave 0), the clock it
// ran at (MHz), and with the partner the cycles per MFMA of the median partner wave (32 when it is not held up).
// Returns 0, or -1 on a HIP error.
extern "C" int cvt_probe_run(int stream, int with_mfma, double *cycles_per_inst, double *clock_mhz, double *cycles_per_mfma) {
  if (stream < 0 || stream > 1) return -1;
  int dev = 0;
  hipDeviceProp_t prop;
  if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) return -1;
  const int blocks = prop.multiProcessorCount, threads = with_mfma ? 512 : 256;
  uint32_t *out = nullptr;
  unsigned long long *st = nullptr;
  int rc = -1;
  std::vector<unsigned long long> h((size_t)blocks * 3);
  if (hipMalloc(&out, (size_t)blocks * 512 * 4) != hipSuccess || hipMalloc(&st, (size_t)blocks * 24) != hipSuccess) goto done;
  if (hipMemset(st, 0, (size_t)blocks * 24) != hipSuccess) goto done;
  for (int rep = 0; rep < 3; rep++) {  // the last of three launches is read (the first ones settle the clock)
    if (stream == 0) hipLaunchKernelGGL(k_cvt_probe<0>, dim3(blocks), dim3(threads), 0, nullptr, out, st, with_mfma);
    else hipLaunchKernelGGL(k_cvt_probe<1>, dim3(blocks), dim3(threads), 0, nullptr, out, st, with_mfma);
    if (hipDeviceSynchronize() != hipSuccess) goto done;
  }
  if (hipMemcpy(h.data(), st, (size_t)blocks * 24, hipMemcpyDeviceToHost) != hipSuccess) goto done;
  {
    std::vector<double> cyc, mhz, mf;
    for (int b = 0; b < blocks; b++) {
      cyc.push_back((double)h[3 * b]);
      mhz.push_back(100.0 * (double)h[3 * b] / (double)h[3 * b + 1]);
      mf.push_back((double)h[3 * b + 2]);
    }
    std::sort(cyc.begin(), cyc.end());
    std::sort(mhz.begin(), mhz.end());
    std::sort(mf.begin(), mf.end());
    *cycles_per_inst = cyc[blocks / 2] / ((double)ITERS * PER_ITER);
    *clock_mhz = mhz[blocks / 2];
    *cycles_per_mfma = with_mfma ? mf[blocks / 2] / MFMAS : 0.0;
    rc = 0;
  }
done:
  if (out) (void)hipFree(out);
  if (st) (void)hipFree(st);
  return rc;
}

// converts `pairs` pairs of floats; out[i]: bits 8..11 = FP4 of in[2i], bits 12..15 = FP4 of in[2i + 1], other bits 0
extern "C" int cvt_probe_values(const float *in, uint32_t *out, int pairs) {
  float *din = nullptr;
  uint32_t *dout = nullptr;
  int rc = -1;
  if (hipMalloc(&din, (size_t)pairs * 8) != hipSuccess || hipMalloc(&dout, (size_t)pairs * 4) != hipSuccess) goto done;
  if (hipMemcpy(din, in, (size_t)pairs * 8, hipMemcpyHostToDevice) != hipSuccess) goto done;
  hipLaunchKernelGGL(k_cvt_values, dim3((pairs + 63) / 64), dim3(64), 0, nullptr, din, dout, pairs);
  if (hipMemcpy(out, dout, (size_t)pairs * 4, hipMemcpyDeviceToHost) != hipSuccess) goto done;
  rc = 0;
done:
  if (din) (void)hipFree(din);
  if (dout) (void)hipFree(dout);
  return rc;
}
