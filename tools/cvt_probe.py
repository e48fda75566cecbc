#!/usr/bin/env python3
"""tools/cvt_probe.py: SIMD-cycles per instruction of the two sign collections of the matrix-form conv kernels
(tools/cvt_probe.hip) -- a dependent v_alignbit_b32 chain against the eight read-modify-write
v_cvt_scalef32_pk_fp4_f32 of a packed collection (built and not kept, CHANGELOG), each alone on the SIMD and beside a wave that issues MFMAs back to back -- the
cost of a whole 16-sign collection in either form (16 + 4 against 8 + 4 instructions, the 4 priced as v_alignbit_b32),
and the FP4 nibbles of the conversion's edge values.  Builds the library if it is missing or older than its source."""
import ctypes as C
import os
import struct
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
LIB, SRC = os.path.join(HERE, "libcvt_probe.so"), os.path.join(HERE, "cvt_probe.hip")
if not os.path.exists(LIB) or os.path.getmtime(LIB) < os.path.getmtime(SRC):
    subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "-shared", "--offload-arch=gfx950", SRC, "-o", LIB], check=True)
L = C.CDLL(LIB)
L.cvt_probe_run.argtypes = [C.c_int, C.c_int] + [C.POINTER(C.c_double)] * 3
L.cvt_probe_values.argtypes = [C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.c_int]


def f32(bits):
    return struct.unpack("<f", struct.pack("<I", bits))[0]


cost = {}
for with_mfma in (0, 1):
    for stream, name in ((0, "v_alignbit_b32 (dependent chain)"), (1, "v_cvt_scalef32_pk_fp4_f32 (8 rmw, 2 destinations)")):
        runs = []
        for _ in range(3):
            cyc, mhz, mf = C.c_double(), C.c_double(), C.c_double()
            assert L.cvt_probe_run(stream, with_mfma, C.byref(cyc), C.byref(mhz), C.byref(mf)) == 0
            runs.append((cyc.value, mhz.value, mf.value))
        runs.sort()
        cyc, mhz, mf = runs[1]
        cost[stream, with_mfma] = cyc
        print("%-52s %s: %.2f SIMD-cycles per instruction (3 runs %.2f..%.2f), %.0f MHz%s" % (
            name, "beside MFMAs" if with_mfma else "alone       ", cyc, runs[0][0], runs[2][0], mhz,
            ", partner %.1f cycles per MFMA" % mf if with_mfma else ""), flush=True)
for with_mfma in (0, 1):
    a, c = cost[0, with_mfma], cost[1, with_mfma]
    print("16 signs %s: sign_nibbles 20 x %.2f = %.0f cycles, packed 8 x %.2f + 4 x %.2f = %.0f cycles" % (
        "beside MFMAs" if with_mfma else "alone", a, 20 * a, c, a, 8 * c + 4 * a))

# edge values: (first source, second source) -> nibbles; the sign must sit in bit 3 of each nibble
vals = [(0x00000000, 0x80000000), (0xBF800000, 0x3F800000), (0xC5102000, 0x45102000), (0x80400000, 0x00400000),
        (0x80000001, 0x00000001), (0xBE800000, 0x3E800000), (0xC0C00000, 0x40C00000), (0xC0E00000, 0x40E00000), (0xBF000000, 0x3F000000),
        (0x80800000, 0x00800000)]
n = len(vals)
fin = (C.c_float * (2 * n))(*[f32(b) for p in vals for b in p])
out = (C.c_uint32 * n)()
assert L.cvt_probe_values(fin, out, n) == 0
ok = True
for (a, b), d in zip(vals, out):
    lo, hi = (d >> 8) & 15, (d >> 12) & 15
    good = (d & ~0xFF00) == 0 and (lo >> 3) == (a >> 31) and (hi >> 3) == (b >> 31)
    ok &= good
    print("cvt(%#010x = %g, %#010x = %g) into byte 1 -> %#010x: first source nibble %#x, second %#x  %s" % (
        a, f32(a), b, f32(b), d, lo, hi, "sign kept" if good else "SIGN LOST"))
print("edge values:", "every sign kept, first source in the low nibble" if ok else "FAILED")
