"""GPU: the pixel formats' kernel (bnn_mi355x_unpack_frames; csrc/pixfmt_kernels.hip, DESIGN.md 9 "Camera frames").

Everything is exact: the kernel must equal the host model (bnn_mi355x_unpack_frames_host, which tests/test_pixfmt_host.py
pins to Pillow and to tests/pixfmt_ref.py) byte for byte.  The uploaded frames keep their row stride, so the strides below
choose the kernel's path: 8- and 16-byte accesses where base and strides allow them, bytes elsewhere and in row tails.
The output lies between canaries on the host, and between guards on the device that the entry point checks itself."""
import numpy as np
import pytest

import pixfmt_cases as pc
import pixfmt_ref as ref

pytestmark = pytest.mark.gpu

FORMATS = sorted(ref.FORMATS)


@pytest.fixture(scope="module")
def lib():
    return pc.gl.load("cnvW1A1")  # (no parameters are needed)


def same_as_host(lib, buf, fr, what):
    want = pc.unpack(lib, pc.HOST, buf, fr)
    got = pc.unpack(lib, pc.DEVICE, buf, fr)
    assert got.tobytes() == want.tobytes(), (what, int((got != want).any(axis=-1).sum()))
    return got


@pytest.mark.parametrize("video_range", [0, 1])
def test_every_triple_in_one_launch(lib, video_range):
    buf = pc.exhaustive_nv12()[0]
    same_as_host(lib, buf, pc.struct("nv12", 4096, 4096, 1, video_range=video_range), "exhaustive")


@pytest.mark.parametrize("strides", ["packed", "padded", "wide"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_every_format_equals_the_host_model(lib, fmt, strides):
    """widths 2, 6, 34, 66 and 2050 (more than one block of 256 lanes a row pair), heights 2 and 6, 3 frames; packed, padded
    (odd strides where the format allows them: the byte path) and 16-byte strides (the wide path, with a byte tail)"""
    for w in (2, 6, 34, 66, 2050):
        for h in (2, 6):
            s, fs = {"packed": lambda *a: (0, 0), "padded": pc.padded_strides, "wide": pc.wide_strides}[strides](fmt, w, h)
            buf = pc.random_frames(fmt, w, h, 3, s, fs)
            for video_range in ((0, 1) if fmt in ("nv12", "i420", "yuyv") else (0,)):
                same_as_host(lib, buf, pc.struct(fmt, w, h, 3, s, fs, video_range), (fmt, strides, w, h, video_range))


def test_whole_units_on_the_wide_path(lib):
    """widths that are multiples of 8 and 16, packed: no byte tail, every lane of more than one block on the wide path"""
    for fmt in FORMATS:
        for w, h in ((16, 2), (2064, 6)):
            buf = pc.random_frames(fmt, w, h, 2, seed=1)
            same_as_host(lib, buf, pc.struct(fmt, w, h, 2, video_range=1), (fmt, w, h))


def test_odd_strides_take_the_byte_path(lib):
    for fmt, per in (("yuyv", 2), ("bgr", 3)):
        for w in (34, 2050):
            s = per * w + 1
            buf = pc.random_frames(fmt, w, 6, 3, s, 0, seed=2)
            same_as_host(lib, buf, pc.struct(fmt, w, 6, 3, s, 0), (fmt, w, s))


def test_device_time_and_refusals(lib):
    import ctypes as C
    fr = pc.struct("nv12", 66, 6, 3)
    buf = pc.random_frames("nv12", 66, 6, 3)
    out = np.zeros((3, 6, 66, 3), np.uint8)
    usec = C.c_float(-1)
    assert lib.bnn_mi355x_unpack_frames(C.byref(fr), buf.ctypes.data, out.ctypes.data, C.byref(usec)) == 0
    assert usec.value > 0
    rc, msg = pc.unpack(lib, pc.DEVICE, buf, pc.struct("nv12", 65, 6, 3), raw=True)
    assert rc == -1 and msg.startswith("unpack_frames: ") and "width" in msg
    rc, msg = pc.unpack(pc.gl.load("lfcW1A1"), pc.DEVICE, buf, fr, raw=True)
    assert rc == -1 and "CNV networks only" in msg


def test_another_cnv_library_unpacks_without_parameters():
    L = pc.gl.load("cnvW2A2")
    buf = pc.random_frames("i420", 66, 6, 3, 72, 0, seed=3)
    same_as_host(L, buf, pc.struct("i420", 66, 6, 3, 72, 0), "cnvW2A2")
