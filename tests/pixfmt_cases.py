"""Inputs of the pixel formats' tests (tests/test_pixfmt_host.py, tests/test_gpu_pixfmt.py, tests/test_gpu_clip_frames.py) and
the calls into bnn_mi355x_unpack_frames_host / bnn_mi355x_unpack_frames.  Every buffer is seeded random, padding included."""
import ctypes as C
import functools

import numpy as np

import gpu_lib as gl
import pixfmt_ref as ref

abi = gl.abi
HOST, DEVICE = "bnn_mi355x_unpack_frames_host", "bnn_mi355x_unpack_frames"
CANARY = 64


def struct(fmt, w, h, frames, row_stride=0, frame_stride=0, video_range=0):
    return abi.Frames(fmt if isinstance(fmt, int) else ref.FORMATS[fmt], video_range, w, h, frames, row_stride, frame_stride)


def random_frames(fmt, w, h, frames, row_stride=0, frame_stride=0, seed=0):
    """exactly the bytes from the first frame to past the last, padding included"""
    total = ref.geometry(fmt, w, h, frames, row_stride, frame_stride)[3]
    return np.random.default_rng([ref.FORMATS[fmt], w, h, frames, row_stride, frame_stride, seed]).integers(0, 256, total, dtype=np.uint8)


def padded_strides(fmt, w, h):
    """a row stride wider than the row -- odd where the format allows it (YUYV, BGR; RGB and L too), even otherwise -- and a
    frame stride with a gap of 7 bytes"""
    rb = ref.row_bytes(fmt, w)
    s = rb + 6 if fmt in ("nv12", "i420") else rb + 5 + (rb % 2)
    assert s % 2 == (0 if fmt in ("nv12", "i420") else 1)
    return s, s * ref.geometry(fmt, w, h, 1, s)[1] + 7


def wide_strides(fmt, w, h):
    """row and frame strides that are multiples of 16, wider than the row: the kernel's wide path"""
    s = (ref.row_bytes(fmt, w) + 15) // 16 * 16 + 16
    return s, s * ref.geometry(fmt, w, h, 1, s)[1] + 32


def unpack(lib, symbol, buf, fr, raw=False):
    """packed RGB [F, h, w, 3] of `symbol`; the output lies between two canaries of 64 bytes, which must survive.  With
    `raw` the return code and the message instead of an assertion."""
    n = fr.n_frames * fr.height * fr.width * 3 if min(fr.n_frames, fr.height, fr.width) > 0 else 0
    out = np.full(n + 2 * CANARY, 0x5A, np.uint8)
    args = [C.byref(fr), buf.ctypes.data if buf is not None else None, out.ctypes.data + CANARY]
    if symbol == DEVICE:
        args.append(None)
    rc = getattr(lib, symbol)(*args)
    if raw:
        return rc, lib.bnn_mi355x_last_error().decode()
    assert rc == 0, lib.bnn_mi355x_last_error().decode()
    assert (out[:CANARY] == 0x5A).all() and (out[CANARY + n:] == 0x5A).all(), "canary"
    return out[CANARY:CANARY + n].reshape(fr.n_frames, fr.height, fr.width, 3)


@functools.lru_cache(maxsize=None)
def exhaustive_nv12():
    """one NV12 frame of 4096 x 4096 whose 2 x 2 blocks run through all 65 536 (Cb, Cr) pairs, each with all 256 Y values (64
    blocks of 4): -> (the frame's bytes, Y, Cb, Cr replicated to [4096, 4096])"""
    block = np.arange(2048 * 2048).reshape(2048, 2048)
    pair, k = block // 64, block % 64
    y = np.empty((4096, 4096), np.uint8)
    for dy in (0, 1):
        for dx in (0, 1):
            y[dy::2, dx::2] = 4 * k + 2 * dy + dx
    uv = np.empty((2048, 4096), np.uint8)
    uv[:, 0::2], uv[:, 1::2] = pair >> 8, pair & 255
    up = lambda c: np.repeat(np.repeat(c, 2, axis=0), 2, axis=1)  # noqa: E731
    buf = np.concatenate([y.ravel(), uv.ravel()])
    triples = np.stack([y, up(uv[:, 0::2]), up(uv[:, 1::2])], axis=-1).reshape(-1, 3).astype(np.uint32)
    assert len(np.unique(triples[:, 0] << 16 | triples[:, 1] << 8 | triples[:, 2])) == 1 << 24
    return buf, y, up(uv[:, 0::2]), up(uv[:, 1::2])
