"""The pixel formats' model (csrc/pixfmt.h, DESIGN.md 9 "Camera frames") restated in plain numpy: where the planes of a
frame lie, how chroma is replicated, and the two colour statements.  Written from the header's words, not from its code:
the tables of range 0 are the floating-point statement, `(int)(c * 64 * (i - 128) + 0.5)` with C truncation."""
import numpy as np

FORMATS = {"rgb": 0, "l": 1, "bgr": 2, "nv12": 3, "i420": 4, "yuyv": 5}
COEFFS = (1.402, -0.34414, -0.71414, 1.772)


def tables():
    """T_c[i] for the four coefficients, int64 [4, 256]"""
    i = np.arange(256, dtype=np.float64)
    return np.stack([np.trunc(c * 64 * (i - 128) + 0.5).astype(np.int64) for c in COEFFS])


def yuv_to_rgb(y, cb, cr, video_range=0, clip=True):
    """int arrays of one shape -> [..., 3]; with clip=False the values before clip8"""
    y, cb, cr = (np.asarray(a).astype(np.int64) for a in (y, cb, cr))
    if not video_range:
        t = tables()
        rgb = np.stack([y + (t[0][cr] >> 6), y + ((t[1][cb] + t[2][cr]) >> 6), y + (t[3][cb] >> 6)], axis=-1)
    else:
        c, d, e = y - 16, cb - 128, cr - 128
        rgb = np.stack([(298 * c + 409 * e + 128) >> 8, (298 * c - 100 * d - 208 * e + 128) >> 8, (298 * c + 516 * d + 128) >> 8], axis=-1)
    return np.clip(rgb, 0, 255).astype(np.uint8) if clip else rgb


def row_bytes(fmt, w):
    return w * {"rgb": 3, "bgr": 3, "l": 1, "nv12": 1, "i420": 1, "yuyv": 2}[fmt]


def geometry(fmt, w, h, frames, row_stride=0, frame_stride=0):
    """(row stride, rows of a frame counted in strides, frame stride, bytes from the first frame to past the last)"""
    s = row_stride or row_bytes(fmt, w)
    rows = h * 3 // 2 if fmt in ("nv12", "i420") else h
    fs = frame_stride or s * rows
    return s, rows, fs, fs * (frames - 1) + s * rows


def planes(buf, fmt, w, h, frames, row_stride=0, frame_stride=0):
    """the planes of every frame as a list of [F, rows, cols] arrays: what the format stores, without any padding"""
    s, _, fs, total = geometry(fmt, w, h, frames, row_stride, frame_stride)
    buf = np.asarray(buf, np.uint8).ravel()
    assert len(buf) >= total

    def plane(off, rows, cols, stride):
        idx = (np.arange(frames)[:, None, None] * fs + off + np.arange(rows)[None, :, None] * stride + np.arange(cols)[None, None, :])
        return buf[idx]

    if fmt == "nv12":
        return [plane(0, h, w, s), plane(h * s, h // 2, w, s)]
    if fmt == "i420":
        return [plane(0, h, w, s), plane(h * s, h // 2, w // 2, s // 2), plane(h * s + (h // 2) * (s // 2), h // 2, w // 2, s // 2)]
    return [plane(0, h, row_bytes(fmt, w), s)]


def packed(buf, fmt, w, h, frames, row_stride=0, frame_stride=0):
    """the same frames with row_stride = frame_stride = 0"""
    return np.concatenate([p.reshape(frames, -1) for p in planes(buf, fmt, w, h, frames, row_stride, frame_stride)], axis=1).ravel()


def unpack(buf, fmt, w, h, frames, row_stride=0, frame_stride=0, video_range=0):
    """packed RGB uint8 [F, h, w, 3]"""
    p = planes(buf, fmt, w, h, frames, row_stride, frame_stride)
    if fmt in ("rgb", "bgr"):
        a = p[0].reshape(frames, h, w, 3)
        return np.ascontiguousarray(a[..., ::-1] if fmt == "bgr" else a)
    if fmt == "l":
        return np.ascontiguousarray(np.repeat(p[0][..., None], 3, axis=-1))
    if fmt == "yuyv":
        y, cb, cr = p[0][:, :, 0::2], p[0][:, :, 1::4], p[0][:, :, 3::4]
        cb, cr = np.repeat(cb, 2, axis=2), np.repeat(cr, 2, axis=2)
    else:
        y = p[0]
        cb, cr = (p[1][:, :, 0::2], p[1][:, :, 1::2]) if fmt == "nv12" else (p[1], p[2])
        cb, cr = (np.repeat(np.repeat(c, 2, axis=1), 2, axis=2) for c in (cb, cr))
    return yuv_to_rgb(y, cb, cr, video_range)
