"""The dense scan's host rules (csrc/scan.h) in plain Python: the grid, the six map sizes, the level and box rule of a
multi-level call, and the records the per-window pass would be given.  The level / box rule is this project's own (the
reference tiles with Image.crop alone); it is stated once in scan.h and restated here, independently of the C code."""
import numpy as np

MAX_SIDE = 8192
MAX_WINDOWS = 1 << 20
MAX_MAP_BYTES = 1 << 27
STAGE_DWORDS = (2, 2, 4, 4, 8, 8)
# what a window's cell (i, j) of the scan's map of stage s starts at: (scale * i, scale * j)
STAGE_SCALE = (4, 2, 2, 1, 1, 1)
# the side of a 32 x 32 record's map of stage s
STAGE_SIDE = (30, 14, 12, 5, 3, 1)


def grid(width, height):
    """(nx, ny), or None for a side below 32"""
    if width < 32 or height < 32:
        return None
    return (width - 32) // 4 + 1, (height - 32) // 4 + 1


def map_sizes(n):
    """the six map sizes along an axis with n windows"""
    u = 32 + 4 * (n - 1)
    p1 = (u - 4) // 2
    p2 = (p1 - 4) // 2
    return (u - 2, p1, p1 - 2, p2, p2 - 2, p2 - 4)


def map_bytes(width, height):
    """bytes of the two activation buffers of one picture (even stages and layer 6 in the first, odd ones and layer 7 in
    the second)"""
    nx, ny = grid(width, height)
    w, h = map_sizes(nx), map_sizes(ny)
    stage = [w[s] * h[s] * STAGE_DWORDS[s] * 4 for s in range(6)]
    tail = nx * ny * 64
    return max(stage[0], stage[2], stage[4], tail) + max(stage[1], stage[3], stage[5], tail)


def acceptable(width, height):
    g = grid(width, height)
    return (g is not None and width <= MAX_SIDE and height <= MAX_SIDE and g[0] * g[1] <= MAX_WINDOWS and
            map_bytes(width, height) <= MAX_MAP_BYTES)


def level(width, height, size):
    """(level_w, level_h) of window size `size`, or None when refused"""
    if size < 8 or size % 8:
        return None
    lw, lh = width * 32 // size, height * 32 // size
    if lw < 32 or lh < 32:
        return None
    return lw, lh


def boxes(width, height, size):
    """the boxes of one level, raster order (rows outer), or None when refused"""
    lv = level(width, height, size)
    if lv is None or width > MAX_SIDE or height > MAX_SIDE or not acceptable(*lv):
        return None
    nx, ny = grid(*lv)
    step = size // 8
    return [(i * step, j * step, i * step + size, j * step + size) for j in range(ny) for i in range(nx)]


def cut_records(planes):
    """planar uint8 [3, H, W] -> the nx * ny record bodies [n, 3072] the per-window pass is given, raster order"""
    _, h, w = planes.shape
    nx, ny = grid(w, h)
    return np.stack([planes[:, 4 * j:4 * j + 32, 4 * i:4 * i + 32].reshape(3072) for j in range(ny) for i in range(nx)])
