"""The clip scan's host rules (csrc/scan_clip.h) in plain Python on top of scan_ref.py: the order of the maps, `first`,
where every map of every stage lies, the work items and blocks of the merged launches, the limits and the capacity.
Stated independently of the C code."""
import scan_ref

MAX_FRAMES = 4096
MAX_CLIP_BYTES = 1 << 30
BLOCK = 256


def levels(width, height, sizes):
    """[(size, (level_w, level_h), (nx, ny))] of one frame, or None when scan_scene would refuse it"""
    if not sizes or width < 32 or height < 32 or width > scan_ref.MAX_SIDE or height > scan_ref.MAX_SIDE:
        return None
    out = []
    for s in sizes:
        lv = scan_ref.level(width, height, s)
        if lv is None or not scan_ref.acceptable(*lv):
            return None
        out.append((s, lv, scan_ref.grid(*lv)))
    return out


def stage_sizes(nx, ny):
    """[(map_w, map_h)] of the six stages"""
    return list(zip(scan_ref.map_sizes(nx), scan_ref.map_sizes(ny)))


def stage_bytes(nx, ny):
    return [w * h * scan_ref.STAGE_DWORDS[s] * 4 for s, (w, h) in enumerate(stage_sizes(nx, ny))]


def items(nx, ny):
    """work items per stage: output pixels (stages 0, 4, 5), 2 x 2 quads of conv outputs (stages 1-3)"""
    sz = stage_sizes(nx, ny)
    return [sz[0][0] * sz[0][1], sz[1][0] * sz[1][1], (sz[2][0] // 2) * (sz[2][1] // 2), sz[3][0] * sz[3][1], sz[4][0] * sz[4][1],
            sz[5][0] * sz[5][1]]


def blocks(nx, ny):
    return [(n + BLOCK - 1) // BLOCK for n in items(nx, ny)]


def layout(width, height, sizes, frames):
    """dict of the clip's layout, or None when refused: maps [(frame, size, (nx, ny), first, [off per stage])] in map
    order m = f * len(sizes) + k, windows, stage totals, blocks per stage, the two buffer sizes"""
    lv = levels(width, height, sizes)
    if lv is None or frames < 1 or frames > MAX_FRAMES:
        return None
    maps, first, total, nblocks = [], 0, [0] * 6, [0] * 6
    for f in range(frames):
        for s, _, (nx, ny) in lv:
            maps.append((f, s, (nx, ny), first, list(total)))
            first += nx * ny
            total = [a + b for a, b in zip(total, stage_bytes(nx, ny))]
            nblocks = [a + b for a, b in zip(nblocks, blocks(nx, ny))]
    buf0 = max(total[0], total[2], total[4], first * 64)
    buf1 = max(total[1], total[3], total[5], first * 64)
    return {"maps": maps, "windows": first, "stage_bytes": total, "blocks": nblocks, "buf": (buf0, buf1)}


def acceptable(width, height, sizes, frames, bands=3):
    lay = layout(width, height, sizes, frames)
    return (lay is not None and lay["windows"] <= scan_ref.MAX_WINDOWS and max(lay["buf"]) <= scan_ref.MAX_MAP_BYTES and
            frames * width * height * bands <= MAX_CLIP_BYTES)


def capacity(width, height, sizes):
    """the largest accepted number of RGB frames; 0 when one frame is refused.  By search, not by division: accepted(F)
    is monotone in F."""
    if not acceptable(width, height, sizes, 1):
        return 0
    lo, hi = 1, MAX_FRAMES + 1  # accepted(lo), not accepted(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if acceptable(width, height, sizes, mid):
            lo = mid
        else:
            hi = mid
    return lo
