"""CPU: the tables of the clip scan's matrix-core stage 0 (clip_l0_tables, host only), printed by a stand-alone program built
here under ASan + UBSan and run directly: the bands tile every stage-0 map exactly once, every block names a map that holds
its band, and every staging load the kernel can issue lies inside the planes up to the stated highest byte, at most 7 bytes
behind them.  The shapes are those of tests/test_gpu_scan_l0_matrix.py, and one clip at the capacity limit."""
import os
import subprocess

import numpy as np
import pytest

import gpu_lib as gl
import scan_clip_ref as ref

CSRC = os.path.join(gl.ROOT, "bnn-pynq_amd", "csrc")
SHAPES = ([(w, 37, 2, (32,)) for w in (44, 45, 46, 47)] + [(w, 36, 1, (32,)) for w in (36, 64, 68)] +
          [(200, 52, 1, (32,)), (164, 50, 1, (32,)), (90, 74, 3, (32, 64)), (100, 52, 1, (32,)), (100, 52, 3, (32, 40)), (640, 480, 0, (64, 96))])


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("scan_l0") / "tables")
    srcs = [os.path.join(gl.ROOT, "tests", "host_scan_l0", "main.cpp"), os.path.join(CSRC, "scan_clip.cpp"), os.path.join(CSRC, "scan.cpp")]
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, "-o", path] + srcs,
                   check=True)
    return path


@pytest.mark.parametrize("width,height,frames,sizes", SHAPES)  # (frames 0: the clip's capacity)
def test_bands_tile_every_map_and_loads_stay_inside(exe, width, height, frames, sizes):
    out = subprocess.run([exe, str(width), str(height), str(frames)] + [str(s) for s in sizes], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    rows = [l.split() for l in out.stdout.splitlines()]
    (band_rows, band_cols), (n_frames, planes_bytes, planes_top, blocks) = [[int(v) for v in r[1:]] for r in rows[:2]]
    assert n_frames == (frames or ref.capacity(width, height, sizes)) >= 1
    maps = [[int(v) for v in r[1:]] for r in rows if r[0] == "map"]
    bands = [[int(v) for v in r[1:]] for r in rows if r[0] == "band"]
    lay, lv = ref.layout(width, height, sizes, n_frames), ref.levels(width, height, sizes)
    level_bytes = [3 * w * h * n_frames for _, (w, h), _ in lv]
    assert len(maps) == len(lay["maps"]) and [b[0] for b in bands] == list(range(blocks)) and planes_bytes == sum(level_bytes)
    covered, highest = [np.zeros((m[6], m[5]), np.uint8) for m in maps], 0
    for block, m, y0, x0 in bands:
        _, in_off, out_off, plane_stride, row_stride, ow, oh, first_block, level_w, level_h = maps[m]
        assert 0 <= y0 < oh and 0 <= x0 < ow and y0 % band_rows == 0 and x0 % band_cols == 0 and block >= first_block
        nrows, cols = min(band_rows, oh - y0), min(band_cols, ow - x0)
        covered[m][y0:y0 + nrows, x0:x0 + cols] += 1
        for plane in range(3):
            for row in range(nrows + 2):
                # cols + 2 bytes from `start`: loaded as the aligned dwords from `start` & ~3 to one past ceil((cols + 2) / 4) of them
                start = in_off + plane * plane_stride + (y0 + row) * row_stride + x0
                assert in_off + plane * plane_stride <= start and start + cols + 2 <= in_off + (plane + 1) * plane_stride
                top = (start & ~3) + 4 * ((cols + 2 + 3) // 4) + 4
                assert start + cols + 2 <= top <= planes_top
                highest = max(highest, top)
    assert highest == planes_top <= planes_bytes + 7  # (below planes_bytes where the scan leaves the level's last rows unused)
    for i, (m, in_off, out_off, plane_stride, row_stride, ow, oh, first_block, level_w, level_h) in enumerate(maps):
        f, size, (nx, ny), _, offs = lay["maps"][i]
        k = [s for s, _, _ in lv].index(size)
        assert (covered[i] == 1).all() and (level_w, level_h) == lv[k][1] and (ow, oh) == ref.stage_sizes(nx, ny)[0]
        assert (row_stride, plane_stride) == (level_w, level_w * level_h) and ow + 2 <= level_w and oh + 2 <= level_h
        assert in_off == sum(level_bytes[:k]) + 3 * level_w * level_h * f and out_off == offs[0]
        assert first_block == next(b[0] for b in bands if b[1] == i)
