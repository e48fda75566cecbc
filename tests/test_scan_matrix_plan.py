"""CPU: the band tables of the clip scan's matrix form (clip_mfma_tables, host only), printed by a stand-alone program built
here under ASan + UBSan: every block names a band inside its map, the bands of a map tile its conv outputs exactly once,
and the input patch of every block, the last of every map included, lies inside the map's input bytes."""
import os
import subprocess

import pytest

import gpu_lib as gl
import scan_clip_ref as ref

CSRC, IN_DWORDS = os.path.join(gl.ROOT, "bnn-pynq_amd", "csrc"), {1: 2, 2: 2, 3: 4}  # (dwords per pixel of the stage's input map)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("scan_matrix") / "tables")
    srcs = [os.path.join(gl.ROOT, "tests", "host_scan_matrix", "main.cpp"), os.path.join(CSRC, "scan_clip.cpp"), os.path.join(CSRC, "scan.cpp")]
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, "-o", path] + srcs,
                   check=True)
    return path


@pytest.mark.parametrize("width,height,frames,sizes", [(w, h, 1, (32,)) for w in (32, 36, 40, 72, 76, 100, 140) for h in (32, 36, 40, 44, 48)] +
                         [(100, 52, 3, (32, 40)), (640, 480, 2, (64, 96))])
def test_bands_tile_every_map(exe, width, height, frames, sizes):
    out = subprocess.run([exe, str(width), str(height), str(frames)] + [str(s) for s in sizes], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    rows = [l.split() for l in out.stdout.splitlines()]
    rp_band, chunk = (int(v) for v in rows[0][1:])
    lay = ref.layout(width, height, sizes, frames)
    for stage in (1, 2, 3):
        maps = [[int(v) for v in r[2:]] for r in rows if r[0] == "map" and int(r[1]) == stage]
        bands = [[int(v) for v in r[2:]] for r in rows if r[0] == "band" and int(r[1]) == stage]
        assert len(maps) == len(lay["maps"]) and [b[0] for b in bands] == list(range(len(bands)))
        covered = [set() for _ in maps]
        for block, m, rp0, x0 in bands:
            _, in_off, out_off, iw, ow, row_pairs, first_block, in_bytes, out_w, out_h = maps[m]
            assert 0 <= rp0 < row_pairs and 0 <= x0 < ow and rp0 % rp_band == 0 and x0 % chunk == 0 and block >= first_block
            nrp, cols = min(rp_band, row_pairs - rp0), min(chunk, ow - x0)
            cells = {(rp, x) for rp in range(rp0, rp0 + nrp) for x in range(x0, x0 + cols)}
            assert not (cells & covered[m]), "a conv output in two bands"
            covered[m] |= cells
            # the patch's last pixel: row 2 rp0 + 2 nrp + 1, column x0 + cols + 1 of the input map
            assert ((2 * rp0 + 2 * nrp + 1) * iw + x0 + cols + 2) * IN_DWORDS[stage] * 4 <= in_bytes and x0 + cols + 2 <= iw
        for m, (_, in_off, out_off, iw, ow, row_pairs, first_block, in_bytes, out_w, out_h) in enumerate(maps):
            assert len(covered[m]) == ow * row_pairs and ow == iw - 2 and (out_w, out_h) == ((ow, 2 * row_pairs) if stage == 2 else (ow // 2, row_pairs))
            assert in_off == lay["maps"][m][4][stage - 1] and out_off == lay["maps"][m][4][stage] and first_block == sum(1 for b in bands if b[1] < m)
            assert in_bytes == ref.stage_bytes(*lay["maps"][m][2])[stage - 1] == (2 * row_pairs + 2) * iw * IN_DWORDS[stage] * 4
