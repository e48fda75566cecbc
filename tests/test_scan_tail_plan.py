"""CPU: the band tables of the clip scan's stages 4 and 5 on the matrix cores (clip_tail_tables), printed by a stand-alone program built
here under ASan + UBSan: bands in their maps, covering them exactly once, patches inside the input map, the layout's offsets.  Widths 144 ..
160 / 272 .. 288 put both stages under, at and over a 32-pair tile / the 64-column band; heights 48 .. 64 the band's four row pairs."""
import os
import subprocess

import pytest

import gpu_lib as gl
import scan_clip_ref as ref

CSRC, IN_DWORDS = os.path.join(gl.ROOT, "bnn-pynq_amd", "csrc"), {4: 4, 5: 8}  # (dwords per pixel of the stage's input map)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("scan_tail") / "tables")
    srcs = [os.path.join(gl.ROOT, "tests", "host_scan_tail", "main.cpp"), os.path.join(CSRC, "scan_clip.cpp"), os.path.join(CSRC, "scan.cpp")]
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, "-o", path] + srcs,
                   check=True)
    return path


@pytest.mark.parametrize("width,height,frames,sizes", [(w, h, 1, (32,)) for w in (32, *range(144, 161, 4), *range(272, 289, 4))
                                                       for h in (32, *range(48, 65, 4))] + [(100, 52, 3, (32, 40)), (640, 480, 2, (64, 96))])
def test_bands_cover_every_map(exe, width, height, frames, sizes):
    out = subprocess.run([exe, str(width), str(height), str(frames)] + [str(s) for s in sizes], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    rows = [l.split() for l in out.stdout.splitlines()]
    max_rps, max_cols = (int(v) for v in rows[0][1:])
    lay = ref.layout(width, height, sizes, frames)
    for stage in (4, 5):
        maps = [[int(v) for v in r[2:]] for r in rows if r[0] == "map" and int(r[1]) == stage]
        bands = [[int(v) for v in r[2:]] for r in rows if r[0] == "band" and int(r[1]) == stage]
        assert len(maps) == len(lay["maps"]) and [b[0] for b in bands] == list(range(len(bands)))
        covered = [set() for _ in maps]
        for block, m, rp0, x0 in bands:
            _, in_off, out_off, ow, oh, band_cols, band_rps, first_block, in_bytes, iw, ih = maps[m]
            assert 0 < band_cols <= max_cols and 0 < band_rps <= max_rps and block >= first_block
            assert 0 <= 2 * rp0 < oh and 0 <= x0 < ow and rp0 % band_rps == 0 and x0 % band_cols == 0
            nrp, cols = min(band_rps, (oh + 1) // 2 - rp0), min(band_cols, ow - x0)  # as the kernel takes them
            cells = {(y, x) for y in range(2 * rp0, min(2 * (rp0 + nrp), oh)) for x in range(x0, x0 + cols)}
            assert nrp > 0 and cols > 0 and not (cells & covered[m]), "an output pixel in two bands"
            covered[m] |= cells
            prows = min(2 * nrp + 2, oh + 2 - 2 * rp0)  # the patch the kernel loads: rows 2 rp0 .. 2 rp0 + prows - 1, columns x0 .. x0 + cols + 1
            assert 2 * rp0 + prows <= ih and x0 + cols + 2 <= iw and ((2 * rp0 + prows - 1) * iw + x0 + cols + 2) * IN_DWORDS[stage] * 4 <= in_bytes
            assert prows >= min(2 * (rp0 + nrp), oh) - 2 * rp0 + 2  # ... holds every input row of the band's real outputs
        for m, (_, in_off, out_off, ow, oh, band_cols, band_rps, first_block, in_bytes, iw, ih) in enumerate(maps):
            nx, ny = lay["maps"][m][2]
            assert len(covered[m]) == ow * oh and (ow, oh) == ((nx + 2, ny + 2) if stage == 4 else (nx, ny)) and (iw, ih) == (ow + 2, oh + 2)
            assert in_off == lay["maps"][m][4][stage - 1] and out_off == lay["maps"][m][4][stage] and first_block == sum(1 for b in bands if b[1] < m)
            assert in_bytes == ref.stage_bytes(nx, ny)[stage - 1] == ih * iw * IN_DWORDS[stage] * 4
