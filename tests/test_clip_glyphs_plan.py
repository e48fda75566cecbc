"""CPU: the host-only plan of the clip of glyphs (csrc/clip_glyphs.{h,cpp}) -- the split of a component list into frames and
the limits -- in a stand-alone program built with AddressSanitizer and UBSan (tests/host_clip_glyphs/main.cpp)."""
import os
import subprocess

import pytest

import gpu_lib as gl

CSRC = os.path.join(gl.ROOT, "bnn-pynq_amd", "csrc")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("clip_glyphs") / "plan")
    srcs = [os.path.join(gl.ROOT, "tests", "host_clip_glyphs", "main.cpp")] + [os.path.join(CSRC, s) for s in
                                                                                ("clip_glyphs.cpp", "page.cpp", "components.cpp", "glyphs.cpp",
                                                                                 "resample.cpp")]
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    "-o", path] + srcs, check=True)
    return path


def run(exe, *args, stdin=""):
    out = subprocess.run([exe] + [str(a) for a in args], input=stdin, capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout.splitlines()


# a clip of 3 frames of 20 x 10 (frame f: rows 10 f .. 10 f + 9, first pixels 200 f .. 200 f + 199), tall coordinates, in the
# device's arrival order (none): (first, left, upper, right, lower, pixels)
W, H = 20, 10
LIST = [(2 * 200 + 3 * W + 12, 12, 23, 15, 27, 9),   # frame 2, right
        (5, 5, 0, 8, 4, 7),                          # frame 0: a first line of two ...
        (0 * 200 + 6 * W + 1, 1, 6, 4, 10, 6),       # frame 0: ... and a second line, further left: it touches the frame's last row
        (2 * 200 + 2 * W + 1, 1, 22, 4, 26, 8),      # frame 2, left: first in both orders
        (1, 0, 1, 3, 4, 5),                          # frame 0, first line, left of (5, ...) but later in raster order
        (2 * 200 + 9 * W + 19, 19, 29, 20, 30, 1)]   # frame 2: a speck in the clip's last pixel
TEXT = "\n".join(" ".join(str(v) for v in c) for c in LIST)


def frames(lines):
    out, cur = [], None
    for l in lines:
        v = l.split()
        if v[0] == "frame":
            cur = dict(total=int(v[2]), kept=int(v[3]), rows=[])
            out.append(cur)
        else:
            cur["rows"].append(tuple(int(x) for x in v))
    return out


@pytest.mark.parametrize("cap,lines,order,min_pixels,want", [
    # raster order: ascending first pixel; the empty frame 1 is there with nothing in it; boxes in FRAME rows
    (8, 0, 0, 1, [(3, [(1, 0, 1, 3, 4), (5, 5, 0, 8, 4), (121, 1, 6, 4, 10)]), (0, []), (3, [(441, 1, 2, 4, 6), (472, 12, 3, 15, 7), (599, 19, 9, 20, 10)])]),
    # left order: ascending (left, upper, first)
    (8, 0, 1, 1, [(3, [(1, 0, 1, 3, 4), (121, 1, 6, 4, 10), (5, 5, 0, 8, 4)]), (0, []), (3, [(441, 1, 2, 4, 6), (472, 12, 3, 15, 7), (599, 19, 9, 20, 10)])]),
    # the line model per frame, then the cap per frame: the totals stay what they were
    (2, 1, 0, 1, [(3, [(1, 0, 1, 3, 4), (5, 5, 0, 8, 4)]), (0, []), (3, [(441, 1, 2, 4, 6), (472, 12, 3, 15, 7)])]),
    # min_pixels drops the speck from the total too
    (8, 1, 0, 2, [(3, [(1, 0, 1, 3, 4), (5, 5, 0, 8, 4), (121, 1, 6, 4, 10)]), (0, []), (2, [(441, 1, 2, 4, 6), (472, 12, 3, 15, 7)])]),
])
def test_split_by_frame(exe, cap, lines, order, min_pixels, want):
    got = frames(run(exe, "split", 3, W, H, cap, lines, order, min_pixels, stdin=TEXT))
    assert [(f["total"], [r[:5] for r in f["rows"]]) for f in got] == want
    assert all(f["kept"] == len(f["rows"]) == min(cap, f["total"]) for f in got)
    if lines and cap == 8:  # frame 0 holds two lines, frame 2 starts again at line 0
        assert [r[5] for r in got[0]["rows"]] == [0, 0, 1] and got[2]["rows"][0][5] == 0
    else:
        assert lines or all(r[5] == 0 and r[6] == 0 for f in got for r in f["rows"])


def test_a_component_that_leaves_its_frame_is_an_internal_error(exe):
    assert "leaves its frame" in run(exe, "split", 3, W, H, 8, 0, 0, 1, stdin="5 5 8 8 12 9")[0]


@pytest.mark.parametrize("args,want", [
    ((1, 0, 64, 32, 64, 1), "ok 1 1 1 512"), ((3, 0, 65, 33, 65, 1), "ok 2 2 12 1683"), ((54, 0, 640, 480, 640, 4096), "ok 10 15 8100 4147200"),
    ((0, 0, 64, 32, 64, 1), "n_frames must be 1..4096"), ((4097, 0, 1, 1, 1, 1), "n_frames must be 1..4096"),
    ((55, 0, 640, 480, 640, 1), "at most 16777216 pixels"), ((4096, 0, 64, 64, 64, 1), "ok 1 2 8192 4194304"),
    ((2, 64 * 32 - 1, 64, 32, 64, 1), "frame stride shorter"), ((2, 80 * 32, 64, 32, 80, 1), "ok 1 1 2 1024"),
    ((2, 0, 64, 32, 64, 0), "cap must be 1 or more"), ((4096, 0, 4, 4, 4, 1 << 20), "cap must be 1 or more"),
])
def test_limits(exe, args, want):
    assert want in run(exe, "limits", *args)[0]
