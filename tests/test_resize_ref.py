"""CPU: tests/resize_ref.py against Pillow itself, on every (shape, content, mode) that test_gpu_scan_resize.py sends to the
device, and the preconditions that keep those GPU tests from going blind: where a case is there to tell the two pass
orders apart, the other order must give other bytes; where it is there for clip8, both ends of clip8 must work in
every pass.  These are conditions on the inputs, computed from the restatement alone -- no kernel runs here."""
import numpy as np
import pytest

import resize_ref as rr
import scan_ref

PIL = pytest.importorskip("PIL")
from PIL import Image  # noqa: E402


def pillow(a, out_w, out_h):
    return np.asarray(Image.fromarray(a).resize((out_w, out_h), Image.LANCZOS))


# the scenes of test_gpu_scan_resize.py's scan_scene / scan_clip tests: (w, h, mode, seed, level size)
SCENES = [(40, 4001, "RGB", 11, 40), (40, 4001, "RGB", 12, 40), (40, 4001, "L", 13, 40), (40, 4000, "RGB", 14, 40)]


@pytest.mark.parametrize("case", rr.CASES, ids=rr.case_id)
def test_restatement_equals_pillow(case):
    w, h, ow, oh = case[:4]
    for mode in rr.MODES:
        for kind in rr.KINDS:
            a = rr.picture(w, h, mode, kind)
            got, want = rr.resize(a, ow, oh), pillow(a, ow, oh)
            assert got.shape == want.shape and (got == want).all(), (case[:5], mode, kind, int((got != want).sum()))


def test_restatement_equals_pillow_on_the_scenes():
    for w, h, mode, seed, size in SCENES:
        a = rr.blocks_plus_noise(w, h, mode, seed)
        lw, lh = scan_ref.level(w, h, size)
        assert (lw, lh) == (32, 3200)
        assert (rr.resize(a, lw, lh) == pillow(a, lw, lh)).all(), (w, h, mode)
    a = np.random.default_rng(7).integers(0, 256, (72, 80, 3), dtype=np.uint8)  # the scene of test_gpu_scan.py::test_scan_scene
    for size in (64, 48):
        lw, lh = scan_ref.level(80, 72, size)
        assert (rr.resize(a, lw, lh) == pillow(a, lw, lh)).all(), size


def test_pass_order_rule_equals_pillows():
    """on either side of the edge, only the restatement's own order gives Pillow's bytes"""
    for w, h, ow, oh, first in [(8, 800, 6, 600, False), (8, 801, 6, 600, True), (8, 801, 6, 801, False), (8, 801, 6, 900, False),
                                (40, 4000, 32, 3200, False), (40, 4001, 32, 3200, True)]:
        assert rr.vertical_pass_first(w, h, oh) == first
        if oh == h:
            continue
        a = rr.picture(w, h, "RGB", "noise")
        want = pillow(a, ow, oh)
        assert (rr.resize(a, ow, oh, vertical_first=first) == want).all(), (w, h)
        assert (rr.resize(a, ow, oh, vertical_first=not first) != want).any(), (w, h)


@pytest.mark.parametrize("case", [c for c in rr.CASES if rr.order_kind(c)], ids=rr.case_id)
def test_both_orders_differ(case):
    w, h, ow, oh = case[:4]
    kind = rr.order_kind(case)
    for mode in rr.marked_modes(case):
        a = rr.picture(w, h, mode, kind)
        other = rr.resize(a, ow, oh, vertical_first=not rr.vertical_pass_first(w, h, oh))
        n = int((other != pillow(a, ow, oh)).sum())
        print(case[:5], mode, kind, "bytes the other order changes:", n)
        assert n >= rr.ORDER_MIN_BYTES, (case[:5], mode, n)


def clip_counts(a, ow, oh):
    """[(pass, samples below 0, samples above 255)] of every pass that runs"""
    return [(name, int((raw < 0).sum()), int((raw > 255).sum())) for name, raw in rr.passes(a, ow, oh)[1]]


@pytest.mark.parametrize("case", [c for c in rr.CASES if "clips" in c[5]], ids=rr.case_id)
def test_both_ends_clip_in_every_pass(case):
    w, h, ow, oh = case[:4]
    for mode in rr.marked_modes(case):
        counts = clip_counts(rr.picture(w, h, mode, "blocks"), ow, oh)
        print(case[:5], mode, counts)
        assert len(counts) == (ow != w) + (oh != h)
        for name, low, high in counts:
            assert low >= rr.CLIPS_MIN and high >= rr.CLIPS_MIN, (case[:5], mode, name, low, high)


def test_the_scenes_clip_and_tell_the_orders_apart():
    """the blocks-plus-noise scenes that go through scan_scene and scan_clip: clip8 still works at both ends of both
    passes, and the other pass order gives another level picture"""
    for w, h, mode, seed, size in SCENES:
        a = rr.blocks_plus_noise(w, h, mode, seed)
        lw, lh = scan_ref.level(w, h, size)
        for name, low, high in clip_counts(a, lw, lh):
            assert low >= rr.CLIPS_MIN and high >= rr.CLIPS_MIN, (w, h, mode, name, low, high)
        other = rr.resize(a, lw, lh, vertical_first=not rr.vertical_pass_first(w, h, lh))
        assert int((other != rr.resize(a, lw, lh)).sum()) >= rr.ORDER_MIN_BYTES, (w, h, mode)
