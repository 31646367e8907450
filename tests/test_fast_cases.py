"""The inputs of tests/_fast_cases.py reach what they are meant to reach -- shown on the CPU oracle alone (no GPU): a tile
row with 64 corners without NMS and 32 survivors with it (the two record bounds of csrc/fast_scratch.h), emit groups with
and without corners, scores of 0 and of 254, and the clamp of the threshold.  tests/test_gpu_fast_bounds.py then holds
fast.hip to the oracle on the same inputs, so none of its comparisons can pass on an input that misses its point."""
import numpy as np
import pytest

import _fast_cases as fc
from conftest import rand_image

W, H = 135, 39                                  # three tile columns (the last one 7 pixels), two tile rows (the last one 7 rows)
NINE = tuple(range(3, 36, 4))                   # 3, 7, ..., 35: eight rows in tile row 0, the last in tile row 1


@pytest.mark.parametrize("y0", [3, 19, 31, 32, 35])
@pytest.mark.parametrize("thr", [0, 7])
def test_staircase_saturates_one_tile_row(oracle, y0, thr):
    img = fc.staircase_rows(W, H, (y0,))
    assert img[y0].max() == 243 and (np.delete(img, y0, 0) == 255).all()
    all_ = oracle.fast(img, thr, False)
    kept = oracle.fast(img, thr, True)
    assert (all_["y"] == y0).all() and (kept["y"] == y0).all()
    # 61 .. 127 and 131 without NMS; the odd ones of those with it
    assert np.array_equal(all_["x"], np.r_[61:128, 131]) and len(all_) == 68
    assert np.array_equal(kept["x"], np.r_[61:128:2, 131]) and len(kept) == 35
    assert fc.per_tile_row(all_, W, H)[y0].tolist() == [3, 64, 1]
    assert fc.per_tile_row(kept, W, H)[y0].tolist() == [2, 32, 1]
    assert (all_["response"] == 0).all()
    assert (kept["response"][:-1] == 11).all() and kept["response"][-1] == 230      # steps[1] - 1; v(128) - 1 at x = 131


@pytest.mark.parametrize("thr", [0, 7])
def test_nine_staircase_rows(oracle, thr):
    img = fc.staircase_rows(W, H, NINE)
    assert sum(y < 32 for y in NINE) == 8 and NINE[-1] == 35
    for nms, per_row, in_tile in ((False, 68, 64), (True, 35, 32)):
        kps = oracle.fast(img, thr, nms)
        counts = fc.per_tile_row(kps, W, H)
        assert len(kps) == 9 * per_row
        for y in range(H):
            assert counts[y].sum() == (per_row if y in NINE else 0) and counts[y, 1] == (in_tile if y in NINE else 0)


def test_two_saturated_tile_columns_side_by_side(oracle):
    """199x39, x_hi = 191.  With the default steps the staircase reaches 255 at x = 133 (243 at 130, + 12), so tile column 2
    does NOT saturate: column 1 does, and column 2 holds a few live corners beside it ("clipped").  Two more images cover
    what that one cannot: steps (5, 6) stay below 255 over 61 .. 194 and saturate columns 1 AND 2 side by side -- at thr 0
    only, the steps being below 7 ("both") -- and the default steps shifted to x_lo = 125 saturate column 2 alone at
    thr 0 and 7 ("col2")."""
    w, h, y0 = 199, 39, 19
    for thr in (0, 7):
        img = fc.staircase_rows(w, h, (y0,), x_hi=191)
        assert img[y0].max() == 255
        a, k = (fc.per_tile_row(oracle.fast(img, thr, nms), w, h)[y0] for nms in (False, True))
        assert a[1] == 64 and k[1] == 32 and 0 < a[2] < 64 and 0 < k[2] < 32
        img = fc.staircase_rows(w, h, (y0,), x_lo=125, x_hi=191)
        assert img[y0].max() == 243
        a, k = (fc.per_tile_row(oracle.fast(img, thr, nms), w, h)[y0] for nms in (False, True))
        assert a.tolist() == [0, 3, 64, 1] and k.tolist() == [0, 2, 32, 1]
    img = fc.staircase_rows(w, h, (y0,), x_hi=191, steps=(5, 6))
    assert img[y0].max() == 242
    a, k = (fc.per_tile_row(oracle.fast(img, 0, nms), w, h)[y0] for nms in (False, True))
    assert a.tolist() == [3, 64, 64, 1] and k.tolist() == [2, 32, 32, 1]
    kept = oracle.fast(img, 0, True)
    assert (kept["response"][:-1] == 5).all()
    assert len(oracle.fast(img, 7, False)) == 1                     # x = 195 alone: the steps are below the threshold


@pytest.mark.parametrize("w,h", fc.EMIT_SHAPES, ids=[f"{w}x{h}" for w, h in fc.EMIT_SHAPES])
def test_emit_shapes_fill_their_groups(oracle, w, h):
    total = fc.count_bytes(w, h)
    assert total == {(512, 128): 1024, (64, 1025): 1025, (64, 1029): 1029, (128, 517): 1034, (192, 345): 1035}[(w, h)]
    img = fc.emit_image(w, h)
    for thr in (7, 20):
        for nms in (True, False):
            g = fc.per_group(oracle.fast(img, thr, nms, cap=w * h), w, h)
            assert len(g) == (total + fc.GROUP - 1) // fc.GROUP
            assert g[0] > 1024                                      # more corners than entries: the block scan carries
            if (w, h) == (64, 1025):
                assert g[1] == 0                                    # y = 1024 is inside the 3-pixel border
            elif len(g) > 1:
                assert 16 <= g[1] <= 85, (thr, nms, g)


def test_minus_one(oracle):
    img = fc.minus_one(71, 39, 35, 19)
    kp = oracle.fast(img, 0, False)
    assert len(kp) == 1 and (kp["x"][0], kp["y"][0]) == (35, 19)
    assert len(oracle.fast(img, 0, True)) == 0                      # its score is 0: no keypoint
    assert len(oracle.fast(img, 1, False)) == 0 and len(oracle.fast(img, 1, True)) == 0


def test_lattice_extremes_and_the_threshold_clamp(oracle):
    img = fc.lattice(71, 39, 0, 255)
    for nms in (True, False):
        at0, at255 = oracle.fast(img, 0, nms), oracle.fast(img, 255, nms)
        for thr in (-5, 0, 1, 127, 128, 254):
            kp = oracle.fast(img, thr, nms)
            assert len(kp) == 153 and (kp["response"] == (254 if nms else 0)).all(), (thr, nms)
        assert len(at255) == 0 and len(oracle.fast(img, 300, nms)) == 0
        assert oracle.fast(img, -5, nms).tobytes() == at0.tobytes()                 # the clamp: -5 is 0 ...
        noise = rand_image(39, 71, 3, blocks=False)
        assert oracle.fast(noise, -5, nms).tobytes() == oracle.fast(noise, 0, nms).tobytes()
        assert oracle.fast(noise, 300, nms).tobytes() == oracle.fast(noise, 255, nms).tobytes()   # ... and 300 is 255
    # the noise of test_threshold_extremes is not vacuous at any of its thresholds, and thr 0 / 1 differ
    n = {(thr, nms): len(oracle.fast(noise, thr, nms)) for thr in (0, 1, 128) for nms in (True, False)}
    assert min(n.values()) > 0 and n[(0, False)] > n[(1, False)] > n[(128, False)]
