"""CPU test of the yardstick itself: tests/_resize_ref.py (the numpy restatement of cv::resize that the GPU resize and ingest
tests compare against) agrees with the oracle's C restatement where one exists, and with hand arithmetic elsewhere."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _resize_ref as RR   # noqa: E402

SIZES = [(832, 256, 499, 154), (1241, 376, 620, 188), (1280, 720, 768, 432), (1920, 1080, 1152, 648),
         (1226, 370, 1022, 308), (640, 480, 213, 160), (2208, 1242, 1325, 745), (333, 127, 111, 42), (416, 128, 416, 128)]


@pytest.mark.parametrize("sw,sh,dw,dh", SIZES)
def test_bilinear_equals_the_oracle(oracle, sw, sh, dw, dh):
    img = np.random.default_rng(3).integers(0, 256, (sh, sw), dtype=np.uint8)
    assert not RR.is_box(sw, sh, dw, dh)
    a, b = RR.resize_linear(img, dw, dh), oracle.resize_linear(img, dw, dh)
    assert a.shape == b.shape == (dh, dw)
    assert int((a != b).sum()) == 0


def test_nearest_half_is_every_other_pixel():
    img = np.random.default_rng(4).integers(0, 256, (376, 1241), dtype=np.uint8)
    assert RR.out_size(1241, 376, 0.5, 0.5) == (620, 188)           # cvRound(620.5) = 620: ties to even
    assert np.array_equal(RR.resize_nearest(img, 620, 188, 0.5, 0.5), img[::2, ::2][:188, :620])
    img = np.random.default_rng(5).integers(0, 256, (1080, 1920), dtype=np.uint8)
    assert np.array_equal(RR.resize(img, 960, 540, "nearest", 0.5, 0.5), img[::2, ::2])
    # the size form of the same destination is another scale (1241 / 620 = 2.0016...): no box reroute for INTER_LINEAR
    assert RR.is_box(1241, 376, 620, 188, 0.5, 0.5) and not RR.is_box(1241, 376, 620, 188)


def test_box_branch_by_hand():
    img = np.array([[0, 1, 10, 13], [2, 3, 11, 12], [255, 255, 7, 0], [255, 254, 0, 0]], np.uint8)
    out = RR.resize_linear(img, 2, 2, 0.5, 0.5)
    # (0+1+2+3+2)>>2 = 2, (10+13+11+12+2)>>2 = 12, (255+255+255+254+2)>>2 = 255, (7+0+0+0+2)>>2 = 2
    assert out.tolist() == [[2, 12], [255, 2]]
    assert RR.is_box(4, 4, 2, 2) and RR.is_box(4, 4, 2, 2, 0.5, 0.5)
    assert np.array_equal(RR.resize_linear(img, 2, 2), out)         # size form at exactly 2x: the same reroute
    # odd source: the spare row / column is not read
    img5 = np.pad(img, ((0, 1), (0, 1)), constant_values=200)
    assert RR.out_size(5, 5, 0.5, 0.5) == (2, 2)
    assert np.array_equal(RR.resize_linear(img5, 2, 2, 0.5, 0.5), out)


@pytest.mark.parametrize("interp", ["nearest", "linear"])
def test_identity(interp):
    img = np.random.default_rng(6).integers(0, 256, (128, 416), dtype=np.uint8)
    assert np.array_equal(RR.resize(img, 416, 128, interp), img)
    assert np.array_equal(RR.resize(img, 416, 128, interp, 1.0, 1.0), img)


def test_argument_rules():
    img = np.zeros((100, 200), np.uint8)
    with pytest.raises(AssertionError):
        RR.resize_nearest(img, 101, 50, 0.5, 0.5)                   # dsize != cvRound(ssize * f)
    with pytest.raises(AssertionError):
        RR.resize_nearest(img, 400, 200)                            # upscale
    with pytest.raises(AssertionError):
        RR.resize_linear(np.zeros((5, 5), np.uint8), 3, 3, 0.5, 0.5)    # cvRound(2.5) = 2, not 3
