"""CPU tests: known answers of tests/_gftt_ref.py, the numpy restatement of cv::goodFeaturesToTrack that the Shi-Tomasi
kernels (csrc/gftt.hip) are compared with bit for bit in tests/test_gpu_gftt.py."""
import math

import numpy as np
import pytest

import _gftt_ref as G
import conftest


def _square(h=40, w=48, y0=12, x0=15, n=9):
    img = np.zeros((h, w), np.uint8)
    img[y0:y0 + n, x0:x0 + n] = 255
    return img


def test_flat_image_gives_nothing():
    for v in (0, 77, 255):
        img = np.full((24, 31), v, np.uint8)
        eig = G.min_eigen_map(img)
        assert np.all(eig == 0)
        kp, s = G.gftt(img, 0, 0.01, 0)
        assert len(kp) == 0 and len(s) == 0


def test_bright_square_gives_its_four_corners():
    img = _square()
    kp, s = G.gftt(img, 0, 0.01, 3.0)
    assert len(kp) == 4
    corners = [(15, 12), (23, 12), (15, 20), (23, 20)]
    for k in kp:
        d = min(max(abs(k["x"] - cx), abs(k["y"] - cy)) for cx, cy in corners)
        assert d <= 1                                                   # inside a corner's 3x3 neighbourhood
    near = {min(range(4), key=lambda i: abs(k["x"] - corners[i][0]) + abs(k["y"] - corners[i][1])) for k in kp}
    assert near == {0, 1, 2, 3}                                         # one per corner
    assert np.all(kp["size"] == 3) and np.all(kp["angle"] == -1) and np.all(kp["response"] == 0)
    assert np.all(kp["octave"] == 0) and np.all(kp["class_id"] == -1)
    assert np.all(np.diff(s) <= 0) and s.dtype == np.float32


@pytest.mark.parametrize("md", [1.0, 1.5, 2.5, 20.0])
def test_grid_greedy_equals_brute_force(md):
    assert G.cv_round(1.5) == 2 and G.cv_round(2.5) == 2 and G.cv_round(0.5) == 0 and G.cv_round(20.0) == 20
    for seed in range(4):
        rng = np.random.default_rng(100 + seed)
        w, h = (37, 29) if md < 3 else (203, 131)
        n = 400 if md < 3 else 1500
        p = rng.choice(w * h, n, replace=False)
        xs, ys = p % w, p // w
        for maxc in (0, 7, 10 ** 6):
            a = G.greedy_grid(xs, ys, w, h, maxc, md)
            b = G.greedy_brute(xs, ys, maxc, md)
            assert np.array_equal(a, b) and len(a) > 0
            if maxc == 7:
                assert len(a) == 7
            kx, ky = xs[a].astype(np.int64), ys[a].astype(np.int64)
            d2 = (kx[:, None] - kx[None]) ** 2 + (ky[:, None] - ky[None]) ** 2
            d2[np.arange(len(a)), np.arange(len(a))] = 10 ** 9
            assert d2.min() >= md * md                                  # every kept pair is >= min_distance apart
            # at most four kept corners per grid cell (csrc/gftt.hip: kGfttCellCap)
            cell = G.cv_round(md)
            assert np.bincount((ky // cell) * ((w + cell - 1) // cell) + kx // cell).max() <= 4


def test_no_spacing_below_one():
    xs, ys = np.arange(10), np.zeros(10, np.int64)
    assert np.array_equal(G.greedy_grid(xs, ys, 10, 1, 0, 0.99), np.arange(10))
    assert np.array_equal(G.greedy_grid(xs, ys, 10, 1, 4, 0.0), np.arange(4))
    assert np.array_equal(G.greedy_grid(xs, ys, 10, 1, -1, 0.5), np.arange(10))


def test_ties_go_to_the_larger_raster_index():
    # a left-right and up-down symmetric image: equal eigenvalues occur at mirrored positions
    q = conftest.rand_image(20, 24, 5)
    img = np.block([[q, q[:, ::-1]], [q[::-1], q[::-1, ::-1]]])
    eig = G.min_eigen_map(img)
    assert np.array_equal(eig, eig[:, ::-1]) and np.array_equal(eig, eig[::-1])
    idx = G.candidates(eig, 0.01)
    val = eig.reshape(-1)[idx]
    assert len(idx) >= 8 and np.all(np.diff(val) <= 0)
    tied = np.flatnonzero(np.diff(val) == 0)
    assert len(tied) >= 3
    assert np.all(idx[tied] > idx[tied + 1])                            # 3.4's greaterThanPtr
    kp, s = G.gftt(img, 0, 0.01, 0.0)
    assert np.array_equal(kp["y"].astype(np.int64) * img.shape[1] + kp["x"].astype(np.int64), idx)


def _pad_then_compute(img):
    """the WRONG border: the covariance of the image reflected by 2, cropped"""
    big = np.pad(img, 2, mode="reflect")
    return G.min_eigen_map(big)[2:-2, 2:-2]


def test_covariance_border_is_that_of_the_maps():
    img = conftest.rand_image(33, 41, 9)
    eig = G.min_eigen_map(img)
    # column 0 and row 0 by the recipe, scalar by scalar
    dx, dy = G.sobel(img)
    h, w = img.shape
    r = lambda i, n: -i if i < 0 else (2 * n - 2 - i if i >= n else i)

    def one(x, y):
        rows = []
        for j in (-1, 0, 1):
            t = [[], [], []]
            for i in (-1, 0, 1):
                vx, vy = dx[r(y + j, h), r(x + i, w)], dy[r(y + j, h), r(x + i, w)]
                t[0].append(float(np.float32(vx * vx))); t[1].append(float(np.float32(vx * vy))); t[2].append(float(np.float32(vy * vy)))
            rows.append([(q[0] + q[1]) + q[2] for q in t])
        s = [(rows[0][k] + rows[1][k]) + rows[2][k] for k in range(3)]
        a, b, c = np.float32(s[0]) * np.float32(0.5), np.float32(s[1]), np.float32(s[2]) * np.float32(0.5)
        return np.float32((a + c) - np.sqrt((a - c) * (a - c) + b * b))

    for y in range(h):
        assert eig[y, 0] == one(0, y) and eig[y, w - 1] == one(w - 1, y)
    for x in range(w):
        assert eig[0, x] == one(x, 0) and eig[h - 1, x] == one(x, h - 1)
    wrong = _pad_then_compute(img)
    assert np.array_equal(wrong[2:-2, 2:-2], eig[2:-2, 2:-2])           # the interior does not see the border
    assert np.any(wrong[:, 0] != eig[:, 0]) and np.any(wrong[0] != eig[0])


def test_double_sums_equal_fsum():
    img = conftest.rand_image(35, 67, 3)
    dx, dy = G.sobel(img)
    sums = G.cov_sums(img)
    # Where a product is tiny beside its neighbours (dy = q[y+1] - q[y-1] of two nearly equal floats leaves a rounding
    # residue of 1e-8 where the integers cancel) the nine products do not sum exactly in 53 bits: the recipe fixes the order
    # -- a box filter's: (p0 + p1) + p2 per row, then (r0 + r1) + r2 -- and on THIS image what it rounds to float32 is the
    # exactly rounded sum at every pixel.
    inexact = 0
    for c, s in zip((dx * dx, dx * dy, dy * dy), sums):
        assert c.dtype == np.float32
        p = np.pad(c, 1, mode="reflect")
        for y in range(35):
            for x in range(67):
                win = p[y:y + 3, x:x + 3].reshape(-1)
                exact = math.fsum(float(v) for v in win)
                r = [(float(win[3 * j]) + float(win[3 * j + 1])) + float(win[3 * j + 2]) for j in range(3)]
                seq = (r[0] + r[1]) + r[2]
                assert s[y, x] == seq                                   # the stated order
                assert np.float32(s[y, x]) == np.float32(exact)
                inexact += s[y, x] != exact
    print("sums that are not exact in double:", inexact, "of", 3 * 35 * 67)


def test_sobel_known_answers():
    img = np.zeros((5, 7), np.uint8)
    img[:, 4:] = 255                                                    # a vertical step
    dx, dy = G.sobel(img)
    assert np.all(dy == 0)
    assert np.allclose(dx[:, 3], 255 * 4 * float(G.S)) and np.allclose(dx[:, 4], 255 * 4 * float(G.S)) and np.all(dx[:, :3] == 0)
    assert G.S == np.float32(1.0 / 3060.0) and G.F0 == np.float32(2) * G.S


def test_threshold_is_strict_and_in_double():
    img = conftest.rand_image(40, 56, 2)
    eig = G.min_eigen_map(img)
    assert len(G.candidates(eig, 1.0)) == 0                             # eig > thr is strict
    assert G.threshold(eig, 0.01) == np.float32(float(eig.max()) * 0.01)
    assert (eig < 0).sum() >= 0 and eig.dtype == np.float32
    n_all, n_q = len(G.candidates(eig, 1e-6)), len(G.candidates(eig, 0.01))
    assert n_all > n_q > 0


def test_against_opencv_if_present():
    cv2 = pytest.importorskip("cv2")
    img = conftest.rand_image(97, 161, 4)
    eig = G.min_eigen_map(img)
    ref = cv2.cornerMinEigenVal(img, 3, ksize=3)
    diff = np.abs(ref - eig)
    print("cornerMinEigenVal: max abs diff", diff.max(), "pixels that differ", int((ref != eig).sum()))
    pts = cv2.goodFeaturesToTrack(img, 500, 0.01, 20)
    kp, _ = G.gftt(img, 500, 0.01, 20)
    got = np.stack([kp["x"], kp["y"]], 1)
    print("goodFeaturesToTrack: ", len(pts), "corners, reference", len(kp))
    assert diff.max() <= 1e-6 * max(1.0, float(np.abs(ref).max()))
    assert len(pts) == len(kp) and np.array_equal(pts.reshape(-1, 2), got)
