"""CPU tests of the guided ORB matcher's reference twin (tests/_orbmatch_ref.py): hand-built cases that pin every rule of
stages S and T as include/svo_abi.h states them, and the quality test -- the matcher must give the pose solver at least twice
the brute-force matcher's inliers on the synthetic sequences (the reason it exists)."""
import numpy as np
import pytest

import _orbmatch_ref as M

F = np.float32
W, H, NL = 160, 100, 8


def _kps(oracle, rows):
    k = np.zeros(len(rows), dtype=oracle.KP_DTYPE)
    for i, (x, y, o) in enumerate(rows):
        k[i]["x"], k[i]["y"], k[i]["octave"] = x, y, o
    return k


def _flip(d, nbits):
    out = d.copy()
    for b in range(nbits):
        out[b // 8] ^= np.uint8(1 << (b % 8))
    return out


def _scene(shift=6, noise=True, seed=1):
    """Eight equal-size random levels; the right image is the left one moved `shift` pixels to the left (disparity = shift),
    plus a little noise so that no SAD is exactly zero."""
    rng = np.random.default_rng(seed)
    levL = [rng.integers(0, 256, (H, W), dtype=np.uint8) for _ in range(NL)]
    levR = []
    for L in levL:
        R = np.roll(L, -shift, axis=1).astype(np.int32)
        if noise:
            R = np.clip(R + rng.integers(-2, 3, R.shape), 0, 255)
        levR.append(R.astype(np.uint8))
    return levL, levR, rng


def _stereo1(oracle, left, rights, levL, levR, maxd=30.0, dR=None, th=75, seed=2):
    """Stage S of ONE left keypoint against the listed right keypoints; equal descriptors unless given."""
    rng = np.random.default_rng(seed)
    dL = rng.integers(0, 256, (1, 32), dtype=np.uint8)
    dR = np.repeat(dL, len(rights), 0) if dR is None else dR
    uR, sd, _ = M.stereo(_kps(oracle, [left]), dL, _kps(oracle, rights), dR, levL, levR, maxd, th)
    return float(uR[0]), int(sd[0])


def test_scales_are_the_extractors(oracle):
    sc, inv = M.scales()
    osc, oinv, _, _ = oracle.orb_setup()
    assert sc.tobytes() == osc.tobytes() and inv.tobytes() == oinv.tobytes()


def test_band_edges_floor_and_ceil(oracle):
    levL, levR, _ = _scene()
    left = (80.0, 40.3, 0)                                   # truncf(vL) = 40; r_j = 2 at octave 0
    for yj, ok in [(42.5, True), (43.0, False), (37.5, True), (37.0, False), (40.0, True)]:
        uR, sd = _stereo1(oracle, left, [(74.0, yj, 0)], levL, levR)
        assert (uR >= 0) == ok, yj
        if ok:
            assert abs(uR - 74.0) < 0.5 and sd > 0


def test_octave_limit(oracle):
    levL, levR, _ = _scene()
    for oj, ok in [(0, True), (1, True), (2, False)]:
        uR, _ = _stereo1(oracle, (80.0, 40.0, 0), [(74.0, 40.0, oj)], levL, levR)
        assert (uR >= 0) == ok, oj
    uR, _ = _stereo1(oracle, (80.0, 40.0, 3), [(74.0 * 1.728, 40.0, 1)], levL, levR)
    assert uR < 0


def test_disparity_bounds_and_clamp(oracle):
    levL, levR, _ = _scene(shift=6)
    # candidate window uL - maxD <= x_j <= uL (maxD = 10): x_j = 70 is a candidate (the slide reaches column 74), 69.9 is not
    assert _stereo1(oracle, (80.0, 40.0, 0), [(70.0, 40.0, 0)], levL, levR, maxd=10.0)[0] >= 0
    assert _stereo1(oracle, (80.0, 40.0, 0), [(69.9, 40.0, 0)], levL, levR, maxd=10.0)[0] < 0
    levL2, levR2, _ = _scene(shift=2)
    assert _stereo1(oracle, (80.0, 40.0, 0), [(80.0, 40.0, 0)], levL2, levR2)[0] >= 0
    assert _stereo1(oracle, (80.0, 40.0, 0), [(80.1, 40.0, 0)], levL2, levR2)[0] < 0
    # accepted iff 0 <= disp < maxD: disparity ~6 against maxD 5.5 / 6.5
    assert _stereo1(oracle, (80.0, 40.0, 0), [(75.0, 40.0, 0)], levL, levR, maxd=5.5)[0] < 0
    assert _stereo1(oracle, (80.0, 40.0, 0), [(75.0, 40.0, 0)], levL, levR, maxd=6.5)[0] >= 0
    # disp == 0 (zero shift, a patch neighbourhood mirrored about its centre column: delta = 0): uR = uL - 0.01f
    levL3, _, rng = _scene(shift=0, noise=False)
    for L in levL3:
        L[:, 80 - 16:80][:, ::-1] = L[:, 81:81 + 16]
    levR3 = [L.copy() for L in levL3]
    levR3[0][60:, :] = np.clip(np.roll(levL3[0][60:, :], -4, axis=1).astype(int) + rng.integers(-3, 4, (H - 60, W)), 0, 255).astype(np.uint8)
    dL = rng.integers(0, 256, (2, 32), dtype=np.uint8)
    kL = _kps(oracle, [(80.0, 40.0, 0), (50.0, 80.0, 0)])       # the second keypoint (noisy rows, disparity 4) keeps the median above 0
    kR = _kps(oracle, [(80.0, 40.0, 0), (46.0, 80.0, 0)])
    uR, sd, _ = M.stereo(kL, dL, kR, dL, levL3, levR3, 30.0)
    assert sd[0] == 0 and sd[1] > 0
    assert uR[0] == F(F(80.0) - F(0.01)) and uR[1] >= 0


def test_th_stereo_is_strict(oracle):
    levL, levR, _ = _scene()
    d = np.random.default_rng(2).integers(0, 256, (1, 32), dtype=np.uint8)       # _stereo1's left descriptor
    for bits, ok in [(74, True), (75, False)]:
        uR, _ = _stereo1(oracle, (80.0, 40.0, 0), [(74.0, 40.0, 0)], levL, levR, dR=_flip(d[0], bits)[None, :])
        assert (uR >= 0) == ok, bits
    assert _stereo1(oracle, (80.0, 40.0, 0), [(74.0, 40.0, 0)], levL, levR, dR=_flip(d[0], 75)[None, :], th=76)[0] >= 0


def test_first_minimum_ties(oracle):
    levL, levR, rng = _scene()
    # Hamming tie: the lowest j wins -- one candidate's slide finds the true column, the other's leaves the level (sr - 10 < 0)
    good, far = (74.0, 40.0, 0), (9.0, 40.0, 0)
    assert _stereo1(oracle, (80.0, 40.0, 0), [good, far], levL, levR, maxd=100.0)[0] >= 0
    assert _stereo1(oracle, (80.0, 40.0, 0), [far, good], levL, levR, maxd=100.0)[0] < 0
    # SAD tie: rows 20..59 repeat every 4 columns (zero SAD at k = -3, 1, 5 around sr = 75): the first one wins
    base = rng.integers(0, 256, (H, 4), dtype=np.uint8)
    L = levL[0].copy()
    L[20:60, :] = np.tile(base, (1, W // 4))[20:60, :]
    R = L.copy()
    R[60:, :] = levR[0][60:, :]
    lL, lR = [L] + levL[1:], [R] + levR[1:]
    dL = rng.integers(0, 256, (2, 32), dtype=np.uint8)
    kL = _kps(oracle, [(80.0, 40.0, 0), (50.0, 80.0, 0)])       # the second keypoint keeps the median above 0
    kR = _kps(oracle, [(75.0, 40.0, 0), (44.0, 80.0, 0)])
    uR, sd, _ = M.stereo(kL, dL, kR, dL, lL, lR, 30.0)
    assert sd[0] == 0 and abs(float(uR[0]) - 72.0) <= 0.5 and sd[1] > 0


def test_median_cut_on_known_lists():
    assert M.median_cut([10, 20, 30, 40, 100]).tolist() == [True, True, True, True, False]     # med 30, cut at 63.0000...
    assert M.median_cut([10, 20, 30, 62]).tolist() == [True, True, True, True]                 # even n: element n/2 = 30
    assert M.median_cut([10, 20, 30, 63]).tolist() == [True, True, True, False]                # (1.5f * 1.4f) * 30.0f = 62.999996f
    assert M.median_cut([40, 10]).tolist() == [True, True]                                     # element 1 of (10, 40)
    assert M.median_cut([0, 0, 0]).tolist() == [False, False, False]                           # >= : a zero median drops everything
    assert M.median_cut([]).tolist() == []


def _track_scene(oracle, prev_rows, cur_rows, bits, shift=(3, 2), seed=3, **kw):
    """Stage T on hand-made keypoints: the current image is the previous one moved by `shift`; bits[i][j] = Hamming distance."""
    rng = np.random.default_rng(seed)
    levP = [rng.integers(0, 256, (H, W), dtype=np.uint8) for _ in range(NL)]
    levC = [np.roll(np.roll(L, shift[0], axis=1), shift[1], axis=0) for L in levP]
    kP, kC = _kps(oracle, prev_rows), _kps(oracle, cur_rows)
    _, inv = M.scales()
    patches = np.stack([M.patch_of(kP[i], levP, inv)[3].reshape(-1) for i in range(len(kP))])
    base = rng.integers(0, 256, 32, dtype=np.uint8)
    dC = np.stack([_flip(base, 0) for _ in cur_rows])
    # distances to the FIRST current keypoint are set by flipping leading bits, to the others by flipping trailing bits
    dP = np.stack([base.copy() for _ in prev_rows])
    assert len(cur_rows) <= 2
    for i in range(len(prev_rows)):
        dP[i] = _flip(base, bits[i][0])
    if len(cur_rows) == 2:
        extra = [b[1] - b[0] for b in bits]
        assert len(set(extra)) == 1 and extra[0] >= 0
        for b in range(extra[0]):
            dC[1][31 - b // 8] ^= np.uint8(1 << (b % 8))
    uR = np.array([r[0] - 5.0 for r in prev_rows], F)
    return M.track(kP, dP, uR, patches, kC, dC, levC, **kw)


def test_ratio_test_and_th_track(oracle):
    p, c = (60.0, 40.0, 0), (63.0, 42.0, 0)
    far = (120.0, 70.0, 0)
    assert len(_track_scene(oracle, [p], [c], [[100]])[0]) == 1              # b <= th_track, no second candidate
    assert len(_track_scene(oracle, [p], [c], [[101]])[0]) == 0
    assert len(_track_scene(oracle, [p], [c, far], [[50, 55]])[0]) == 0      # 50 < 0.9f * 55 = 49.5 fails
    assert len(_track_scene(oracle, [p], [c, far], [[50, 56]])[0]) == 1      # 50 < 50.4
    assert len(_track_scene(oracle, [p], [c, far], [[50, 50]], ratio=1.0)[0]) == 0       # strict <
    # radius: the far keypoint is no candidate any more, so there is no second one
    assert len(_track_scene(oracle, [p], [c, far], [[50, 55]], radius=8.0)[0]) == 1
    # octave limit
    assert len(_track_scene(oracle, [p], [(63.0, 42.0, 2)], [[10]])[0]) == 0


def test_uniqueness_tie_breaks(oracle):
    p, c = (60.0, 40.0, 0), (63.0, 42.0, 0)
    out = _track_scene(oracle, [p, p], [c], [[10], [5]])
    assert out[3].tolist() == [1] and out[4].tolist() == [0]                 # the smallest b wins
    out = _track_scene(oracle, [p, p], [c], [[7], [7]])
    assert out[3].tolist() == [0]                                            # ties to the lowest i
    assert out[0].tolist() == [[60.0, 40.0]] and out[1].tolist() == [[55.0, 40.0]]


def test_subpixel_step_and_its_borders(oracle):
    p = (60.0, 40.0, 0)
    out = _track_scene(oracle, [p], [(64.0, 43.0, 0)], [[10]])               # one pixel off in x and y: the step finds (63, 42)
    assert len(out[0]) == 1 and np.abs(out[2][0] - np.array([63.0, 42.0])).max() < 0.5
    assert len(_track_scene(oracle, [p], [(65.0, 42.0, 0)], [[10]])[0]) == 0          # minimum on the 5 x 5 border
    assert len(_track_scene(oracle, [p], [(63.0, 44.0, 0)], [[10]])[0]) == 0
    # the 15 x 15 support must lie inside the level
    assert len(_track_scene(oracle, [(8.0, 40.0, 0)], [(6.0, 42.0, 0)], [[10]], shift=(-2, 2))[0]) == 0
    assert len(_track_scene(oracle, [(9.0, 40.0, 0)], [(7.0, 42.0, 0)], [[10]], shift=(-2, 2))[0]) == 1
    # first minimum in raster order: an image of period 2 ties at every even offset; (-2, -2) comes first and is on the border
    rng = np.random.default_rng(5)
    tile = rng.integers(0, 256, (2, 2), dtype=np.uint8)
    lev = [np.tile(tile, (H // 2, W // 2))] * NL
    kP = _kps(oracle, [p])
    _, inv = M.scales()
    patches = M.patch_of(kP[0], lev, inv)[3].reshape(1, -1)
    d = rng.integers(0, 256, (1, 32), dtype=np.uint8)
    assert len(M.track(kP, d, np.array([55.0], F), patches, kP.copy(), d, lev)[0]) == 0


def test_slide_border_rejects(oracle):
    levL, levR, _ = _scene(shift=6)
    # the true column (74) is five columns from sr: the minimum sits on the slide's border
    assert _stereo1(oracle, (80.0, 40.0, 0), [(79.0, 40.0, 0)], levL, levR)[0] < 0
    assert _stereo1(oracle, (80.0, 40.0, 0), [(78.0, 40.0, 0)], levL, levR)[0] >= 0
    # sr - 10 < 0 and sr + 11 >= w, an invalid patch
    assert _stereo1(oracle, (15.0, 40.0, 0), [(9.0, 40.0, 0)], levL, levR)[0] < 0
    assert _stereo1(oracle, (16.0, 40.0, 0), [(10.0, 40.0, 0)], levL, levR)[0] >= 0
    assert _stereo1(oracle, (80.0, 3.0, 0), [(74.0, 3.0, 0)], levL, levR)[0] < 0        # patch leaves the level (pv < 5)


@pytest.fixture(scope="module")
def seq_832(synth):
    seq = synth.StereoSequence(width=832, height=256, n_frames=3, seed=5)
    return seq, [tuple(x.numpy() for x in seq.render(t)) for t in range(3)]


@pytest.mark.parametrize("which", ["832x256", "small_seq"])
def test_guided_matcher_doubles_the_inliers(oracle, seq_832, small_seq, which):
    """Twin tracks -> oracle.triangulate -> oracle.pnp_ransac against oracle.orb_robust_match through the same two calls: on
    every pair the guided matcher has more tracks and at least twice the inliers (a non-vacuity bar, not a target)."""
    seq, frames = seq_832 if which == "832x256" else small_seq
    P1, P2 = seq.proj()
    K = np.asarray(P1, np.float64).reshape(3, 4)[:, :3]
    fr = [M.frame_stereo(oracle, L, R, float(F(np.asarray(P1).reshape(-1)[0]))) for L, R in frames]
    for t in range(1, len(frames)):
        t1l, t1r, t2l, _, _ = M.pair_tracks(fr[t - 1], fr[t])
        g = oracle.pnp_ransac(oracle.triangulate(P1, P2, t1l, t1r), t2l, K)
        b2l, b1l, b1r = oracle.orb_robust_match(fr[t - 1]["kL"], fr[t - 1]["dL"], fr[t - 1]["kR"], fr[t - 1]["dR"], fr[t]["kL"], fr[t]["dL"])
        b = oracle.pnp_ransac(oracle.triangulate(P1, P2, b1l, b1r), b2l, K)
        print(f"{which} pair {t}: guided {len(t1l)} tracks / {g['n_inliers']} inliers / {g['ransac_iters']} iterations, "
              f"brute {len(b1l)} / {b['n_inliers']} / {b['ransac_iters']}: ratio {g['n_inliers'] / max(b['n_inliers'], 1):.1f}")
        assert len(t1l) > len(b1l)
        assert g["n_inliers"] >= 2 * b["n_inliers"] and b["n_inliers"] > 0
