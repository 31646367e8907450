"""CPU tests of the guided ORB matcher's reference twin (tests/_orbmatch_ref.py): hand-built cases that pin every rule of
stages S and T as include/svo_abi.h states them, and the quality test -- the matcher must give the pose solver at least twice
the brute-force matcher's inliers on the synthetic sequences (the reason it exists)."""
import numpy as np
import pytest

import _orbmatch_cases as C
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


# ---- the edge cases of tests/_orbmatch_cases.py reach the paths they are named after ------------------------------------------
# (tests/test_gpu_orbmatch_edges.py compares the kernels with the twin on these inputs; a case that never crossed the chunk, never
# tied or never cut anything would pass there and prove nothing.  The floors are conditions, far below the measured counts.)
@pytest.mark.parametrize("orb", [C.CHUNK_ORB, C.CHUNK3_ORB], ids=["one_level", "three_levels"])
def test_chunk_pair_crosses_the_chunk(oracle, orb):
    fr = C.twin(oracle, "chunk", orb)
    j, acc = fr[0]["j"], fr[0]["uR"] >= 0
    lo, hi = C.stereo_candidates(fr[0], C.CHUNK_MAXD)
    tr = M.pair_tracks(fr[0], fr[1])
    print(f"chunk pair, {orb['nlevels']} level(s): {[len(f['kL']) for f in fr]} left / {[len(f['kR']) for f in fr]} right keypoints, "
          f"{[C.accepted(f) for f in fr]} accepted, winners j >= 2048: {int((acc & (j >= 2048)).sum())}, below: {int((acc & (j < 2048)).sum())}, "
          f"candidates in both chunks: {int(((lo > 0) & (hi > 0)).sum())}, {len(tr[0])} tracks, idx_cur >= 2048: "
          f"{int((tr[4] >= 2048).sum())}, idx_prev >= 2048: {int((tr[3] >= 2048).sum())}")
    assert all(len(f["kR"]) > 2048 and len(f["kL"]) > 2048 for f in fr)
    assert (acc & (j >= 2048)).sum() >= 300 and (acc & (j >= 0) & (j < 2048)).sum() >= 300
    assert ((lo > 0) & (hi > 0)).sum() >= 1000
    assert (tr[4] >= 2048).sum() >= 100 and (tr[3] >= 2048).sum() >= 100
    assert fr[0]["scale_factor"] == orb["scale_factor"] and len(fr[0]["levL"]) == orb["nlevels"]


def test_return_j_is_optional_and_names_the_winner(oracle):
    fr = C.twin(oracle, "shift")[0]
    args = (fr["kL"], fr["dL"], fr["kR"], fr["dR"], fr["levL"], fr["levR"], 300.0)
    three, four = M.stereo(*args), M.stereo(*args, return_j=True)
    assert len(three) == 3 and len(four) == 4
    assert all(a.tobytes() == b.tobytes() for a, b in zip(three, four))
    j = four[3]
    assert j.dtype == np.int32 and j.shape == fr["uR"].shape and (j[fr["uR"] >= 0] >= 0).all() and (j == -1).any()
    for i in np.nonzero(j >= 0)[0][:50]:                      # no candidate of a lower index is as close as the winner
        d = M.hamming(fr["dL"][i], fr["dR"])
        band = np.abs(fr["kR"]["y"] - fr["kL"]["y"][i]) <= 1.0          # inside every band (r_j >= 2)
        near = band & (fr["kR"]["x"] <= fr["kL"]["x"][i]) & (fr["kR"]["x"] >= fr["kL"]["x"][i] - 299.0)
        near &= fr["kR"]["octave"] == fr["kL"]["octave"][i]
        assert not (near[:j[i]] & (d[:j[i]] <= d[j[i]])).any() and not (near & (d < d[j[i]])).any()


def test_shift_pair_counts(oracle):
    fr = C.twin(oracle, "shift")
    tr = M.pair_tracks(fr[0], fr[1])
    print(f"shift pair: {[len(f['kL']) for f in fr]} keypoints, {[C.accepted(f) for f in fr]} accepted, {len(tr[0])} tracks")
    assert min(len(f["kL"]) for f in fr) >= 1000 and min(C.accepted(f) for f in fr) >= 400 and len(tr[0]) >= 200
    # a frame against itself: every accepted keypoint tracks, to itself
    me = M.pair_tracks(fr[0], fr[0])
    assert len(me[0]) == C.accepted(fr[0]) and np.array_equal(me[3], me[4])
    assert np.array_equal(me[3], np.nonzero(fr[0]["uR"] >= 0)[0])


@pytest.mark.parametrize("name", sorted(C.SCALE_ORBS))
def test_scale_tables_populate_their_octaves(oracle, name):
    orb = C.SCALE_ORBS[name]
    fr = C.twin(oracle, "shift", orb)
    tr = M.pair_tracks(fr[0], fr[1])
    per = np.bincount(fr[0]["kL"]["octave"], minlength=orb["nlevels"])
    per_acc = np.bincount(fr[0]["kL"]["octave"][fr[0]["uR"] >= 0], minlength=orb["nlevels"])
    print(f"scale table {name}: {len(fr[0]['kL'])} keypoints {per.tolist()}, accepted {per_acc.tolist()}, {len(tr[0])} tracks")
    # (on this image the 1.5 table's extractor keeps keypoints on two octaves, the 1.1 table's on all eight)
    assert (per > 0).sum() >= (8 if name == "8x1.1" else min(orb["nlevels"], 2))
    assert (per_acc > 0).sum() >= min(orb["nlevels"], 2) and C.accepted(fr[0]) >= 100 and len(tr[0]) >= 50
    sc, _ = M.scales(orb.get("scale_factor", 1.2), orb["nlevels"])
    osc, _, _, _ = oracle.orb_setup(orb["nfeatures"], orb.get("scale_factor", 1.2), orb["nlevels"])
    assert sc.tobytes() == osc[:orb["nlevels"]].tobytes()
    if orb["nlevels"] > 1:                                   # the scale table matters: the default one gives other matches
        other = M.stereo(fr[0]["kL"], fr[0]["dL"], fr[0]["kR"], fr[0]["dR"], fr[0]["levL"], fr[0]["levR"], 300.0,
                         scale_factor=1.3 if orb["scale_factor"] != 1.3 else 1.2)
        assert other[0].tobytes() != fr[0]["uR"].tobytes()


def test_tiled_pair_contests_and_ties(oracle):
    fr = C.twin(oracle, "tiled")
    for kw, floor in ((dict(ratio=0.9), 300), (dict(ratio=1.0), 300), (dict(radius=20.0, ratio=1.0), 300)):
        n, ties = C.contested(fr[0], fr[1], **kw)
        tr = M.pair_tracks(fr[0], fr[1], **kw)
        print(f"tiled pair {kw}: {[C.accepted(f) for f in fr]} accepted, {len(tr[0])} tracks, {n} contested current keypoints, {ties} at equal distance")
        assert len(tr[0]) >= floor
        if not kw.get("radius"):
            assert n >= 20 and ties >= 10


def test_small_radius_leaves_one_candidate_or_none(oracle):
    fr = C.twin(oracle, "shift")
    nc = C.track_candidates(fr[0], fr[1], 3.0)
    n3, n05 = len(M.pair_tracks(fr[0], fr[1], radius=3.0)[0]), len(M.pair_tracks(fr[0], fr[1], radius=0.5)[0])
    print(f"radius 3.0: {int((nc == 1).sum())} previous keypoints with one candidate, {int((nc == 0).sum())} with none, {n3} tracks; radius 0.5: {n05}")
    assert (nc == 1).sum() >= 100 and (nc == 0).sum() >= 1 and n3 >= 100 and n05 == 0


def test_threshold_settings_change_the_counts(oracle):
    fr = C.twin(oracle, "shift")
    base = C.accepted(fr[0])
    got = [C.accepted(C.restereo(fr[0], md, th)) for th, md in C.STEREO_SETTINGS]
    print(f"stage S accepted at {C.STEREO_SETTINGS}: {got}, default {base}")
    assert all(g != base for g in got)
    assert got[0] < base < got[1] and got[3] > 0 and got[4] == 0            # th_stereo orders the counts; max_disparity 11 < 12 cuts all
    base_t = len(M.pair_tracks(fr[0], fr[1])[0])
    got_t = [len(M.pair_tracks(fr[0], fr[1], **kw)[0]) for kw in C.TRACK_SETTINGS]
    print(f"stage T tracks at {C.TRACK_SETTINGS}: {got_t}, default {base_t}")
    assert all(g != base_t for g in got_t)
    # the boundary settings: the largest accepted distance b* sits on either side of < (stage S) and <= (stage T)
    bs = int(C.stereo_best(fr[0]).max())
    at, above = C.restereo(fr[0], 300.0, bs), C.restereo(fr[0], 300.0, bs + 1)
    assert bs + 1 <= M.TH_STEREO and above["uR"].tobytes() == fr[0]["uR"].tobytes()
    assert (C.stereo_best(at) < bs).all() and C.accepted(at) != C.accepted(above)
    tr = M.pair_tracks(fr[0], fr[1])
    bt = int(C.track_best(fr[0], fr[1], tr).max())
    below, at = M.pair_tracks(fr[0], fr[1], th_track=bt - 1), M.pair_tracks(fr[0], fr[1], th_track=bt)
    print(f"boundary: stage S b* = {bs}, stage T b* = {bt}: {len(below[0])} / {len(at[0])} tracks")
    assert all(a.tobytes() == b.tobytes() for a, b in zip(at, tr)) and len(below[0]) < len(at[0])


def test_identical_pair_on_one_level_has_median_zero(oracle):
    left, right = C.median_pair()
    fr = M.frame_stereo(oracle, left, right, 300.0, orb=dict(nlevels=1))
    assert len(fr["kL"]) >= 1000 and C.accepted(fr) == 0 and (fr["sad"] == -1).all()
    assert (fr["j"] >= 0).sum() >= 1000                                      # ... although nearly every keypoint finds its partner
    uncut = [M.sad(fr["patches"][i].reshape(11, 11), fr["levR"][0], int(fr["kL"]["x"][i]), int(fr["kL"]["y"][i])) for i in range(20)]
    assert uncut == [0] * 20


def test_clamp_pair_reaches_the_zero_disparity_clamp(oracle):
    fr = M.frame_stereo(oracle, *C.clamp_pair(), 300.0)
    acc = fr["uR"] >= 0
    clamped = acc & (fr["uR"] == (fr["kL"]["x"] - F(0.01)).astype(F))
    print(f"clamp pair: {int(acc.sum())} accepted, {int(clamped.sum())} clamped to uL - 0.01")
    assert acc.sum() >= 300 and clamped.sum() >= 1
    assert (fr["kL"]["x"][clamped] == np.round(fr["kL"]["x"][clamped])).all()


def test_flat_sequence_records(oracle, small_seq):
    seq, frames = small_seq
    ref, fr = C.flat_ref(oracle, seq, frames)
    got = [(r["ok"], r["fail_stage"], r["n_prev_kps"], r["n_cur_kps"], r["n_tracked"]) for r, _ in ref]
    assert got == [(1, 0, 1490, 1503, 330), (0, 2, 1503, 0, 0), (0, 2, 0, 1507, 0), (1, 0, 1507, 1495, 346), (0, 2, 1495, 1495, 0)]
    assert [C.accepted(f) for f in fr] == [905, 911, 0, 939, 0, 953]
    assert len(fr[4]["kL"]) == 1495 and len(fr[4]["kR"]) == 0 and len(fr[2]["kL"]) == 0
    # the pose chain skips the failed pairs
    assert np.array_equal(ref[1][1], ref[0][1]) and np.array_equal(ref[2][1], ref[0][1]) and np.array_equal(ref[4][1], ref[3][1])
    assert not np.array_equal(ref[3][1], ref[0][1])
