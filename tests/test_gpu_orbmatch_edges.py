"""GPU tests (-m gpu) of the guided ORB matcher (csrc/orb_match.hip) at the edges tests/test_gpu_orbmatch.py does not reach: the
second LDS chunk of stage S (more than 2048 right keypoints) and indices >= 2048 through stage T, scale tables other than
1.2 / 8 levels, the thresholds as data (th_stereo <, th_track <=, ratio, max_disparity, a radius that leaves one candidate or
none), a median of 0, empty keypoint lists inside a batch, contested winners with equal distances, a frame tracked against
itself, and the matcher behind the ingest stage and in front of the pose refinement stage.

The inputs are tests/_orbmatch_cases.py's; tests/test_orbmatch_ref.py proves on the CPU that each reaches the path it is named
after.  The bar is test_gpu_orbmatch.py's: keypoints, uR, sad, idx_prev, idx_cur and the point lists are the twin's
(tests/_orbmatch_ref.py) BYTE FOR BYTE, poses within TIGHT = 1e-9; no other tolerance exists here."""
import numpy as np
import pytest

import _orbmatch_cases as C
import _orbmatch_ref as M
from test_gpu_orbmatch import TIGHT, _check_records, _check_step, _ctx, relfro

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tc():
    import torch
    assert torch.cuda.is_available()
    return torch


def _pair_ctx(pkg, name, orb=None, **kw):
    h, w = C.frames_of(name)[0][0].shape
    return _ctx(pkg, C.Rig(w, h), w, h, **C.ctx_orb(orb or {}), **kw)


def _eq_stereo(got, fr, what):
    kps, uR, sad = got
    assert len(kps) == len(fr["kL"]), what
    assert kps.tobytes() == fr["kL"].tobytes(), what
    assert uR.tobytes() == fr["uR"].tobytes() and sad.tobytes() == fr["sad"].tobytes(), what


def _eq_tracks(got, want, what):
    assert len(got) == len(want) == 5
    assert len(got[0]) == len(want[0]), (what, len(got[0]), len(want[0]))
    for g, r, name in zip(got, want, ("t1_left", "t1_right", "t2_left", "idx_prev", "idx_cur")):
        assert g.dtype == r.dtype and g.tobytes() == r.tobytes(), (what, name)


def _stage_both(c, frames, fr, what, tc=None):
    """Stage S of a pair's two frames into stage slots 0 and 1 (the second one from device memory where torch is given)."""
    for t in range(2):
        src = frames[t] if (t == 0 or tc is None) else tuple(tc.from_numpy(x).cuda() for x in frames[t])
        _eq_stereo(c.orb_stereo_frame(*src, slot=t), fr[t], f"{what}, frame {t}")


def _online(c, frames, ref, fr, what, tc=None):
    """The frames through add_frame: every record, the pose, the frame's stage S outputs and the track lists are the twin's."""
    rc, g0 = c.add_frame(*frames[0])
    assert rc == 0 and int(g0["n_cur_kps"]) == len(fr[0]["kL"]), what
    uR, sad = c.get_frame_stereo()
    assert uR.tobytes() == fr[0]["uR"].tobytes() and sad.tobytes() == fr[0]["sad"].tobytes(), what
    for t in range(1, len(frames)):
        src = frames[t] if (t % 2 or tc is None) else tuple(tc.from_numpy(x).cuda() for x in frames[t])
        rc, g = c.add_frame(*src)
        r, pose = ref[t - 1]
        assert rc == r["fail_stage"], (what, t)
        _check_step(g, r)
        assert relfro(c.get_pose(), pose) <= TIGHT, (what, t)
        uR, sad = c.get_frame_stereo()
        assert uR.tobytes() == fr[t]["uR"].tobytes() and sad.tobytes() == fr[t]["sad"].tobytes(), (what, t)
        if r["n_tracked"] > 0:
            t1l, t1r, _, t2l, _ = c.last_tracks()
            assert t1l.tobytes() == r["tracks"][0].tobytes() and t1r.tobytes() == r["tracks"][1].tobytes(), (what, t)
            assert t2l.tobytes() == r["tracks"][2].tobytes(), (what, t)


def _stack(tc, frames):
    return (tc.stack([tc.from_numpy(f[0]) for f in frames]).cuda(), tc.stack([tc.from_numpy(f[1]) for f in frames]).cuda())


# ---- 1. the second chunk of stage S, indices >= 2048 through stage T ----------------------------------------------------------
@pytest.mark.parametrize("orb", [C.CHUNK_ORB, C.CHUNK3_ORB], ids=["one_level", "three_levels"])
def test_chunks_stage_calls(pkg, oracle, tc, orb):
    frames, fr = C.frames_of("chunk"), C.twin(oracle, "chunk", orb)
    want = M.pair_tracks(fr[0], fr[1])
    acc, j = fr[0]["uR"] >= 0, fr[0]["j"]
    print(f"chunk pair, {orb['nlevels']} level(s): {[len(f['kL']) for f in fr]} / {[len(f['kR']) for f in fr]} keypoints, "
          f"{[C.accepted(f) for f in fr]} accepted, {int((acc & (j >= 2048)).sum())} winners with j >= 2048, {len(want[0])} tracks, "
          f"{int((want[4] >= 2048).sum())} with idx_cur >= 2048")
    assert min(len(f["kR"]) for f in fr) > 2048 and (acc & (j >= 2048)).sum() >= 300 and (want[4] >= 2048).sum() >= 100
    c = _pair_ctx(pkg, "chunk", orb)
    c.set_orb_matcher("guided", max_disparity=C.CHUNK_MAXD)
    _stage_both(c, frames, fr, "chunk pair", tc)
    _eq_tracks(c.orb_track_frames(0, 1), want, "chunk pair")
    c.close()


@pytest.fixture(scope="module")
def chunk_ref(pkg, oracle):
    """The twin's record of the chunk pair through the fused step (one-level extractor)."""
    frames = C.frames_of("chunk")
    h, w = frames[0][0].shape
    rig = C.Rig(w, h)
    ref, fr = M.ref_sequence(oracle, rig, frames, orb=C.CHUNK_ORB, max_disparity=C.CHUNK_MAXD)
    assert fr[1]["uR"].tobytes() == C.twin(oracle, "chunk", C.CHUNK_ORB)[1]["uR"].tobytes()
    return rig, ref, fr


def test_chunks_fused(pkg, oracle, tc, chunk_ref):
    rig, ref, fr = chunk_ref
    frames = C.frames_of("chunk")
    r = ref[0][0]
    print(f"chunk pair fused: {r['n_tracked']} tracks, {r['n_inliers']} inliers, ok {r['ok']} fail_stage {r['fail_stage']}")
    assert r["n_tracked"] >= 1000 and r["fail_stage"] != 2
    h, w = frames[0][0].shape
    c = _ctx(pkg, rig, w, h, max_batch=2, **C.ctx_orb(C.CHUNK_ORB))
    c.set_orb_matcher("guided", max_disparity=C.CHUNK_MAXD)
    _online(c, frames, ref, fr, "chunk pair, add_frame")
    # one batch of device frames: level 0 is read in place
    c.reset()
    L, R = _stack(tc, frames)
    res = c.track_batch(L, R)
    _check_records(res, ref)
    t1l, t1r, _, t2l, _ = c.batch_tracks(0)
    assert t1l.tobytes() == r["tracks"][0].tobytes() and t1r.tobytes() == r["tracks"][1].tobytes()
    assert t2l.tobytes() == r["tracks"][2].tobytes()
    c.close()


# ---- 2. scale tables ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(C.SCALE_ORBS))
def test_scale_tables(pkg, oracle, tc, name):
    orb = C.SCALE_ORBS[name]
    frames, fr = C.frames_of("shift"), C.twin(oracle, "shift", orb)
    want = M.pair_tracks(fr[0], fr[1])
    print(f"scale table {name}: {[len(f['kL']) for f in fr]} keypoints on octaves {np.bincount(fr[0]['kL']['octave']).tolist()}, "
          f"{[C.accepted(f) for f in fr]} accepted, {len(want[0])} tracks")
    assert C.accepted(fr[0]) >= 100 and len(want[0]) >= 50
    c = _pair_ctx(pkg, "shift", orb)
    c.set_orb_matcher("guided", max_disparity=300.0)
    _stage_both(c, frames, fr, f"scale table {name}", tc)
    _eq_tracks(c.orb_track_frames(0, 1), want, f"scale table {name}")
    c.close()


def test_scale_table_fused(pkg, oracle, tc):
    """Frames 0, 1, 0 of the shift pair through add_frame with the 1.5 / 5-level extractor: two pairs."""
    orb = C.SCALE_ORBS["5x1.5"]
    two = C.frames_of("shift")
    frames = [two[0], two[1], two[0]]
    h, w = frames[0][0].shape
    rig = C.Rig(w, h)
    ref, fr = M.ref_sequence(oracle, rig, frames, orb=orb, max_disparity=300.0)
    print(f"scale table 5x1.5 fused: {[(r['ok'], r['fail_stage'], r['n_tracked'], r['n_inliers']) for r, _ in ref]}")
    assert all(r["n_tracked"] >= 50 for r, _ in ref)
    c = _ctx(pkg, rig, w, h, **C.ctx_orb(orb))
    c.set_orb_matcher("guided", max_disparity=300.0)
    _online(c, frames, ref, fr, "scale table 5x1.5, add_frame", tc)
    c.close()


# ---- 3. the thresholds as data -----------------------------------------------------------------------------------------------
def _stereo_boundary(oracle):
    fr = C.twin(oracle, "shift")
    bs = int(C.stereo_best(fr[0]).max())
    return [(bs, 300.0), (bs + 1, 300.0)]


@pytest.mark.parametrize("k", range(len(C.STEREO_SETTINGS) + 2))
def test_stage_s_thresholds(pkg, oracle, tc, k):
    """th_stereo and max_disparity at C.STEREO_SETTINGS, then th_stereo = b* and b* + 1 for the largest accepted distance b* of
    the default run: the kernel's `<` against a `<=` differs exactly there."""
    th, md = (C.STEREO_SETTINGS + _stereo_boundary(oracle))[k]
    frames, base = C.frames_of("shift"), C.twin(oracle, "shift")
    want = C.cached(("restereo", th, md), lambda: C.restereo(base[0], md, th))
    print(f"stage S th_stereo {th} max_disparity {md}: {len(want['kL'])} keypoints, twin accepts {C.accepted(want)} (default {C.accepted(base[0])})")
    if k >= len(C.STEREO_SETTINGS):
        other = C.restereo(base[0], md, th + (1 if k == len(C.STEREO_SETTINGS) else -1))
        assert C.accepted(other) != C.accepted(want)
    c = _pair_ctx(pkg, "shift")
    c.set_orb_matcher("guided", th_stereo=th, max_disparity=md)
    _eq_stereo(c.orb_stereo_frame(*frames[0]), want, f"th_stereo {th} max_disparity {md}")
    c.close()


def _track_boundary(oracle):
    fr = C.twin(oracle, "shift")
    bt = int(C.track_best(fr[0], fr[1], M.pair_tracks(fr[0], fr[1])).max())
    return [dict(th_track=bt - 1), dict(th_track=bt)]


@pytest.mark.parametrize("k", range(len(C.TRACK_SETTINGS) + 2))
def test_stage_t_thresholds(pkg, oracle, tc, k):
    """th_track, ratio and radius at C.TRACK_SETTINGS (radius 3: a keypoint with one candidate skips the ratio test; radius
    0.5: no candidate), then th_track = b* - 1 and b* for the largest distance b* of the default tracks (`<=` against `<`)."""
    kw = (C.TRACK_SETTINGS + _track_boundary(oracle))[k]
    frames, fr = C.frames_of("shift"), C.twin(oracle, "shift")
    want = M.pair_tracks(fr[0], fr[1], **kw)
    print(f"stage T {kw}: {len(want[0])} tracks")
    if k == len(C.TRACK_SETTINGS):
        assert len(want[0]) < len(M.pair_tracks(fr[0], fr[1], th_track=kw["th_track"] + 1)[0])
    c = _pair_ctx(pkg, "shift")
    c.set_orb_matcher("guided", max_disparity=300.0, **kw)
    _stage_both(c, frames, fr, f"stage T {kw}")
    _eq_tracks(c.orb_track_frames(0, 1), want, f"stage T {kw}")
    c.close()


# ---- 4. a median of 0 -------------------------------------------------------------------------------------------------------
def test_median_zero_cuts_every_match(pkg, oracle, tc):
    left, right = C.median_pair()
    fr = M.frame_stereo(oracle, left, right, 300.0, orb=dict(nlevels=1))
    assert len(fr["kL"]) >= 1000 and C.accepted(fr) == 0
    c = pkg.Context(416, 128, device=0, track_mode=pkg.MODE_ORB, orb_nlevels=1)
    c.set_orb_matcher("guided", max_disparity=300.0)
    for slot in range(2):
        kps, uR, sad = c.orb_stereo_frame(left, right, slot=slot)
        print(f"identical pair, one level, slot {slot}: {len(kps)} keypoints, {int((uR >= 0).sum())} accepted")
        assert kps.tobytes() == fr["kL"].tobytes()
        assert (uR == np.float32(-1.0)).all() and (sad == -1).all() and len(uR) == len(kps) == len(sad)
        assert uR.tobytes() == fr["uR"].tobytes() and sad.tobytes() == fr["sad"].tobytes()
    got = c.orb_track_frames(0, 1)
    assert all(len(g) == 0 for g in got)
    c.close()


def test_zero_disparity_clamp(pkg, oracle, tc):
    left, right = C.clamp_pair()
    fr = M.frame_stereo(oracle, left, right, 300.0)
    clamped = (fr["uR"] >= 0) & (fr["uR"] == (fr["kL"]["x"] - np.float32(0.01)).astype(np.float32))
    print(f"clamp pair: {len(fr['kL'])} keypoints, {C.accepted(fr)} accepted, {int(clamped.sum())} clamped")
    assert clamped.sum() >= 1
    c = pkg.Context(416, 128, device=0, track_mode=pkg.MODE_ORB)
    c.set_orb_matcher("guided", max_disparity=300.0)
    _eq_stereo(c.orb_stereo_frame(left, right), fr, "clamp pair")
    c.close()


# ---- 5. empty lists inside a batch --------------------------------------------------------------------------------------------
def test_empty_frames_in_a_batch(pkg, oracle, tc, small_seq):
    seq, four = small_seq
    frames = C.flat_sequence(four)
    ref, fr = C.flat_ref(oracle, seq, four)
    recs = [(r["ok"], r["fail_stage"], r["n_prev_kps"], r["n_cur_kps"], r["n_tracked"]) for r, _ in ref]
    print(f"flat sequence: records {recs}, accepted {[C.accepted(f) for f in fr]}")
    assert [x[1] for x in recs] == [0, 2, 2, 0, 2] and len(fr[2]["kL"]) == 0 and len(fr[4]["kR"]) == 0 and len(fr[4]["kL"]) > 1000
    h, w = four[0][0].shape
    c = _ctx(pkg, seq, w, h, max_batch=5)
    c.set_orb_matcher("guided")
    L, R = _stack(tc, frames)
    res = c.track_batch(L, R)
    assert len(res) == 5
    _check_records(res, ref)
    for p in (0, 3):
        t1l, t1r, _, t2l, _ = c.batch_tracks(p)
        want = ref[p][0]["tracks"]
        assert t1l.tobytes() == want[0].tobytes() and t1r.tobytes() == want[1].tobytes() and t2l.tobytes() == want[2].tobytes()
    # overlap mode gives the same records
    c.set_overlap(True)
    dres = tc.zeros((5, pkg.STEP_DTYPE.itemsize), dtype=tc.uint8, device="cuda")
    c.track_batch(L, R, results=dres)
    c.track_batch(L, R, results=dres)
    c.sync()
    assert np.frombuffer(dres.cpu().numpy().tobytes(), dtype=pkg.STEP_DTYPE).tobytes() == res.tobytes()
    c.set_overlap(False)
    # one stream of a stream set
    c.streams_create(1)
    r = c.streams_step([0], [frames[0][0]], [frames[0][1]])
    assert int(r[0]["ok"]) == 1 and int(r[0]["n_prev_kps"]) == 0
    for t in range(1, 6):
        r = c.streams_step([0], [frames[t][0]], [frames[t][1]])
        _check_step(r[0], ref[t - 1][0])
        assert relfro(r[0]["pose"].reshape(4, 4), ref[t - 1][1]) <= TIGHT, t
    c.close()
    # frame by frame: the stage S outputs of every frame, the empty ones too
    c = _ctx(pkg, seq, w, h)
    c.set_orb_matcher("guided")
    _online(c, frames, ref, fr, "flat sequence, add_frame", tc)
    c.close()


# ---- 6. contested winners and ties in stage T -----------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(ratio=0.9), dict(ratio=1.0), dict(radius=20.0, ratio=1.0)], ids=["0.9", "1.0", "radius20"])
def test_contention_and_ties(pkg, oracle, tc, kw):
    frames, fr = C.frames_of("tiled"), C.twin(oracle, "tiled")
    want = M.pair_tracks(fr[0], fr[1], **kw)
    n, ties = C.contested(fr[0], fr[1], **kw)
    print(f"tiled pair {kw}: {[len(f['kL']) for f in fr]} keypoints, {[C.accepted(f) for f in fr]} accepted, {len(want[0])} tracks, "
          f"{n} contested current keypoints, {ties} at equal distance")
    assert len(want[0]) >= 300 and (kw.get("radius") or (n >= 20 and ties >= 10))
    c = _pair_ctx(pkg, "tiled")
    c.set_orb_matcher("guided", max_disparity=C.TILED_MAXD, **kw)
    _stage_both(c, frames, fr, f"tiled pair {kw}")
    _eq_tracks(c.orb_track_frames(0, 1), want, f"tiled pair {kw}")
    c.close()


# ---- 7. a frame against itself ----------------------------------------------------------------------------------------------
def test_self_tracking(pkg, oracle, tc):
    """Every accepted keypoint finds itself at distance 0: the 25 SADs have their minimum (0) at the centre, and where both
    neighbours are equal the parabola's denominator can be 0."""
    frame, fr = C.frames_of("shift")[0], C.twin(oracle, "shift")[0]
    want = M.pair_tracks(fr, fr)
    assert len(want[0]) == C.accepted(fr) >= 400
    c = _pair_ctx(pkg, "shift")
    c.set_orb_matcher("guided", max_disparity=300.0)
    _stage_both(c, [frame, frame], [fr, fr], "self")
    got = c.orb_track_frames(0, 1)
    print(f"self-tracking: {len(got[0])} of {C.accepted(fr)} accepted keypoints track")
    assert np.array_equal(got[3], got[4]) and len(got[0]) == C.accepted(fr)
    _eq_tracks(got, want, "self")
    c.close()


# ---- 8. behind the ingest stage ------------------------------------------------------------------------------------------------
def test_guided_behind_ingest(pkg, synth, tc):
    """A guided context with an ingest stage (832 x 256 -> 416 x 128, nearest, 0.5) against a plain guided context fed the
    resized frames: records and track lists byte for byte, stage S outputs equal."""
    from test_gpu_ingest import ORB_KW, _pair, _render, _same, _same_tracks, _small
    seq, frames = _render(synth, tc, 832, 256, 4)
    small = _small(frames, 416, 128, "nearest", 0.5)
    a, b = _pair(pkg, seq, 832, 256, 416, 128, "nearest", 0.5, track_mode=pkg.MODE_ORB, **ORB_KW)
    a.set_orb_matcher("guided")
    b.set_orb_matcher("guided")
    for t, (fr, sm) in enumerate(zip(frames, small)):
        src = fr if t % 2 == 0 else tuple(tc.from_numpy(x).cuda() for x in fr)
        rca, ga = a.ingest_add_frame(*src)
        rcb, gb = b.add_frame(*sm)
        assert rca == rcb == 0
        _same(ga, gb, f"frame {t}")
        _same_tracks(a.last_tracks(), b.last_tracks(), f"tracks of frame {t}")
        sa, sb = a.get_frame_stereo(), b.get_frame_stereo()
        assert sa[0].tobytes() == sb[0].tobytes() and sa[1].tobytes() == sb[1].tobytes()
        print(f"ingest frame {t}: {int(ga['n_cur_kps'])} keypoints, {int((sa[0] >= 0).sum())} accepted, {int(ga['n_tracked'])} tracks")
        assert (sa[0] >= 0).sum() >= 300
        assert int(ga["ok"]) == 1 and (t == 0 or int(ga["n_tracked"]) >= 100)
        assert np.array_equal(a.get_pose(), b.get_pose())
    a.close()
    b.close()


# ---- 9. in front of the pose refinement stage ----------------------------------------------------------------------------------
def test_guided_with_pose_refine(pkg, oracle, tc, small_seq):
    """set_orb_matcher("guided") + set_pose_refine("reproj") through add_frame: the refinement of the twin's tracks from the
    oracle's RANSAC pose, as tests/_refine_ref.py computes it."""
    import _refine_ref as RR
    from test_gpu_refine import _check_result, _gates
    seq, frames = small_seq
    ref, fr = C.small_ref(oracle, seq, frames)
    P1, P2 = (np.asarray(p, np.float64).reshape(3, 4) for p in seq.proj())
    h, w = frames[0][0].shape
    c = _ctx(pkg, seq, w, h)
    c.set_orb_matcher("guided")
    c.set_pose_refine("reproj")
    rc, _ = c.add_frame(*frames[0])
    assert rc == 0
    pose = np.eye(4)
    for t in range(1, 4):
        r, _ = ref[t - 1]
        what = f"guided + reproj, pair {t}"
        assert r["ok"] == 1 and r["n_tracked"] >= 100
        _, g = c.add_frame(*frames[t])
        rr = c.refine_result(0)
        tracks = c.last_tracks()
        m = r["n_tracked"]
        # the matcher's lists and the RANSAC stage are untouched by the refinement
        assert int(g["n_tracked"]) == m and int(g["n_inliers"]) == r["n_inliers"], what
        assert tracks[0].tobytes() == r["tracks"][0].tobytes() and tracks[1].tobytes() == r["tracks"][1].tobytes(), what
        assert tracks[3].tobytes() == r["tracks"][2].tobytes(), what
        assert relfro(rr["pnp_tvec"], r["tvec"]) <= TIGHT, what                   # the stage started from the oracle's RANSAC pose
        X = oracle.triangulate(P1, P2, r["tracks"][0], r["tracks"][1])
        run = RR.refine(X, r["tracks"][2], None, P1, P2, r["R"], r["tvec"])     # (ORB mode: one view, as test_gpu_refine._reference)
        print(f"{what}: {m} tracks, {r['n_inliers']} inliers, reference status {run['status']} active {run['n_active']}, "
              f"margins {[round(e['margin'], 3) for e in run['log']]}")
        assert run["status"] == RR.APPLIED and all(e["margin"] >= 1e-6 for e in run["log"]), what     # no flag hangs on a last bit
        _check_result(rr, run, m, 2, what)
        R, tv = run["R"], run["t"]
        fail = _gates(c.cfg, R, tv, r["n_inliers"], m)
        assert int(g["fail_stage"]) == fail and int(g["ok"]) == (fail == 0), what
        assert np.abs(g["tvec"] - tv).max() <= TIGHT and np.abs(g["R"].reshape(3, 3) - R).max() <= TIGHT, what
        if fail == 0:
            T = np.eye(4)
            T[:3, :3], T[:3, 3] = R.T, -R.T @ tv
            pose = pose @ T
        assert np.abs(g["pose"].reshape(4, 4) - pose).max() <= TIGHT, what
    c.close()
