"""GPU tests (-m gpu) of the guided ORB matcher (svo_set_orb_matcher, csrc/orb_match.hip) against its numpy twin
tests/_orbmatch_ref.py: stage S (epipolar stereo + SAD slide + median cut), stage T (ratio-test match + sub-pixel step), the
fused entry points, the off switch, the setter's rules and the failure exits.  Everything the matcher computes is integer or
float32 with one rounding per operation: the bar for keypoints, uR, sad, indices and point lists is BIT-EXACT; poses hold the
tolerances of test_gpu_parity_orb.py."""
import numpy as np
import pytest

import _orbmatch_ref as M
from conftest import rand_image

pytestmark = pytest.mark.gpu

POSE_TOL, TIGHT = 1e-4, 1e-9
KW = dict(min_move2=0.05 ** 2, max_move2=10.0 ** 2)


def relfro(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(np.asarray(b)), 1e-300)


@pytest.fixture(scope="module")
def tc():
    import torch
    assert torch.cuda.is_available()
    return torch


def _maxd(P1):
    return float(np.float32(np.asarray(P1, np.float64).reshape(-1)[0]))


@pytest.fixture(scope="module")
def ref_small(oracle, small_seq):
    """The twin's records of small_seq (3 pairs) and its per-frame stage S; computed once, never modified."""
    seq, frames = small_seq
    return M.ref_sequence(oracle, seq, frames)


@pytest.fixture(scope="module")
def ref_odd(oracle, synth):
    """Stage S of two 333 x 201 frames (odd sizes: every level has an odd width or height somewhere)."""
    seq = synth.StereoSequence(width=333, height=201, n_frames=2, seed=5)
    frames = [tuple(x.numpy() for x in seq.render(t)) for t in range(2)]
    return seq, frames, [M.frame_stereo(oracle, L, R, _maxd(seq.proj()[0])) for L, R in frames]


def _ctx(pkg, seq, w, h, **kw):
    P1, P2 = seq.proj()
    return pkg.Context(w, h, device=0, P1=P1, P2=P2, track_mode=pkg.MODE_ORB, **KW, **kw)


def _cases(small_seq, ref_small, ref_odd):
    seq, frames = small_seq
    return [(seq, frames, ref_small[1]), ref_odd]


def test_stage_s_parity(pkg, oracle, tc, small_seq, ref_small, ref_odd):
    for seq, frames, fr in _cases(small_seq, ref_small, ref_odd):
        h, w = frames[0][0].shape
        c = _ctx(pkg, seq, w, h)
        for t in range(2):
            src = frames[t] if t == 0 else tuple(tc.from_numpy(x).cuda() for x in frames[t])       # host and device images
            kps, uR, sad = c.orb_stereo_frame(*src, slot=t)
            n_acc = int((fr[t]["uR"] >= 0).sum())
            print(f"{w}x{h} frame {t}: {len(kps)} keypoints, twin accepts {n_acc}")
            assert n_acc >= 300
            assert kps.tobytes() == fr[t]["kL"].tobytes()
            assert uR.tobytes() == fr[t]["uR"].tobytes() and sad.tobytes() == fr[t]["sad"].tobytes()
        c.close()


def test_stage_s_exact_ties(pkg, oracle, tc):
    """A frame pair tiled from one 96-pixel-wide block: descriptors and patches repeat every 96 pixels, so Hamming distances
    and SADs tie exactly -- the lowest j and the first minimum must win."""
    block = rand_image(128, 96, 21)
    big = np.tile(block, (1, 6))
    left, right = np.ascontiguousarray(big[:, :416]), np.ascontiguousarray(big[:, 9:425])
    c = pkg.Context(416, 128, device=0, track_mode=pkg.MODE_ORB)
    kps, uR, sad = c.orb_stereo_frame(left, right)
    fr = M.frame_stereo(oracle, left, right, _maxd(c.cfg.P1))
    print(f"tiled pair: {len(kps)} keypoints, twin accepts {int((fr['uR'] >= 0).sum())}")
    assert len(kps) > 100 and (fr["uR"] >= 0).sum() > 0
    assert kps.tobytes() == fr["kL"].tobytes()
    assert uR.tobytes() == fr["uR"].tobytes() and sad.tobytes() == fr["sad"].tobytes()
    c.close()


@pytest.mark.parametrize("radius,ratio", [(0.0, 0.9), (0.0, 1.0), (64.0, 0.9), (64.0, 1.0)])
def test_stage_t_parity(pkg, oracle, tc, small_seq, ref_small, ref_odd, radius, ratio):
    for seq, frames, fr in _cases(small_seq, ref_small, ref_odd):
        h, w = frames[0][0].shape
        c = _ctx(pkg, seq, w, h)
        c.set_orb_matcher("guided", ratio=ratio, radius=radius)
        for t in range(2):
            c.orb_stereo_frame(*frames[t], slot=t)
        got = c.orb_track_frames(0, 1)
        want = M.pair_tracks(fr[0], fr[1], ratio=ratio, radius=radius)
        print(f"{w}x{h} radius {radius} ratio {ratio}: {len(want[0])} tracks")
        assert len(want[0]) >= 100
        assert len(got[0]) == len(want[0])
        for g, r in zip(got, want):
            assert g.tobytes() == r.tobytes()
        c.close()


def _check_step(g, r):
    assert int(g["ok"]) == r["ok"] and int(g["fail_stage"]) == r["fail_stage"]
    assert int(g["n_prev_kps"]) == r["n_prev_kps"] and int(g["n_cur_kps"]) == r["n_cur_kps"]
    assert int(g["n_tracked"]) == r["n_tracked"]
    if r["fail_stage"] != 2:
        assert int(g["n_inliers"]) == r["n_inliers"]
        Tg = np.hstack([g["R"].reshape(3, 3), g["tvec"][:, None]])
        Tr = np.hstack([r["R"], r["tvec"][:, None]])
        assert relfro(Tg, Tr) <= POSE_TOL and relfro(Tg, Tr) <= TIGHT


def _check_records(res, ref):
    for p in range(len(ref)):
        _check_step(res[p], ref[p][0])
        assert relfro(res[p]["pose"].reshape(4, 4), ref[p][1]) <= TIGHT


def test_fused_online_parity(pkg, oracle, tc, small_seq, ref_small):
    seq, frames = small_seq
    ref, fr = ref_small
    assert all(r["ok"] for r, _ in ref) and min(r["n_tracked"] for r, _ in ref) >= 100
    h, w = frames[0][0].shape
    c = _ctx(pkg, seq, w, h)
    c.set_orb_matcher("guided")
    rc, g0 = c.add_frame(*frames[0])
    assert rc == 0 and g0["n_cur_kps"] == len(fr[0]["kL"])
    for t in range(1, 4):
        src = frames[t] if t % 2 else tuple(tc.from_numpy(x).cuda() for x in frames[t])
        rc, g = c.add_frame(*src)
        r, pose = ref[t - 1]
        assert rc == 0
        _check_step(g, r)
        assert relfro(c.get_pose(), pose) <= TIGHT
        uR, sad = c.get_frame_stereo()
        assert uR.tobytes() == fr[t]["uR"].tobytes() and sad.tobytes() == fr[t]["sad"].tobytes()
        t1l, t1r, _, t2l, _ = c.last_tracks()
        assert t1l.tobytes() == r["tracks"][0].tobytes() and t1r.tobytes() == r["tracks"][1].tobytes()
        assert t2l.tobytes() == r["tracks"][2].tobytes()
    c.close()


def test_fused_batch_overlap_async_parity(pkg, oracle, tc, small_seq, ref_small):
    seq, frames = small_seq
    ref, _ = ref_small
    h, w = frames[0][0].shape
    c = _ctx(pkg, seq, w, h, max_batch=3)
    c.set_orb_matcher("guided")
    L = tc.stack([tc.from_numpy(f[0]) for f in frames]).cuda()
    R = tc.stack([tc.from_numpy(f[1]) for f in frames]).cuda()
    res = c.track_batch(L, R)
    _check_records(res, ref)
    # overlap mode gives the same records
    c.set_overlap(True)
    dres = tc.zeros((3, pkg.STEP_DTYPE.itemsize), dtype=tc.uint8, device="cuda")
    c.track_batch(L, R, results=dres)
    c.track_batch(L, R, results=dres)
    c.sync()
    assert np.frombuffer(dres.cpu().numpy().tobytes(), dtype=pkg.STEP_DTYPE).tobytes() == res.tobytes()
    c.set_overlap(False)
    # host frame buffers: frames 0, 1, then 1 (carried on the device), 2, 3
    hl, hr = c.host_frames(2), c.host_frames(2)
    for k in range(2):
        hl[k, :, :w], hr[k, :, :w] = frames[k]
    c.upload_frames(0, hl, hr)
    c.wait_upload(0)
    c.track_uploaded_async(0, 2)
    for k in range(2):
        hl[k, :, :w], hr[k, :, :w] = frames[2 + k]
    c.upload_frames(1, hl, hr, first_slot=1)
    c.wait_upload(1)
    c.track_uploaded_async(1, 3, continue_chain=True, carry_frame=True)
    got = np.concatenate([c.collect_results(1), c.collect_results(2)])
    _check_records(got, ref)
    assert got.tobytes() == res.tobytes()
    c.host_free(hl); c.host_free(hr)
    c.close()


def test_fused_streams_parity(pkg, oracle, tc, small_seq, ref_small):
    """Two streams fed the same sequence, one a frame behind the other: every record is the twin's."""
    seq, frames = small_seq
    ref, _ = ref_small
    h, w = frames[0][0].shape
    c = _ctx(pkg, seq, w, h, max_batch=3)
    c.set_orb_matcher("guided")
    c.streams_create(2)
    r = c.streams_step([1], [frames[0][0]], [frames[0][1]])
    assert int(r[0]["ok"]) == 1
    for t in range(1, 4):
        r = c.streams_step([0, 1], [frames[t - 1][0], frames[t][0]], [frames[t - 1][1], frames[t][1]])
        _check_step(r[1], ref[t - 1][0])
        assert relfro(r[1]["pose"].reshape(4, 4), ref[t - 1][1]) <= TIGHT
        if t >= 2:
            _check_step(r[0], ref[t - 2][0])
            assert relfro(r[0]["pose"].reshape(4, 4), ref[t - 2][1]) <= TIGHT
    c.close()


def test_fused_kitti_size_pair(pkg, oracle, tc, synth):
    seq = synth.StereoSequence(width=1241, height=376, n_frames=2, seed=20200710)
    frames = [tuple(x.numpy() for x in seq.render(t)) for t in range(2)]
    ref, fr = M.ref_sequence(oracle, seq, frames)
    print(f"1241x376: {ref[0][0]['n_tracked']} tracks, {ref[0][0]['n_inliers']} inliers, {ref[0][0].get('ransac_iters')} RANSAC iterations")
    assert ref[0][0]["ok"] and ref[0][0]["n_tracked"] >= 100
    c = _ctx(pkg, seq, 1241, 376)
    c.set_orb_matcher("guided")
    c.add_frame(*frames[0])
    rc, g = c.add_frame(*frames[1])
    assert rc == 0
    _check_step(g, ref[0][0])
    assert relfro(c.get_pose(), ref[0][1]) <= TIGHT
    uR, sad = c.get_frame_stereo()
    assert uR.tobytes() == fr[1]["uR"].tobytes() and sad.tobytes() == fr[1]["sad"].tobytes()
    c.close()


def test_off_means_off(pkg, tc, small_seq):
    """guided -> brute and a reset: the records are byte for byte a fresh context's."""
    seq, frames = small_seq
    h, w = frames[0][0].shape

    def run(c):
        out = []
        for f in frames:
            out.append(c.add_frame(*f)[1].tobytes())
        return out

    fresh = _ctx(pkg, seq, w, h)
    want = run(fresh)
    fresh.close()
    c = _ctx(pkg, seq, w, h)
    c.set_orb_matcher("guided")
    guided = run(c)
    assert guided != want
    c.set_orb_matcher("brute")
    c.reset()
    assert run(c) == want
    c.close()


def test_setter_rules(pkg, tc):
    lk = pkg.Context(416, 128, device=0)
    with pytest.raises(pkg.SvoError):
        lk.set_orb_matcher("guided")
    lk.close()
    c = pkg.Context(416, 128, device=0, track_mode=pkg.MODE_ORB)
    assert c.get_orb_matcher() == ("brute", 75, 100, 0.9, 0.0, 0.0)
    c.set_orb_matcher("guided", th_stereo=60, th_track=90, ratio=0.8, radius=48.0, max_disparity=200.0)
    want = ("guided", 60, 90, 0.8, 48.0, 200.0)
    assert c.get_orb_matcher() == want
    bad = [dict(mode=2), dict(mode=-1), dict(th_stereo=0), dict(th_stereo=257), dict(th_track=0), dict(th_track=257),
           dict(ratio=0.0), dict(ratio=1.0001), dict(ratio=float("nan")), dict(radius=-1.0), dict(radius=float("inf")),
           dict(radius=float("nan")), dict(max_disparity=-0.5), dict(max_disparity=float("inf")), dict(max_disparity=float("nan"))]
    for kw in bad:
        args = dict(mode=pkg.ORB_MATCHER_GUIDED, th_stereo=75, th_track=100, ratio=0.9, radius=0.0, max_disparity=0.0)
        args.update(kw)
        with pytest.raises(pkg.SvoError):
            c.set_orb_matcher(**args)
        assert c.get_orb_matcher() == want, kw
    c.set_orb_matcher("guided", th_stereo=1, th_track=256, ratio=1.0)
    assert c.get_orb_matcher() == ("guided", 1, 256, 1.0, 0.0, 0.0)
    c.set_orb_matcher("brute")
    assert c.get_orb_matcher()[0] == "brute"
    c.close()


def test_failure_exits(pkg, oracle, tc, small_seq, ref_small):
    seq, frames = small_seq
    ref, _ = ref_small
    h, w = frames[0][0].shape
    flat = np.full((h, w), 60, np.uint8)
    # a flat pair: the same exit as the brute matcher
    stages = []
    for mode in ("brute", "guided"):
        c = _ctx(pkg, seq, w, h)
        c.set_orb_matcher(mode)
        c.add_frame(*frames[0])
        rc, g = c.add_frame(flat, flat)
        stages.append((rc, int(g["fail_stage"]), int(g["n_tracked"]), int(g["n_cur_kps"])))
        rc, g = c.add_frame(*frames[1])
        stages.append((rc, int(g["fail_stage"]), int(g["n_tracked"]), int(g["n_prev_kps"])))
        c.close()
    assert stages[:2] == stages[2:] and stages[0] == (2, 2, 0, 0)
    # a frame stored before the switch has no patches: its pair finds no tracks, the next pair is the twin's
    c = _ctx(pkg, seq, w, h)
    c.add_frame(*frames[0])
    c.set_orb_matcher("guided")
    rc, g = c.add_frame(*frames[1])
    assert rc == 2 and int(g["fail_stage"]) == 2 and int(g["n_tracked"]) == 0
    rc, g = c.add_frame(*frames[2])
    assert rc == 0
    _check_step(g, ref[1][0])
    c.close()
    # the same for a stream's stored frame
    c = _ctx(pkg, seq, w, h, max_batch=1)
    c.streams_create(1)
    c.streams_step([0], [frames[0][0]], [frames[0][1]])
    c.set_orb_matcher("guided")
    r = c.streams_step([0], [frames[1][0]], [frames[1][1]])
    assert int(r[0]["fail_stage"]) == 2 and int(r[0]["n_tracked"]) == 0
    r = c.streams_step([0], [frames[2][0]], [frames[2][1]])
    _check_step(r[0], ref[1][0])
    c.close()
