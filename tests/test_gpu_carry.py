"""Track carry (-m gpu): svo_set_track_carry / svo_carry_merge against the numpy twin tests/_carry_ref.py, bit for bit.

(a) the stage entry on lists at 512 x 264, HOST and DEVICE; (b) the fused online paths -- svo_add_frame, svo_streams_step,
svo_ingest_add_frame -- on 6 frames of the 416 x 128 synthetic sequence against the CPU oracle's LK step fed the twin's merged
list (records and pose to the bar of test_gpu_buckets._check; tracks, lists, ids and ages byte for byte); (c) the rules of the
switch.  Every test fails without the feature: the symbols do not exist."""
import os
import subprocess

import numpy as np
import pytest

import _carry_ref as CR
import _gftt_ref as G
from _bucket_ref import bucket
from test_gpu_ingest import _render
from test_gpu_parity_fullsize import TIGHT, _K, relfro
from test_host_api import _write_pgm, _write_yaml, host_built   # noqa: F401  (host_built: the fixture that builds host/)

pytestmark = pytest.mark.gpu

W, H = 512, 264


@pytest.fixture(scope="module")
def tc():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def stage_ctx(pkg):
    c = pkg.Context(64, 64, device=0)              # the stage entry is independent of the context's frame size
    yield c
    c.close()


# ---- a. the stage kernel ------------------------------------------------------------------------------------------------------
def _lists(q, det, seed=0, keep=None, ages=None):
    rng = np.random.default_rng(seed)
    q = np.asarray(q, np.float32).reshape(-1, 2)
    det = np.asarray(det, np.float32).reshape(-1, 2)
    n, m = len(q), len(det)
    ids = np.sort(rng.choice(10 * n + 10, n, replace=False)).astype(np.int64)
    return dict(q=q, resp=rng.integers(1, 255, n).astype(np.float32), ids=ids,
                ages=(rng.integers(0, 5, n) if ages is None else np.asarray(ages)).astype(np.int32),
                keep=(np.ones(n) if keep is None else np.asarray(keep)).astype(np.uint8), det=det,
                dresp=rng.integers(1, 255, m).astype(np.float32), next_id=int(ids.max(initial=0)) + 1)


def _random(seed, n, m, keep_rate=0.8):
    rng = np.random.default_rng(seed)
    q = rng.random((n, 2)) * [W + 8, H + 8] - 4                      # some fall outside the image
    det = np.stack([rng.integers(0, W, m), rng.integers(0, H, m)], 1)
    return _lists(q, det, seed, keep=rng.random(n) < keep_rate)


def _boundary():
    one_in = np.nextafter(np.float32(13.0), np.float32(0))
    q = [[10, 10], [13, 10], [10, 20], [one_in, 20], [100, 100], [100, 103], [200, 100], [200, one_in + 90]]
    return _lists(q, [[10, 13], [10, 17.5], [103, 100], [100 + one_in - 10, 103]], 1, ages=np.zeros(8))


def _edges():
    # image corners and borders, and pairs straddling every multiple of 6, 7 and 21 (the cell sizes of min_distance 3 and 20.5 here)
    xs = np.concatenate([[0, 0.25, W - 1, W - 1.25], np.arange(6, W - 1, 6) - 0.5, np.arange(6, W - 1, 6) + 0.5,
                         np.arange(7, W - 1, 7), np.arange(7, W - 1, 7) - 1, np.arange(21, W - 1, 21) + 0.75])
    rng = np.random.default_rng(5)
    q = np.concatenate([np.stack([xs, np.full(len(xs), y)], 1) for y in (0.0, 5.5, 6.0, 20.5, 21.0, 42.0, H - 1.0, H - 1.5)])
    q = q[rng.permutation(len(q))]
    det = np.stack([rng.integers(0, W, 800), rng.choice([0, 5, 6, 7, 20, 21, 22, 41, 42, 43, H - 2, H - 1], 800)], 1)
    det[:4] = [[0, 0], [W - 1, 0], [0, H - 1], [W - 1, H - 1]]
    return _lists(q, det, 5)


def _one_cell():
    rng = np.random.default_rng(6)
    q = 100 + rng.random((64, 2)) * 5.5                              # 64 candidates in one cell of 6 pixels
    return _lists(q, 98 + rng.integers(0, 10, (40, 2)), 6)


def _bad_q():
    q = [[50, 50], [np.nan, 60], [70, np.inf], [-np.inf, 5], [-0.5, 80], [W - 0.75, 90], [100, H - 0.5], [110, -1e-3], [120, 120]]
    return _lists(q, [[50, 51], [60, 60], [119, 121]], 7, ages=np.zeros(9))


# name: (lists, min_distance, max_age, cap (None: n_trk + n_det))
STAGE_CASES = {
    "both_empty": lambda: (_lists([], []), 3.0, 0, None),
    "no_tracks": lambda: (_random(1, 0, 300), 3.0, 0, None),
    "no_detections": lambda: (_random(2, 300, 0), 3.0, 0, None),
    "distance_boundary": lambda: (_boundary(), 3.0, 0, None),
    "edges_md3": lambda: (_edges(), 3.0, 0, None),
    "edges_md1": lambda: (_edges(), 1.0, 0, None),
    "edges_md20_5": lambda: (_edges(), 20.5, 0, None),
    "one_cell_64": lambda: (_one_cell(), 1.0, 0, None),
    "one_cell_64_md3": lambda: (_one_cell(), 3.0, 0, None),
    "trips_1500_1500": lambda: (_random(3, 1500, 1500), 3.0, 0, None),
    "trips_1500_1500_md20_5": lambda: (_random(3, 1500, 1500), 20.5, 0, None),
    "trips_1500_1500_md1": lambda: (_random(4, 1500, 1500), 1.0, 0, None),
    "truncated": lambda: (_random(8, 1100, 1300), 3.0, 0, 1100 + 37),
    "cap_is_n_trk": lambda: (_random(9, 200, 300), 3.0, 0, 200),
    "max_age_1": lambda: (_random(10, 900, 900), 3.0, 1, None),
    "max_age_3": lambda: (_random(11, 900, 900), 3.0, 3, None),
    "bad_q": lambda: (_bad_q(), 3.0, 0, None),
}
_WANT = {}


def _want(name):
    if name not in _WANT:
        c, md, max_age, cap = STAGE_CASES[name]()
        cap = len(c["q"]) + len(c["det"]) if cap is None else cap
        _WANT[name] = (c, md, max_age, cap,
                       CR.merge(W, H, md, max_age, c["q"], c["resp"], c["ids"], c["ages"], c["keep"], c["det"], c["dresp"], c["next_id"], cap))
    return _WANT[name]


def _same(got, want, n=None):
    for k in ("xy", "resp", "id", "age", "src"):
        g = got[k] if n is None else got[k][:n]
        assert g.dtype == want[k].dtype and g.shape == want[k].shape and g.tobytes() == want[k].tobytes(), k


@pytest.mark.parametrize("name", list(STAGE_CASES))
def test_stage_equals_twin_host(stage_ctx, name):
    c, md, max_age, cap, want = _want(name)
    got = stage_ctx.carry_merge(W, H, md, max_age, c["q"], c["resp"], c["ids"], c["ages"], c["keep"], c["det"], c["dresp"], c["next_id"], cap)
    assert got["n_carried"] == want["n_carried"]
    _same(got, want)
    n_trk, n_det, n_c = len(c["q"]), len(c["det"]), want["n_carried"]
    if name.startswith("trips") or name.startswith("max_age") or name.startswith("edges"):      # not vacuous
        assert 0 < n_c < int(c["keep"].sum()) and 0 < len(want["src"]) - n_c < n_det
    if name == "truncated":
        assert len(want["src"]) == cap and n_c + n_det > cap + 100
    if name == "distance_boundary":
        # d2 == 9 exactly: kept (1, 5, 7, detections 8, 10, 11); one float ulp inside: dropped (3); 2.5 from a carried point: dropped (9)
        assert want["src"].tolist() == [0, 1, 2, 4, 5, 6, 7, 8, 10, 11]
    if name == "bad_q":
        assert want["src"].tolist() == [0, 8, 10]
    if name == "one_cell_64":
        assert 1 < n_c < 64


@pytest.mark.parametrize("name", ["both_empty", "distance_boundary", "trips_1500_1500", "truncated", "max_age_3"])
def test_stage_equals_twin_device(stage_ctx, tc, name):
    c, md, max_age, cap, want = _want(name)
    d = {k: tc.from_numpy(c[k]).cuda() for k in ("q", "resp", "ids", "ages", "keep", "det", "dresp")}
    got = stage_ctx.carry_merge(W, H, md, max_age, d["q"], d["resp"], d["ids"], d["ages"], d["keep"], d["det"], d["dresp"], c["next_id"], cap)
    tc.cuda.synchronize()
    n = int(got["n_out"].cpu()[0])
    assert n == len(want["src"]) and int(got["n_carried"].cpu()[0]) == want["n_carried"]
    _same({k: got[k].cpu().numpy() for k in ("xy", "resp", "id", "age", "src")}, want, n)


def test_stage_argument_errors(pkg, stage_ctx):
    c = _random(20, 50, 50)
    args = lambda: [c["q"], c["resp"], c["ids"], c["ages"], c["keep"], c["det"], c["dresp"]]
    for md, max_age in [(0.5, 0), (257.0, 0), (float("nan"), 0), (float("inf"), 0), (3.0, -1)]:
        with pytest.raises(pkg.SvoError):
            stage_ctx.carry_merge(W, H, md, max_age, *args())
    with pytest.raises(pkg.SvoError):
        stage_ctx.carry_merge(W, H, 3.0, 0, *args(), cap=49)          # cap < n_trk
    with pytest.raises(pkg.SvoError):
        stage_ctx.carry_merge(0, H, 3.0, 0, *args())
    assert len(stage_ctx.carry_merge(W, H, 256.0, 0, *args())["src"]) >= 1


# ---- b. the fused online paths ------------------------------------------------------------------------------------------------
N_FRAMES = 6
GF = (100, 0.01, 8.0)
GRID = (32, 32, 2)
DETECT = {
    "fast": lambda O, img: O.fast(img),
    "buckets": lambda O, img: bucket(O.fast(img), img.shape[1], img.shape[0], *GRID),
    "gftt": lambda O, img: G.gftt(img, *GF)[0],
}
_SEQ, _REF = {}, {}


def _setup(c, det):
    if det == "buckets":
        c.set_fast_buckets(*GRID)
    if det == "gftt":
        c.set_lk_detector("gftt", *GF)


@pytest.fixture(scope="module")
def seq6(synth):
    if "s" not in _SEQ:
        seq = synth.StereoSequence(width=416, height=128, n_frames=N_FRAMES, seed=11)
        _SEQ["s"] = (seq, [tuple(x.numpy() for x in seq.render(t)) for t in range(N_FRAMES)])
    return _SEQ["s"]


def _pair(oracle, prm, P1, P2, ch, prev, cur, det, pose):
    """One pair of the twin chain: the oracle's four LK calls + circular_keep give keep and t2_left per list entry, the oracle's
    step on the same list gives the record."""
    ch.number()
    Lp = ch.kps.copy()
    p0 = np.stack([Lp["x"], Lp["y"]], 1).astype(np.float32)
    (L1, R1), (L2, R2) = prev, cur
    p1, s1 = oracle.lk_track(L1, R1, p0)
    p2, s2 = oracle.lk_track(R1, R2, p1)
    p3, s3 = oracle.lk_track(R2, L2, p2)
    p0r, s4 = oracle.lk_track(L2, L1, p3)
    keep, _ = oracle.circular_keep(p0, p1, p2, p3, p0r, s1, s2, s3, s4)
    res, _cur, pose = oracle.lk_track_step(prm, L1, R1, L2, R2, Lp, pose, want_tracks=True, threads=8)
    assert res["tracks"][3].tobytes() == p3[keep != 0].tobytes() and res["tracks"][0].tobytes() == p0[keep != 0].tobytes()
    pnp = oracle.pnp_ransac(oracle.triangulate(P1, P2, res["tracks"][0], res["tracks"][1]), res["tracks"][3], _K(P1))
    trk = ch.step(p3, keep, det)
    return dict(res=res, pnp=pnp, n_prev=len(Lp), n_cur=len(det), trk_ids=trk[0], trk_ages=trk[1], kps=ch.kps.copy(), ids=ch.ids.copy(),
                ages=ch.ages.copy(), pose=pose.copy())


def _chain_ref(oracle, seq6, det, first_plain=False, md=3.0, max_age=0):
    """Per frame of the sequence what the chain holds and reports; first_plain: frame 0 was stored with carry off (C6)."""
    key = (det, first_plain, md, max_age)
    if key in _REF:
        return _REF[key]
    seq, frames = seq6
    P1, P2 = seq.proj()
    prm = oracle.make_params(P1, P2)
    ch = CR.Chain(416, 128, md, max_age)
    out, pose = [], np.eye(4)
    for t, fr in enumerate(frames):
        D = DETECT[det](oracle, fr[0])
        if t == 0:
            ch.store_plain(D) if first_plain else ch.first(D)
            out.append(dict(n_cur=len(D), kps=ch.kps.copy(), ids=None if first_plain else ch.ids.copy(), ages=None if first_plain else ch.ages.copy()))
            continue
        e = _pair(oracle, prm, P1, P2, ch, frames[t - 1], fr, D, pose)
        pose = e["pose"]
        out.append(e)
    # not vacuous: every pair tracks and carries, detections are dropped AND added, some track lives through the whole sequence
    assert all(e["res"]["ok"] for e in out[1:])
    for a, b in zip(out[1:], out[2:]):
        carried = int((b["ages"] > 0).sum())
        assert 30 <= carried < len(b["ids"]) and len(b["ids"]) - carried < b["n_cur"]
    assert out[-1]["ages"].max() == N_FRAMES - 1
    _REF[key] = out
    return out


def _check_step(g, e, tracks, trk_ids):
    r, pnp = e["res"], e["pnp"]
    assert int(g["ok"]) == r["ok"] and int(g["fail_stage"]) == r["fail_stage"]
    assert int(g["n_prev_kps"]) == e["n_prev"] and int(g["n_cur_kps"]) == e["n_cur"]     # the list's length / the detector's count
    assert int(g["n_tracked"]) == r["n_tracked"] and int(g["n_inliers"]) == r["n_inliers"]
    assert int(g["ransac_iters"]) == pnp["ransac_iters"] and int(g["lm_iters"]) == pnp["lm_iters"]
    for got, want in zip(tracks[:4], r["tracks"]):
        assert got.tobytes() == want.tobytes()
    assert tracks[4].tobytes() == pnp["mask"].tobytes()
    assert relfro(g["pose"].reshape(4, 4), e["pose"]) <= TIGHT * 10
    assert trk_ids[0].tobytes() == e["trk_ids"].tobytes() and trk_ids[1].tobytes() == e["trk_ages"].tobytes()


def _check_list(kps, ids_ages, e):
    assert kps.tobytes() == e["kps"].tobytes()
    assert ids_ages[0].tobytes() == e["ids"].tobytes() and ids_ages[1].tobytes() == e["ages"].tobytes()


@pytest.mark.parametrize("det", ["fast", "buckets", "gftt"])
def test_add_frame_equals_twin_chain(pkg, oracle, seq6, det):
    seq, frames = seq6
    P1, P2 = seq.proj()
    ref = _chain_ref(oracle, seq6, det)
    c = pkg.Context(416, 128, device=0, P1=P1, P2=P2)
    _setup(c, det)
    c.set_track_carry(True)
    assert c.track_carry() == (True, 3.0, 0)
    seen = {}
    for t, fr in enumerate(frames):
        rc, g = c.add_frame(*fr)
        assert rc == 0 and int(g["n_cur_kps"]) == ref[t]["n_cur"]
        if t:
            _check_step(g, ref[t], c.last_tracks(), c.last_track_ids())
        ids, ages = c.frame_track_ids()
        _check_list(c.frame_keypoints(), (ids, ages), ref[t])
        # an id seen at step t keeps its id at t + 1: every aged entry was in the previous list, one frame younger
        assert len(np.unique(ids)) == len(ids)
        for i, a in zip(ids[ages > 0], ages[ages > 0]):
            assert seen[int(i)] == a - 1
        seen = dict(zip(ids.tolist(), ages.tolist()))
    # reset restarts the ids at 0
    c.reset()
    c.add_frame(*frames[0])
    _check_list(c.frame_keypoints(), c.frame_track_ids(), ref[0])
    rc, g = c.add_frame(*frames[1])
    _check_list(c.frame_keypoints(), c.frame_track_ids(), ref[1])
    c.close()


def test_streams_step_equals_twin_chain(pkg, oracle, seq6):
    """two streams, the second one frame behind: it joins as an init item in mid-run"""
    seq, frames = seq6
    P1, P2 = seq.proj()
    ref = _chain_ref(oracle, seq6, "fast")
    c = pkg.Context(416, 128, device=0, P1=P1, P2=P2, max_batch=3)
    c.set_track_carry(True, 3.0, 0)
    c.streams_create(2)
    for s in range(N_FRAMES):
        ids = [0] if s == 0 else [0, 1]
        fr = [frames[s]] if s == 0 else [frames[s], frames[s - 1]]
        recs = c.streams_step(ids, [f[0] for f in fr], [f[1] for f in fr])
        for item, sid in enumerate(ids):
            t = s - sid
            g, e = recs[item], ref[t]
            assert int(g["n_cur_kps"]) == e["n_cur"] and int(g["ok"]) == 1
            if t:
                e2 = dict(e, pose=e["pose"])
                _check_step(g, e2, c.streams_tracks(item), c.streams_track_ids(item))
            else:
                assert len(c.streams_track_ids(item)[0]) == 0
            kps, ids_, ages_ = c.streams_frame_tracks(sid)
            _check_list(kps, (ids_, ages_), e)
    # a reset stream starts over at id 0; the other one goes on
    c.streams_reset(1)
    c.streams_step([1], [frames[0][0]], [frames[0][1]])
    kps, ids_, ages_ = c.streams_frame_tracks(1)
    _check_list(kps, (ids_, ages_), ref[0])
    assert c.streams_frame_tracks(0)[1].tobytes() == ref[N_FRAMES - 1]["ids"].tobytes()
    c.close()


def test_enable_after_streams_create_equals_before(pkg, seq6):
    seq, frames = seq6
    P1, P2 = seq.proj()
    a = pkg.Context(416, 128, device=0, P1=P1, P2=P2, max_batch=3)
    a.set_track_carry(True)
    a.streams_create(2)
    b = pkg.Context(416, 128, device=0, P1=P1, P2=P2, max_batch=3)
    b.streams_create(2)
    b.set_track_carry(True)
    for s in range(3):
        L, R = [frames[s][0], frames[s + 1][0]], [frames[s][1], frames[s + 1][1]]
        ra, rb = a.streams_step([1, 0], L, R), b.streams_step([1, 0], L, R)
        assert ra.tobytes() == rb.tobytes()
        for sid in (0, 1):
            for x, y in zip(a.streams_frame_tracks(sid), b.streams_frame_tracks(sid)):
                assert x.tobytes() == y.tobytes() and len(x) > 0
    for c in (a, b):
        c.close()


def test_switch_between_two_frames(pkg, oracle, seq6):
    """C6: a frame stored before the switch is numbered by the step that first sees it"""
    seq, frames = seq6
    P1, P2 = seq.proj()
    ref = _chain_ref(oracle, seq6, "fast", first_plain=True)
    c = pkg.Context(416, 128, device=0, P1=P1, P2=P2)
    c.add_frame(*frames[0])
    with pytest.raises(pkg.SvoError):
        c.frame_track_ids()                                            # carry was off for that step
    c.set_track_carry(True)
    for t in (1, 2):
        rc, g = c.add_frame(*frames[t])
        assert rc == 0
        _check_step(g, ref[t], c.last_tracks(), c.last_track_ids())
        _check_list(c.frame_keypoints(), c.frame_track_ids(), ref[t])
    assert ref[1]["trk_ids"].max() < ref[1]["n_prev"] and not ref[1]["trk_ages"].any()
    c.close()


def test_off_again_equals_a_fresh_context(pkg, tc, seq6):
    seq, frames = seq6
    P1, P2 = seq.proj()
    a = pkg.Context(416, 128, device=0, P1=P1, P2=P2, max_batch=3)
    b = pkg.Context(416, 128, device=0, P1=P1, P2=P2, max_batch=3)
    a.set_track_carry(True, 5.0, 2)
    for fr in frames[:3]:
        a.add_frame(*fr)
    a.set_track_carry(False)
    assert a.track_carry() == (False, 0.0, 0)
    a.reset()
    for fr in frames:
        (rca, ga), (rcb, gb) = a.add_frame(*fr), b.add_frame(*fr)
        assert rca == rcb == 0 and ga.tobytes() == gb.tobytes()
        assert a.frame_keypoints().tobytes() == b.frame_keypoints().tobytes()
        for x, y in zip(a.last_tracks(), b.last_tracks()):
            assert x.tobytes() == y.tobytes()
        with pytest.raises(pkg.SvoError):
            a.frame_track_ids()
    # ... and the batch entry points work again
    L, R = (tc.stack([tc.from_numpy(f[k]) for f in frames[:4]]).cuda() for k in (0, 1))
    assert a.track_batch(L, R).tobytes() == b.track_batch(L, R).tobytes()
    for c in (a, b):
        c.close()


def test_ingest_add_frame_equals_add_frame_on_resized_frames(pkg, synth, tc):
    seq, frames = _render(synth, tc, 832, 256, 4)
    P1, P2 = (pkg.scale_projection(P, 0.5, 0.5, "nearest").reshape(12) for P in seq.proj())
    a = pkg.Context(416, 128, device=0, P1=P1, P2=P2)
    a.ingest_create(832, 256, "nearest", 0.5, 0.5)
    b = pkg.Context(416, 128, device=0, P1=P1, P2=P2)
    for c in (a, b):
        c.set_track_carry(True, 3.0, 2)
    for t, fr in enumerate(frames):
        small = tuple(b.resize(x, 416, 128, "nearest", 0.5, 0.5) for x in fr)
        (rca, ga), (rcb, gb) = a.ingest_add_frame(*fr), b.add_frame(*small)
        assert rca == rcb == 0 and ga.tobytes() == gb.tobytes() and (t == 0 or int(ga["n_tracked"]) > 0)
        assert a.frame_keypoints().tobytes() == b.frame_keypoints().tobytes()
        for x, y in zip(a.frame_track_ids() + (a.last_track_ids() if t else ()), b.frame_track_ids() + (b.last_track_ids() if t else ())):
            assert x.tobytes() == y.tobytes() and len(x) > 0
        assert a.frame_track_ids()[1].max() == min(t, 2)               # max_age 2: no track grows older
    L, R = (tc.stack([tc.from_numpy(f[k]) for f in frames[:2]]).cuda() for k in (0, 1))     # one pair: within any max_batch
    with pytest.raises(pkg.SvoError, match=r"\(-4\).*track carry"):    # the batch twin refuses as well
        a.ingest_track_batch(L, R)
    for c in (a, b):
        c.close()


def test_batch_entry_points_refuse_and_argument_errors(pkg, tc, seq6):
    seq, frames = seq6
    P1, P2 = seq.proj()
    c = pkg.Context(416, 128, device=0, P1=P1, P2=P2, max_batch=3)
    for bad in [(0.5, 0), (256.5, 0), (float("nan"), 0), (float("inf"), 0), (3.0, -1)]:
        with pytest.raises(pkg.SvoError):
            c.set_track_carry(True, *bad)
        assert c.track_carry() == (False, 0.0, 0)                      # nothing changes
    c.set_track_carry(True, 1.0, 7)
    assert c.track_carry() == (True, 1.0, 7)
    L, R = (tc.stack([tc.from_numpy(f[k]) for f in frames[:3]]).cuda() for k in (0, 1))
    with pytest.raises(pkg.SvoError, match=r"\(-4\).*track carry"):    # SVO_ERR_STATE
        c.track_batch(L, R)
    c.upload_frames(0, np.stack([f[0] for f in frames[:3]]), np.stack([f[1] for f in frames[:3]]))
    with pytest.raises(pkg.SvoError, match=r"\(-4\)"):
        c.track_uploaded(0, 3)
    with pytest.raises(pkg.SvoError, match=r"\(-4\)"):
        c.track_uploaded_async(0, 3)
    with pytest.raises(pkg.SvoError):
        c.last_track_ids()                                             # no pair yet
    c.close()
    o = pkg.Context(416, 128, device=0, track_mode=pkg.MODE_ORB, orb_nlevels=3, orb_nfeatures=300)
    with pytest.raises(pkg.SvoError):
        o.set_track_carry(True)
    o.set_track_carry(False)                                           # off is always accepted
    o.close()


# ---- d. the host runner: track_carry keys, the id / age columns of the tracks file ------------------------------------------
def _tracks_rows(path):
    """per F record of a tracks file: the T rows as float arrays"""
    frames = []
    for ln in open(path).read().splitlines():
        if ln.startswith("F "):
            frames.append([])
        elif ln.startswith("T "):
            frames[-1].append([float(v) for v in ln.split()[1:]])
    return [np.array(r, np.float64).reshape(len(r), -1) if r else np.zeros((0, 0)) for r in frames]


def test_runner_track_carry(host_built, pkg, oracle, seq6, tmp_path):
    seq, frames = seq6
    ref = _chain_ref(oracle, seq6, "fast")
    for cam in (0, 1):
        os.makedirs(tmp_path / f"image_{cam}")
        for t, fr in enumerate(frames):
            _write_pgm(tmp_path / f"image_{cam}" / f"{t:06d}.pgm", fr[cam])
    want = np.array([np.eye(4)[:3]] + [e["pose"][:3] for e in ref[1:]])
    exe = os.path.join(host_built, "run_kitti_stereo")
    for on in (1, 0):
        y = tmp_path / f"loop{on}.yaml"
        _write_yaml(y, str(tmp_path), fx=seq.fx, fy=seq.fy, cx=seq.cx, cy=seq.cy)
        with open(y, "a", encoding="utf-8") as f:
            f.write(f"track_carry: {on}\ntracks_file: {tmp_path}/tracks{on}.txt\n")
        r = subprocess.run([exe, str(y), str(tmp_path / f"loop{on}.txt")], capture_output=True)
        assert r.returncode == 0, r.stderr.decode()
        rows = _tracks_rows(tmp_path / f"tracks{on}.txt")
        assert len(rows) == N_FRAMES
        if not on:
            assert all(r.shape[1] == 7 for r in rows[1:])                 # no id / age columns while carry is off
            continue
        poses = np.loadtxt(tmp_path / "loop1.txt").reshape(-1, 3, 4)
        assert poses.shape[0] == N_FRAMES and np.abs(poses - want).max() < 1e-6
        for t in range(1, N_FRAMES):
            assert rows[t].shape[1] == 9
            assert np.array_equal(rows[t][:, 7].astype(np.int64), ref[t]["trk_ids"]) and np.array_equal(rows[t][:, 8].astype(np.int32), ref[t]["trk_ages"])
    # --interleave: two copies of the sequence as the streams of one context, the same poses
    os.makedirs(tmp_path / "out")
    ys = []
    for k in (0, 1):
        y = tmp_path / f"s{k}.yaml"
        _write_yaml(y, str(tmp_path), fx=seq.fx, fy=seq.fy, cx=seq.cx, cy=seq.cy)
        with open(y, "a", encoding="utf-8") as f:
            f.write("track_carry: 1\n")
        ys.append(str(y))
    r = subprocess.run([exe, *ys, "--poses-dir", str(tmp_path / "out"), "--interleave"], capture_output=True)
    assert r.returncode == 0, r.stderr.decode()
    for k in (0, 1):
        poses = np.loadtxt(tmp_path / "out" / f"s{k}.yaml.poses.txt").reshape(-1, 3, 4)
        assert poses.shape[0] == N_FRAMES and np.abs(poses - want).max() < 1e-6
