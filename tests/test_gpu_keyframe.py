"""Keyframe mode (-m gpu): svo_set_keyframe / svo_keyframe_join against the numpy twin tests/_keyframe_ref.py.

(a) the stage join on hand-built lists at the wave, trip and capacity edges, HOST and DEVICE, byte for byte; (b) the fused online
chain -- svo_add_frame with carry and keyframe on -- on 12 frames of the 416 x 128 synthetic sequence against a twin chain made
of the oracle's LK and step, _carry_ref.Chain, _keyframe_ref.Chain and oracle.pnp_ransac on the joined lists: integers, lists,
mask and table byte for byte, rvec / tvec / pose to the bar test_gpu_carry holds for chained poses; (c) off means off, K1, K7,
the ingest twin, the refinement stage beside it, and the rules of the switch.  Every test fails without the feature: the
symbols do not exist."""
import numpy as np
import pytest

import _carry_ref as CR
import _keyframe_ref as KR
import test_gpu_carry as TC
from test_gpu_ingest import _render
from test_gpu_parity_fullsize import TIGHT, _K, relfro

pytestmark = pytest.mark.gpu

BAR = TIGHT * 10                       # test_gpu_carry._check_step's bar for a chained pose (relative Frobenius)


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


# ---- a. the stage join -------------------------------------------------------------------------------------------------------
SIZES = [0, 1, 63, 64, 65, 1025, 16384]            # the wave (64), workgroup (1024), LDS trip (4096) and capacity (16384) edges
OFFSET = 1 << 40
_CASES = {}


def _case(n_rows, n_trk, overlap):
    """Two strictly ascending id lists above 2^40.  overlap: "none" (even rows, odd tracks), "all" (the shorter list is a
    prefix of the longer), "half" (every other id of the shorter list is in the longer)."""
    key = (n_rows, n_trk, overlap)
    if key not in _CASES:
        rng = np.random.default_rng(n_rows * 7 + n_trk)
        if overlap == "none":
            tab, trk = OFFSET + 2 * np.arange(n_rows, dtype=np.int64), OFFSET + 2 * np.arange(n_trk, dtype=np.int64) + 1
        elif overlap == "all":
            tab, trk = OFFSET + 3 * np.arange(n_rows, dtype=np.int64), OFFSET + 3 * np.arange(n_trk, dtype=np.int64)
        else:
            tab, trk = OFFSET + 2 * np.arange(n_rows, dtype=np.int64), OFFSET + 4 * np.arange(n_trk, dtype=np.int64)
            if n_trk > n_rows:                     # the tracks run past the table's end and interleave with it
                trk = OFFSET + np.arange(n_trk, dtype=np.int64)
        X, xy = rng.random((n_rows, 3)).astype(np.float32), rng.random((n_trk, 2)).astype(np.float32) * 400
        _CASES[key] = (tab, X, trk, xy, KR.join(tab, X, trk, xy))
    return _CASES[key]


def _same_join(got, want, n=None):
    for k in ("X", "xy", "trk", "row"):
        g = got[k] if n is None else got[k][:n]
        assert g.dtype == want[k].dtype and g.shape == want[k].shape and g.tobytes() == want[k].tobytes(), k


@pytest.mark.parametrize("overlap", ["none", "all", "half"])
@pytest.mark.parametrize("n_rows", SIZES)
def test_stage_join_equals_twin_host(stage_ctx, n_rows, overlap):
    hits = 0
    for n_trk in SIZES:
        tab, X, trk, xy, want = _case(n_rows, n_trk, overlap)
        _same_join(stage_ctx.keyframe_join(tab, X, trk, xy), want)
        hits += len(want["trk"])
        if overlap == "all":
            assert len(want["trk"]) == min(n_rows, n_trk)
        if overlap == "half" and min(n_rows, n_trk) > 1:
            assert 0 < len(want["trk"]) < max(n_rows, n_trk)
    assert (hits == 0) == (overlap == "none" or n_rows == 0)


@pytest.mark.parametrize("overlap", ["none", "all", "half"])
def test_stage_join_equals_twin_device(stage_ctx, tc, overlap):
    for n_rows in SIZES:
        for n_trk in SIZES:
            tab, X, trk, xy, want = _case(n_rows, n_trk, overlap)
            d = [tc.from_numpy(a).cuda() for a in (tab, X, trk, xy)]
            got = stage_ctx.keyframe_join(*d)
            tc.cuda.synchronize()
            n = int(got["n_out"].cpu()[0])
            assert n == len(want["trk"]), (n_rows, n_trk)
            assert all(int(got[k].shape[0]) == max(min(n_rows, n_trk), 1) for k in ("X", "xy", "trk", "row"))      # outputs of exactly `cap` entries
            _same_join({k: got[k].cpu().numpy() for k in ("X", "xy", "trk", "row")}, want, n)


def test_stage_join_low_words_alone_do_not_match(stage_ctx):
    tab = np.array([5, (1 << 32) + 5, (2 << 32) + 5, OFFSET + 5], np.int64)
    trk = np.array([5, (2 << 32) + 5, (3 << 32) + 5, OFFSET + 5, OFFSET + (1 << 32) + 5], np.int64)
    X, xy = np.arange(12, dtype=np.float32).reshape(4, 3), np.arange(10, dtype=np.float32).reshape(5, 2)
    got = stage_ctx.keyframe_join(tab, X, trk, xy)
    assert got["trk"].tolist() == [0, 1, 3] and got["row"].tolist() == [0, 2, 3]
    _same_join(got, KR.join(tab, X, trk, xy))


def test_stage_join_argument_errors(pkg, stage_ctx):
    tab, X, trk, xy, _ = _case(65, 64, "all")
    with pytest.raises(pkg.SvoError):
        stage_ctx.keyframe_join(tab, X, trk, xy, cap=63)             # cap < min(n_rows, n_trk)
    with pytest.raises(pkg.SvoError):
        stage_ctx.keyframe_join(tab, X, trk, xy, cap=-1)
    big = np.arange((1 << 20) + 1, dtype=np.int64)
    with pytest.raises(pkg.SvoError):
        stage_ctx.keyframe_join(big, np.zeros((len(big), 3), np.float32), trk, xy)      # n_rows > 2^20
    lib, h = stage_ctx.lib, stage_ctx.h
    import ctypes as C
    n = C.c_int(0)
    p = lambda a: C.c_void_p(a.ctypes.data)
    out = [np.zeros((64, 3), np.float32), np.zeros((64, 2), np.float32), np.zeros(64, np.int32), np.zeros(64, np.int32)]
    pn = C.cast(C.byref(n), C.c_void_p)
    assert lib.svo_keyframe_join(h, None, p(X), 65, p(trk), p(xy), 64, *[p(o) for o in out], 64, pn, 0) == -1       # a null list
    assert lib.svo_keyframe_join(h, p(tab), p(X), 65, p(trk), p(xy), 64, *[p(o) for o in out], 64, None, 0) == -1   # a null count
    assert lib.svo_keyframe_join(h, p(tab), p(X), 65, p(trk), p(xy), 64, *[p(o) for o in out], 64, pn, 7) == -1     # no such memory kind
    assert lib.svo_keyframe_join(h, p(tab), p(X), -1, p(trk), p(xy), 64, *[p(o) for o in out], 64, pn, 0) == -1
    assert lib.svo_keyframe_join(h, p(tab), p(X), 65, p(trk), p(xy), 64, *[p(o) for o in out], 64, pn, 0) == 0 and n.value == 64


# ---- b. the fused chain ------------------------------------------------------------------------------------------------------
N_FRAMES = 12
MIN_TRACKS, MAX_GAP = 600, 4                       # test parameters: chosen so that the twin chain alone meets _not_vacuous
_SEQ, _REF = {}, {}


@pytest.fixture(scope="module")
def seq12(synth):
    if "s" not in _SEQ:
        seq = synth.StereoSequence(width=416, height=128, n_frames=N_FRAMES, seed=11)
        _SEQ["s"] = (seq, [tuple(x.numpy() for x in seq.render(t)) for t in range(N_FRAMES)])
    return _SEQ["s"]


def twin_chain(oracle, seq, frames, min_tracks=MIN_TRACKS, max_gap=MAX_GAP):
    """Per frame what the chain holds and reports: test_gpu_carry's twin pair (the oracle's LK and step on _carry_ref.Chain's
    list) with _keyframe_ref.Chain on top; the chain pose handed to the next pair is the keyframe's where it was applied."""
    P1, P2 = seq.proj()
    prm = oracle.make_params(P1, P2)
    ch = CR.Chain(416, 128, 3.0, 0)
    kf = KR.Chain(min_tracks, max_gap, prm.inlier_rate, prm.max_t2, lambda X, xy: oracle.pnp_ransac(X, xy, _K(P1)))
    out, pose = [], np.eye(4)
    for t, fr in enumerate(frames):
        D = oracle.fast(fr[0])
        if t == 0:
            ch.first(D)
            out.append(dict(n_cur=len(D)))
            continue
        pose_a = pose
        e = TC._pair(oracle, prm, P1, P2, ch, frames[t - 1], fr, D, pose_a)
        tri = oracle.triangulate(P1, P2, e["res"]["tracks"][0], e["res"]["tracks"][1])
        k = kf.step(t, e["res"]["ok"], e["pose"], pose_a, e["trk_ids"], e["res"]["tracks"][3], tri)
        e.update(kf=k, pose=k["pose"].copy(), tab_ids=kf.ids.copy(), tab_X=kf.X.copy())
        pose = e["pose"]
        out.append(e)
    return out


def _not_vacuous(ref):
    ks = [e["kf"] for e in ref[1:]]
    assert all(e["res"]["ok"] for e in ref[1:])
    assert any(k["status"] == KR.APPLIED and k["gap"] >= 3 for k in ks)
    assert any(k["switched"] and k["status"] == KR.SHORT for k in ks)                                      # a switch caused by SHORT
    assert any(k["switched"] and k["status"] == KR.APPLIED and k["gap"] >= MAX_GAP for k in ks)            # ... and one by max_gap
    assert any(k["status"] == KR.APPLIED and np.abs(k["pose"] - k["pose_pair"]).max() > 1e-6 for k in ks)


@pytest.fixture(scope="module")
def ref12(oracle, seq12):
    if "r" not in _REF:
        _REF["r"] = twin_chain(oracle, *seq12)
        _not_vacuous(_REF["r"])
    return _REF["r"]


INTS = ("status", "switched", "kf_index", "gap", "n_rows", "n_join", "n_inliers", "ransac_iters")


def _check_kf(c, k, tab_ids, tab_X, lm_iters=True):
    """the context's read-backs of the last step against a twin step k and the twin's table after it"""
    g = c.keyframe_result()
    for f in INTS + (("lm_iters",) if lm_iters else ()):
        assert g[f] == k[f], (f, g[f], k[f])
    m = c.keyframe_matches()
    j = k["join"]
    assert m["ids"].tobytes() == j["ids"].tobytes() and m["X"].tobytes() == j["X"].tobytes() and m["xy"].tobytes() == j["xy"].tobytes()
    assert m["trk"].tobytes() == j["trk"].tobytes() and m["mask"].tobytes() == k["mask"].tobytes()
    ids, X = c.keyframe_table()
    assert ids.tobytes() == tab_ids.tobytes() and X.tobytes() == tab_X.tobytes()
    if k["n_inliers"] > 0:
        assert relfro(g["rvec"], k["rvec"]) <= BAR and relfro(g["tvec"], k["tvec"]) <= BAR
    else:
        assert not g["rvec"].any() and not g["tvec"].any()
    assert relfro(g["pose_pair"], k["pose_pair"]) <= BAR
    if k["kf_index"] >= 0:
        assert relfro(g["pose_K"], k["pose_K"]) <= BAR
    else:
        assert not g["pose_K"].any()
    return g


def _but_pose(rec):
    return b"".join(rec[f].tobytes() for f in rec.dtype.names if f != "pose")


def test_add_frame_equals_twin_chain(pkg, seq12, ref12):
    seq, frames = seq12
    P1, P2 = seq.proj()
    c = pkg.Context(416, 128, device=0, P1=P1, P2=P2, max_batch=2)
    plain = pkg.Context(416, 128, device=0, P1=P1, P2=P2, max_batch=2)           # the carry-only chain
    for x in (c, plain):
        x.set_track_carry(True)
    c.set_keyframe(True, MIN_TRACKS, MAX_GAP)
    assert c.keyframe() == (True, MIN_TRACKS, MAX_GAP) and plain.keyframe() == (False, 0, 0)
    with pytest.raises(pkg.SvoError):
        c.keyframe_result()                                          # no pair yet
    for t, fr in enumerate(frames):
        (rc, g), (rcp, gp) = c.add_frame(*fr), plain.add_frame(*fr)
        assert rc == rcp == 0 and int(g["n_cur_kps"]) == ref12[t]["n_cur"]
        if t == 0:
            with pytest.raises(pkg.SvoError):
                c.keyframe_result()
            continue
        e = ref12[t]
        TC._check_step(g, e, c.last_tracks(), c.last_track_ids())   # counts, tracks, mask, ids; pose = the twin's keyframe-adjusted one
        assert _but_pose(g) == _but_pose(gp)                         # everything but the pose is the carry-only chain's
        for x, y in zip(c.last_tracks() + list(c.frame_track_ids()), plain.last_tracks() + list(plain.frame_track_ids())):
            assert x.tobytes() == y.tobytes()
        k = _check_kf(c, e["kf"], e["tab_ids"], e["tab_X"])
        assert relfro(c.get_pose(), e["pose"]) <= BAR and c.get_pose().tobytes() == g["pose"].reshape(4, 4).tobytes()
        if e["kf"]["status"] != KR.APPLIED:
            assert g["pose"].tobytes() == k["pose_pair"].tobytes()   # untouched, bit for bit
        with pytest.raises(pkg.SvoError):
            plain.keyframe_result()                                  # the mode was off for that step
    for x in (c, plain):
        x.close()


def test_same_bytes_on_every_run(pkg, seq12):
    """K8"""
    seq, frames = seq12
    P1, P2 = seq.proj()
    runs = []
    for _ in range(2):
        c = pkg.Context(416, 128, device=0, P1=P1, P2=P2, max_batch=2)
        c.set_track_carry(True)
        c.set_keyframe(True, MIN_TRACKS, MAX_GAP)
        got = []
        for t, fr in enumerate(frames[:7]):
            rc, g = c.add_frame(*fr)
            got.append(g.tobytes())
            if t:
                r, m = c.keyframe_result(), c.keyframe_matches()
                got += [np.asarray(r[f]).tobytes() for f in sorted(r)] + [m[f].tobytes() for f in sorted(m)] + [a.tobytes() for a in c.keyframe_table()]
        c.close()
        runs.append(got)
    assert runs[0] == runs[1]


# ---- c. the rules of the switch ------------------------------------------------------------------------------------------------
def test_off_means_off(pkg, seq12):
    """never enabled == enabled and switched off again: records, lists and timing-mark names"""
    seq, frames = seq12
    P1, P2 = seq.proj()
    a = pkg.Context(416, 128, device=0, P1=P1, P2=P2, max_batch=2)
    b = pkg.Context(416, 128, device=0, P1=P1, P2=P2, max_batch=2)
    for c in (a, b):
        c.set_track_carry(True)
        c.enable_timing(True)
    b.set_keyframe(True, 30, 3)
    names_on = None
    for fr in frames[:4]:
        b.add_frame(*fr)
        names_on = [n for n, _ in b.get_timing()]
    assert [n for n in names_on if n.startswith("kf_")] == ["kf_join", "kf_pnp", "kf_update"]
    b.set_keyframe(False)
    assert b.keyframe() == (False, 0, 0)
    b.reset()
    b.get_timing()
    for t, fr in enumerate(frames):
        (rca, ga), (rcb, gb) = a.add_frame(*fr), b.add_frame(*fr)
        assert rca == rcb == 0 and ga.tobytes() == gb.tobytes()
        assert a.frame_keypoints().tobytes() == b.frame_keypoints().tobytes()
        for x, y in zip(list(a.frame_track_ids()) + (a.last_tracks() + list(a.last_track_ids()) if t else []),
                        list(b.frame_track_ids()) + (b.last_tracks() + list(b.last_track_ids()) if t else [])):
            assert x.tobytes() == y.tobytes()
        na, nb = [n for n, _ in a.get_timing()], [n for n, _ in b.get_timing()]
        assert na == nb and not any(n.startswith("kf_") for n in na)
        if t:
            with pytest.raises(pkg.SvoError):
                b.keyframe_result()
    for c in (a, b):
        c.close()


def _run(c, frames, ts):
    out = []
    for t in ts:
        rc, g = c.add_frame(*frames[t])
        out.append((rc, g))
    return out


def test_reset_and_set_pose_clear_the_state(pkg, seq12):
    """K1"""
    seq, frames = seq12
    P1, P2 = seq.proj()
    c = pkg.Context(416, 128, device=0, P1=P1, P2=P2, max_batch=2)
    c.set_track_carry(True)
    c.set_keyframe(True, 30, 0)
    _run(c, frames, range(4))
    r = c.keyframe_result()
    assert r["status"] == pkg.KF_APPLIED and r["kf_index"] == 0 and r["gap"] == 3
    # set_pose: the next step has no keyframe and takes its frame a, under the new pose
    T = np.eye(4)
    T[:3, 3] = [1.0, 2.0, 3.0]
    c.set_pose(T)
    rc, g = c.add_frame(*frames[4])
    r = c.keyframe_result()
    assert rc == 0 and (r["status"], r["switched"], r["kf_index"], r["n_rows"], r["n_join"]) == (pkg.KF_NONE, 1, -1, 0, 0)
    assert len(c.keyframe_matches()["trk"]) == 0 and len(c.keyframe_table()[0]) > 30
    rc, g = c.add_frame(*frames[5])
    r = c.keyframe_result()
    assert r["status"] == pkg.KF_APPLIED and r["kf_index"] == 3 and r["gap"] == 2 and r["pose_K"].tobytes() == T.tobytes()    # K6: frame a
    # set_track_carry and set_keyframe clear it as well
    for t, again in ((6, lambda: c.set_track_carry(True)), (7, lambda: c.set_keyframe(True, 30, 0))):
        again()
        c.add_frame(*frames[t])
        r = c.keyframe_result()
        assert (r["status"], r["switched"], r["kf_index"]) == (pkg.KF_NONE, 1, -1)
    # reset: a new chain, frames count from 0 again
    c.reset()
    _run(c, frames, range(3))
    r = c.keyframe_result()
    assert r["status"] == pkg.KF_APPLIED and r["kf_index"] == 0 and r["gap"] == 2 and r["pose_K"].tobytes() == np.eye(4).tobytes()
    c.close()


def test_failed_step_keeps_the_state(pkg, seq12):
    """K7, with one definite status per failed step: a dimmed frame has fewer than 30 corners, so its pair fails, but its LK
    tracks stand -- joined, solved, reported, PAIR_FAILED; an all-black frame tracks nothing -- SHORT.  Neither moves the
    keyframe; the first good pair afterwards finds none of its ids in the table and takes a new one."""
    seq, frames = seq12
    P1, P2 = seq.proj()
    c = pkg.Context(416, 128, device=0, P1=P1, P2=P2, max_batch=2)
    c.set_track_carry(True)
    c.set_keyframe(True, 30, 0)
    _run(c, frames, range(3))
    before, tab = c.keyframe_result(), c.keyframe_table()
    assert before["status"] == pkg.KF_APPLIED and before["kf_index"] == 0
    pose = c.get_pose()

    def kept(r, gap):
        assert r["switched"] == 0 and r["kf_index"] == 0 and r["gap"] == gap and r["n_rows"] == len(tab[0])
        assert r["pose_K"].tobytes() == before["pose_K"].tobytes() and r["pose_pair"].tobytes() == pose.tobytes()
        assert c.get_pose().tobytes() == pose.tobytes()
        after = c.keyframe_table()
        assert after[0].tobytes() == tab[0].tobytes() and after[1].tobytes() == tab[1].tobytes()

    dim = tuple(np.round(im.astype(np.float64) * 0.2 + 100).astype(np.uint8) for im in frames[3])
    rc, g = c.add_frame(*dim)
    r = c.keyframe_result()
    assert rc != 0 and int(g["ok"]) == 0 and int(g["fail_stage"]) == 1 and int(g["n_cur_kps"]) < 30 and g["pose"].reshape(4, 4).tobytes() == pose.tobytes()    # SVO_FAIL_FEW_KEYPOINTS
    assert r["status"] == pkg.KF_PAIR_FAILED and r["n_join"] >= 30 and r["ransac_iters"] > 0                   # the solve ran
    m = c.keyframe_matches()
    assert len(m["trk"]) == r["n_join"] and int(m["mask"].sum()) == r["n_inliers"]
    kept(r, 3)
    black = np.zeros_like(frames[0][0])
    rc, g = c.add_frame(black, black)
    r = c.keyframe_result()
    assert rc != 0 and int(g["ok"]) == 0
    assert r["status"] == pkg.KF_SHORT and r["n_join"] == 0 and r["n_inliers"] == 0 and not r["rvec"].any()
    kept(r, 4)
    rc, g = c.add_frame(*frames[4])                                  # from the black frame: nothing to track, the gap grows
    r = c.keyframe_result()
    assert int(g["ok"]) == 0 and r["status"] == pkg.KF_SHORT and r["n_join"] == 0
    kept(r, 5)
    rc, g = c.add_frame(*frames[5])                                  # a regular pair again, under new ids
    r = c.keyframe_result()
    assert rc == 0 and (r["status"], r["switched"], r["kf_index"], r["gap"], r["n_join"]) == (pkg.KF_SHORT, 1, 0, 6, 0)
    ids, _ = c.keyframe_table()
    assert len(ids) >= 30 and ids.min() > tab[0].max()
    rc, g = c.add_frame(*frames[6])
    r = c.keyframe_result()
    assert rc == 0 and (r["status"], r["kf_index"], r["gap"]) == (pkg.KF_APPLIED, 5, 2)
    c.close()


def test_ingest_add_frame_equals_add_frame_on_resized_frames(pkg, synth, tc):
    seq, frames = _render(synth, tc, 832, 256, 5)
    P1, P2 = (pkg.scale_projection(P, 0.5, 0.5, "nearest").reshape(12) for P in seq.proj())
    a = pkg.Context(416, 128, device=0, P1=P1, P2=P2, max_batch=2)
    a.ingest_create(832, 256, "nearest", 0.5, 0.5)
    b = pkg.Context(416, 128, device=0, P1=P1, P2=P2, max_batch=2)
    for c in (a, b):
        c.set_track_carry(True)
        c.set_keyframe(True, 30, 3)
    applied = 0
    for t, fr in enumerate(frames):
        small = tuple(b.resize(x, 416, 128, "nearest", 0.5, 0.5) for x in fr)
        (rca, ga), (rcb, gb) = a.ingest_add_frame(*fr), b.add_frame(*small)
        assert rca == rcb == 0 and ga.tobytes() == gb.tobytes()
        if t:
            ra, rb = a.keyframe_result(), b.keyframe_result()
            assert all(np.asarray(ra[f]).tobytes() == np.asarray(rb[f]).tobytes() for f in ra)
            ma, mb = a.keyframe_matches(), b.keyframe_matches()
            assert all(ma[f].tobytes() == mb[f].tobytes() for f in ma)
            assert all(x.tobytes() == y.tobytes() for x, y in zip(a.keyframe_table(), b.keyframe_table()))
            applied += ra["status"] == pkg.KF_APPLIED
    assert applied >= 1
    for c in (a, b):
        c.close()


def test_pose_refine_stays_independent(pkg, oracle, seq12):
    """with pose_refine: reproj on, the pair's record is the refine-only chain's and the keyframe solve -- never refined -- is
    the twin's on the step's own lists"""
    seq, frames = seq12
    P1, P2 = seq.proj()
    a = pkg.Context(416, 128, device=0, P1=P1, P2=P2, max_batch=2)               # refine only
    b = pkg.Context(416, 128, device=0, P1=P1, P2=P2, max_batch=2)
    for c in (a, b):
        c.set_track_carry(True)
        c.set_pose_refine("reproj")
    b.set_keyframe(True, MIN_TRACKS, MAX_GAP)
    prm = oracle.make_params(P1, P2)
    kf = KR.Chain(MIN_TRACKS, MAX_GAP, prm.inlier_rate, prm.max_t2, lambda X, xy: oracle.pnp_ransac(X, xy, _K(P1)))
    applied = 0
    for t, fr in enumerate(frames[:8]):
        pose_a = b.get_pose()
        (rca, ga), (rcb, gb) = a.add_frame(*fr), b.add_frame(*fr)
        assert rca == rcb == 0
        if t == 0:
            continue
        assert _but_pose(ga) == _but_pose(gb)
        ra, rb = a.refine_result(), b.refine_result()
        assert all(np.asarray(ra[f]).tobytes() == np.asarray(rb[f]).tobytes() for f in ra)
        trk, (ids, _) = b.last_tracks(), b.last_track_ids()
        tri = oracle.triangulate(P1, P2, trk[0], trk[1])
        pose_pair = pose_a @ gb["T_rel_inv"].reshape(4, 4)
        k = kf.step(t, int(gb["ok"]), pose_pair, pose_a, ids, trk[3], tri)
        g = _check_kf(b, k, kf.ids, kf.X)
        want = k["pose"] if k["status"] == KR.APPLIED else g["pose_pair"]
        assert relfro(gb["pose"].reshape(4, 4), want) <= BAR
        applied += k["status"] == KR.APPLIED
    assert applied >= 2
    for c in (a, b):
        c.close()


def test_setter_and_refusals(pkg, tc, seq12):
    seq, frames = seq12
    P1, P2 = seq.proj()
    c = pkg.Context(416, 128, device=0, P1=P1, P2=P2, max_batch=3)
    with pytest.raises(pkg.SvoError, match=r"\(-4\).*track carry"):  # SVO_ERR_STATE: carry is off
        c.set_keyframe(True)
    c.set_keyframe(False)                                            # off is always accepted
    c.set_track_carry(True)
    lib, h = c.lib, c.h
    for bad in [(3, 0), (c.cfg.max_keypoints + 1, 0), (60, -1), (60, 1)]:
        assert lib.svo_set_keyframe(h, 1, *bad) == -1                # SVO_ERR_ARG, nothing changes
        assert c.keyframe() == (False, 0, 0)
    c.set_window_ba(4)
    with pytest.raises(pkg.SvoError, match=r"\(-4\).*window"):
        c.set_keyframe(True)
    c.set_window_ba(0)
    c.set_keyframe(True, 4, 2)
    assert c.keyframe() == (True, 4, 2)
    c.set_keyframe(True, c.cfg.max_keypoints, 0)
    assert c.keyframe() == (True, c.cfg.max_keypoints, 0)
    with pytest.raises(pkg.SvoError, match=r"\(-4\).*keyframe"):
        c.set_window_ba(4)
    assert c.window_ba()[0] == 0
    with pytest.raises(pkg.SvoError, match=r"\(-4\).*keyframe"):
        c.set_track_carry(False)
    assert c.track_carry()[0] is True
    c.streams_create(2)
    with pytest.raises(pkg.SvoError, match=r"\(-4\).*keyframe"):
        c.streams_step([0], [frames[0][0]], [frames[0][1]])
    L, R = (tc.stack([tc.from_numpy(f[k]) for f in frames[:3]]).cuda() for k in (0, 1))
    with pytest.raises(pkg.SvoError, match=r"\(-4\)"):               # the batch entry points refuse because carry is on
        c.track_batch(L, R)
    c.set_keyframe(False)
    assert len(c.streams_step([0], [frames[0][0]], [frames[0][1]])) == 1
    c.close()
    one = pkg.Context(416, 128, device=0, P1=P1, P2=P2, max_batch=1)
    one.set_track_carry(True)
    assert one.lib.svo_set_keyframe(one.h, 1, 60, 0) == -1           # the solve needs item 1 of the pose workspace
    one.close()
    o = pkg.Context(416, 128, device=0, track_mode=pkg.MODE_ORB, orb_nlevels=3, orb_nfeatures=300)
    assert o.lib.svo_set_keyframe(o.h, 1, 60, 0) == -1
    o.set_keyframe(False)
    o.close()
    # the ingest twin of svo_streams_step refuses too
    i = pkg.Context(416, 128, device=0, P1=P1, P2=P2, max_batch=3)
    i.ingest_create(832, 256, "nearest", 0.5, 0.5)
    i.set_track_carry(True)
    i.set_keyframe(True)
    i.streams_create(1)
    big = np.zeros((256, 832), np.uint8)
    with pytest.raises(pkg.SvoError, match=r"\(-4\).*keyframe"):
        i.ingest_streams_step([0], [big], [big])
    i.close()


def test_read_back_capacity_rules(pkg, seq12):
    import ctypes as C
    seq, frames = seq12
    P1, P2 = seq.proj()
    c = pkg.Context(416, 128, device=0, P1=P1, P2=P2, max_batch=2)
    c.set_track_carry(True)
    c.set_keyframe(True, 30, 0)
    _run(c, frames, range(3))
    n = C.c_int(0)
    m, (ids, X) = c.keyframe_matches(), c.keyframe_table()
    assert len(m["trk"]) >= 30 and len(ids) >= len(m["trk"])
    buf = np.full(len(ids) + 8, -7, np.int64)
    p = C.c_void_p(buf.ctypes.data)
    assert c.lib.svo_get_keyframe_matches(c.h, p, None, None, None, None, len(m["trk"]) - 1, C.byref(n)) == -1 and n.value == len(m["trk"])
    assert c.lib.svo_get_keyframe_table(c.h, p, None, len(ids) - 1, C.byref(n)) == -1 and n.value == len(ids) and (buf == -7).all()
    assert c.lib.svo_get_keyframe_table(c.h, p, None, len(ids), C.byref(n)) == 0 and buf[:len(ids)].tobytes() == ids.tobytes() and buf[len(ids)] == -7
    assert c.lib.svo_get_keyframe_matches(c.h, None, None, None, None, None, 0, None) == -1
    assert c.lib.svo_get_keyframe_result(c.h, None) == -1
    c.close()
