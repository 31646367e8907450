"""The sliding window's landmark table (-m gpu): svo_window_update against the numpy twin tests/_window_ref.py -- counts, ids,
masks and observations bit for bit, poses and X to 1e-12 relative -- on the fixtures of tests/_window_cases.py, from HOST and
from DEVICE memory, at an exact and a short capacity.  Every test fails without the feature: the symbol does not exist."""
import numpy as np
import pytest

import _window_cases as WC
import _window_ref as WR

pytestmark = pytest.mark.gpu

COLS = ("ids", "seen", "active", "obs_left", "obs_right")
_CASE = {}


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


def _case(name):
    """(table in, frames, step, cap, the twin's table out), computed once per case."""
    if name not in _CASE:
        tab, frames, step, cap = WC.UPDATE_CASES[name]()
        want = WC.apply(tab, frames, step, cap)
        _CASE[name] = (tab, frames, step, max(want["m"], tab["m"]) if cap is None else cap, want)      # both tables have cap rows
    return _CASE[name]


def _close(got, want):
    """1e-12 relative to the size of the quantity (a pose entry is O(1); a point, the scene's depth)."""
    want = np.asarray(want, np.float64)
    assert np.isfinite(got).all()
    assert np.abs(got - want).max(initial=0.0) <= 1e-12 * max(1.0, np.abs(want).max(initial=0.0))


def _check(got, want):
    m = want["m"]
    assert (got["n"], got["m"]) == (want["n"], m)
    for k in COLS:
        a, b = np.asarray(got[k])[:m], want[k][:m]
        assert a.dtype.itemsize == b.dtype.itemsize and a.tobytes() == b.tobytes(), k
    _close(np.asarray(got["poses"]), want["poses"])
    _close(np.asarray(got["X"])[:m], want["X"][:m])


def _host(ctx, tab, frames, step, cap):
    p = step["pair"]
    return ctx.window_update(tab, frames, p["t1_left"], p["t1_right"], p["t2_left"], p["t2_right"], p["ids"], p["tri"], step["pose_a"],
                             step["pose_b"], cap=cap)


def _device(tc, ctx, tab, frames, step, cap):
    dev = lambda a, dt=None: tc.from_numpy(np.ascontiguousarray(a if dt is None else np.asarray(a).astype(dt))).cuda()
    p = step["pair"]
    t = {k: dev(tab[k][:tab["m"]]) for k in ("ids", "X", "obs_left", "obs_right")}
    t["seen"], t["active"] = dev(tab["seen"][:tab["m"]].view(np.int32)), dev(tab["active"][:tab["m"]].view(np.int32))
    t["poses"], t["counts"] = dev(tab["poses"]), dev(np.array([tab["n"], tab["m"], 0, 0], np.int32))
    out = ctx.window_update(t, frames, dev(p["t1_left"]), dev(p["t1_right"]), dev(p["t2_left"]), dev(p["t2_right"]), dev(p["ids"]),
                            dev(p["tri"]), dev(step["pose_a"]), dev(step["pose_b"]), cap=cap)
    ctx.sync()
    res = {k: v.cpu().numpy() for k, v in out.items()}
    res["seen"], res["active"] = res["seen"].view(np.uint32), res["active"].view(np.uint32)
    res["n"], res["m"], res["needed"] = (int(v) for v in res["counts"][:3])
    return res


@pytest.mark.parametrize("name", sorted(WC.UPDATE_CASES))
def test_update_host(stage_ctx, name):
    tab, frames, step, cap, want = _case(name)
    _check(_host(stage_ctx, tab, frames, step, cap), want)              # cap: exactly the rows the larger table has


@pytest.mark.parametrize("name", ["empty_table", "slide_w4", "slide_w8", "big_ids", "rows_1025_tracks_63", "rows_65_tracks_2049"])
def test_update_device(tc, stage_ctx, name):
    tab, frames, step, cap, want = _case(name)
    got = _device(tc, stage_ctx, tab, frames, step, cap + 7)
    assert got["needed"] == want["m"] and int(got["counts"][3]) == 0
    _check(got, want)


def test_update_late_row(stage_ctx):
    """T6: an id whose row is made one pair late enters between its neighbours."""
    s0, s1 = WC.late_row_case()
    t = _host(stage_ctx, None, 4, s0, None)
    _check(t, WC.apply(WR.empty(), 4, s0))
    want = WC.apply(WC.apply(WR.empty(), 4, s0), 4, s1)
    assert want["ids"].tolist() == [10, 20, 30, 40]
    _check(_host(stage_ctx, WC.apply(WR.empty(), 4, s0), 4, s1, None), want)


def test_update_is_repeatable(stage_ctx):
    tab, frames, step, cap, _ = _case("rows_2049_tracks_1025")
    a, b = _host(stage_ctx, tab, frames, step, cap), _host(stage_ctx, tab, frames, step, cap)
    for k in COLS + ("poses", "X"):
        assert a[k].tobytes() == b[k].tobytes(), k


@pytest.mark.parametrize("name", ["second_pair_w4", "rows_65_tracks_2049"])
def test_update_cap_one_short(tc, pkg, stage_ctx, name):
    """T7: HOST refuses; DEVICE hands back a cleared table and the rows it needed, and writes no row."""
    tab, frames, step, cap, want = _case(name)
    assert cap == want["m"]
    with pytest.raises(pkg.SvoError, match="cap is too small"):
        _host(stage_ctx, tab, frames, step, cap - 1)
    got = _device(tc, stage_ctx, tab, frames, step, cap - 1)
    assert got["counts"].tolist() == [0, 0, want["m"], 0]
    assert not got["ids"].any() and not got["seen"].any() and not got["obs_left"].any() and not got["poses"].any()


def test_update_refusals(pkg, stage_ctx):
    tab, frames, step, cap, _ = _case("second_pair_w4")
    for bad_frames in (1, 9):
        with pytest.raises(pkg.SvoError, match="frames"):
            _host(stage_ctx, tab, bad_frames, step, cap)
    with pytest.raises(pkg.SvoError, match="more frames"):
        _host(stage_ctx, dict(tab, n=5), 4, step, 4096)
    with pytest.raises(pkg.SvoError, match="more rows"):
        _host(stage_ctx, tab, frames, step, tab["m"] - 1)


# ---- the optimiser (svo_window_ba) against the twin's solve(): status, masks and counts equal; poses, X and info to 1e-9 --------
INT_FIELDS = ("status", "n_frames", "n_landmarks", "n_usable", "n_obs", "n_active", "iters")


def _solve_host(ctx, tab, **kw):
    s = dict(WC.BA_SETTINGS, **kw)
    return ctx.window_solve(tab, WC.P1, WC.P2, rounds=s["rounds"], iters=s["iters"], sigma_px=s["sigma"], min_obs=s["min_obs"])


def _near(got, want, what, tol=1e-9):
    scale = max(1.0, float(np.abs(want).max(initial=0.0)))
    err = float(np.abs(np.asarray(got) - want).max(initial=0.0))
    print("%s: max error %.3e of scale %.3e" % (what, err, scale))
    assert np.isfinite(np.asarray(got)).all() and err <= tol * scale, what


def _check_solve(res, tab_out, tab_in, want):
    for k in INT_FIELDS:
        assert res[k] == want[k], (k, res[k], want[k])
    assert (res["frame_active"] == want["frame_active"]).all()
    n, m, D = tab_in["n"], tab_in["m"], 6 * (tab_in["n"] - 1)
    if np.isfinite(want["info"]).all():
        _near(res["info"], want["info"], "info")
    assert (res["info"][D:] == 0).all() and (res["info"][:, D:] == 0).all()
    for k in ("cost_first", "cost_last"):
        assert (np.isnan(res[k]) and np.isnan(want[k])) or abs(res[k] - want[k]) <= 1e-9 * max(1.0, abs(want[k])), k
    if want["status"] == WR.APPLIED:
        assert (np.asarray(tab_out["active"]) == want["active"]).all()
        _near(tab_out["poses"], want["poses"], "poses")
        _near(tab_out["X"], want["X"], "X")
    else:                                                             # the table is handed back bit for bit
        for k in ("poses", "X", "active"):
            assert np.asarray(tab_out[k]).tobytes() == np.ascontiguousarray(tab_in[k][:m] if k != "poses" else tab_in[k]).tobytes(), k


@pytest.mark.parametrize("name", sorted(WC.BA_CASES))
def test_solve_host(stage_ctx, name):
    tab, want = WC.ba_case(name)
    res, out = _solve_host(stage_ctx, tab, **WC.BA_CASES[name].get("settings", {}))
    _check_solve(res, out, tab, want)


def test_solve_device_in_place_and_repeatable(tc, pkg, stage_ctx):
    """DEVICE: the table's tensors are overwritten in place; two runs of one case give the same bytes (W8), and they are the
    bytes of the HOST call."""
    tab, want = WC.ba_case("n5_Tp1_holes_once")
    dev = lambda a: tc.from_numpy(np.ascontiguousarray(a)).cuda()
    runs = []
    for _ in range(2):
        t = {k: dev(tab[k]) for k in ("ids", "X", "obs_left", "obs_right", "poses")}
        t["seen"], t["active"] = dev(tab["seen"].view(np.int32)), dev(tab["active"].view(np.int32))
        t["counts"] = dev(np.array([tab["n"], tab["m"], 0, 0], np.int32))
        raw, _ = stage_ctx.window_solve(t, WC.P1, WC.P2, rounds=4, iters=2, sigma_px=1.0, min_obs=10)
        stage_ctx.sync()
        runs.append((raw.cpu().numpy().tobytes(), {k: t[k].cpu().numpy() for k in ("poses", "X", "active")}))
    assert runs[0][0] == runs[1][0]
    for k in ("poses", "X", "active"):
        assert runs[0][1][k].tobytes() == runs[1][1][k].tobytes(), k
    from importlib import import_module
    import conftest
    b = import_module(conftest.entry.PKG_NAME + ".binding")
    res = b.WindowResult.from_buffer_copy(runs[0][0]).as_dict()
    out = dict(runs[0][1], active=runs[0][1]["active"].view(np.uint32))
    _check_solve(res, out, tab, want)
    hres, hout = _solve_host(stage_ctx, tab)
    assert hout["X"].tobytes() == out["X"].tobytes() and hout["poses"].tobytes() == out["poses"].tobytes()
    assert hres["info"].tobytes() == res["info"].tobytes()


def test_solve_lambda_exit(stage_ctx):
    """A slot nobody observes: every factorisation fails, lambda passes 1e10 after 15 rejected steps a round, the table stays."""
    tab, _ = WC.ba_case("slot_without_observations")
    want = WR.solve(tab, WC.P1, WC.P2, rounds=2, iters=20, sigma=1.0, min_obs=10)
    assert [r["exit"] for r in want["log"]] == ["lambda", "lambda"]
    res, out = _solve_host(stage_ctx, tab, rounds=2, iters=20)
    assert res["iters"] == want["iters"] == 30
    _check_solve(res, out, tab, want)


def test_solve_skips_a_window_of_one_frame(stage_ctx):
    tab, _ = WC.ba_case("n3_63")
    one = dict(tab, n=1)
    res, out = _solve_host(stage_ctx, one)
    assert res["status"] == WR.SKIPPED and res["n_frames"] == 1 and res["iters"] == 0 and not res["info"].any()
    assert out["X"].tobytes() == tab["X"].tobytes() and out["poses"].tobytes() == tab["poses"].tobytes()


def test_solve_refusals(pkg, stage_ctx):
    tab, _ = WC.ba_case("n3_63")
    for kw, word in ((dict(rounds=0), "rounds"), (dict(rounds=17), "rounds"), (dict(iters=0), "iters"), (dict(iters=101), "iters"),
                     (dict(sigma=0.0), "sigma"), (dict(sigma=float("nan")), "sigma"), (dict(min_obs=0), "min_obs")):
        with pytest.raises(pkg.SvoError, match=word):
            _solve_host(stage_ctx, tab, **kw)
    with pytest.raises(pkg.SvoError, match="SVO_WINDOW_MAX_FRAMES"):
        _solve_host(stage_ctx, dict(tab, n=9))


# ---- the fused path (svo_set_window_ba): svo_add_frame keeps the chain's table and adjusts it after every step --------------------
N_FUSED = 9


@pytest.fixture(scope="module")
def seq9(synth, tc):
    from test_gpu_ingest import _render
    return _render(synth, tc, 416, 128, N_FUSED)


def _ctx(pkg, seq, frames=0):
    c = pkg.Context(416, 128, device=0, P1=seq.proj()[0], P2=seq.proj()[1])
    c.set_track_carry(True, 3.0, 0)
    if frames:
        c.set_window_ba(frames, 4, 2, 1.0, 10)
    return c


def _inverse_of_slot(row):
    R, t = row[:9].reshape(3, 3), row[9:]
    P = np.eye(4)
    P[:3, :3], P[:3, 3] = R.T, -(R.T @ t)
    return P


@pytest.mark.parametrize("W", [3, 4])
def test_fused_steps_equal_the_twin_step_by_step(pkg, oracle, seq9, W):
    """Every step: the twin gets the table read BEFORE the step, the pair's tracks, ids and the oracle's triangulation, and must
    give the table read after it; every record field but `pose`, every track, id and age equals a carry-only context's."""
    seq, frames = seq9
    P1, P2 = (np.asarray(p, np.float64).reshape(3, 4) for p in seq.proj())
    ctx, ref = _ctx(pkg, seq, W), _ctx(pkg, seq)
    before, applied = WR.empty(), 0
    try:
        for f, (L, R) in enumerate(frames):
            pose_a = ctx.get_pose().copy()
            rc, rec = ctx.add_frame(L, R)
            rc2, rec2 = ref.add_frame(L, R)
            assert rc == rc2
            for k in rec.dtype.names:
                if k != "pose":
                    assert rec[k].tobytes() == rec2[k].tobytes(), (f, k)
            if f == 0:
                with pytest.raises(pkg.SvoError):
                    ctx.window()
                continue
            trk, trk2 = ctx.last_tracks(), ref.last_tracks()
            ids, ages = ctx.last_track_ids()
            ids2, ages2 = ref.last_track_ids()
            assert all(a.tobytes() == b.tobytes() for a, b in zip(trk, trk2)) and ids.tobytes() == ids2.tobytes() and ages.tobytes() == ages2.tobytes()
            got, res = ctx.window(), ctx.window_result()
            assert rec["ok"] == 1 and (np.diff(ids) > 0).all()                       # C5: compact order is ascending id
            t1l, t1r, t2r, t2l = trk[:4]
            tri = oracle.triangulate(P1, P2, t1l, t1r)
            pose_b = pose_a @ rec["T_rel_inv"].reshape(4, 4)
            mid = WR.update(before, W, t1l, t1r, t2l, t2r, ids, tri, pose_a, pose_b)
            want = WR.solve(mid, P1, P2, rounds=4, iters=2, sigma=1.0, min_obs=10)
            print("frame %d W %d: n %d m %d status %d margins %s" % (f, W, mid["n"], mid["m"], want["status"],
                                                                      [("%.1e" % r["margin"], "%.1e" % r["accept_margin"]) for r in want["log"]]))
            assert (got["n"], got["m"]) == (mid["n"], mid["m"])
            for k in ("ids", "seen", "obs_left", "obs_right"):
                assert got[k].tobytes() == mid[k][:mid["m"]].tobytes(), (f, k)
            for k in INT_FIELDS:
                assert res[k] == want[k], (f, k, res[k], want[k])
            assert (res["frame_active"] == want["frame_active"]).all()
            _near(got["poses"], want["poses"], "poses")
            _near(got["X"], want["X"], "X")
            assert (got["active"] == want["active"]).all()
            if want["status"] == WR.APPLIED:
                applied += 1
                _near(rec["pose"].reshape(4, 4), _inverse_of_slot(want["poses"][mid["n"] - 1]), "record pose")
            else:
                _near(rec["pose"].reshape(4, 4), pose_b, "record pose", 1e-12)
            assert ctx.get_pose().tobytes() == rec["pose"].reshape(4, 4).tobytes()
            before = got
        assert applied >= N_FUSED - 3
        full = np.uint32((1 << W) - 1)
        assert before["n"] == W and int((before["seen"] == full).sum()) >= 100      # the last window: landmarks seen in every slot
    finally:
        ctx.close()
        ref.close()


def test_fused_off_on_off_and_a_failed_step(pkg, seq9):
    seq, frames = seq9
    ctx, ref = _ctx(pkg, seq), _ctx(pkg, seq)
    try:
        assert ctx.window_ba() == (0, 0, 0, 0.0, 0)
        ctx.set_window_ba(3, 4, 2, 1.0, 10)
        assert ctx.window_ba() == (3, 4, 2, 1.0, 10)
        for L, R in frames[:4]:
            ctx.add_frame(L, R)
        assert ctx.window()["n"] == 3 and ctx.window_result()["status"] == WR.APPLIED
        blank = np.zeros_like(frames[0][0])
        rc, rec = ctx.add_frame(blank, blank)                                         # a failed step clears the window (T1)
        assert rec["ok"] == 0 and (ctx.window()["n"], ctx.window()["m"]) == (0, 0) and ctx.window_result()["status"] == WR.SKIPPED
        ctx.set_window_ba(0)
        ctx.reset()
        for L, R in frames[:5]:
            (rc, a), (rc2, b) = ctx.add_frame(L, R), ref.add_frame(L, R)
            assert rc == rc2 and a.tobytes() == b.tobytes()
            assert all(x.tobytes() == y.tobytes() for x, y in zip(ctx.frame_track_ids(), ref.frame_track_ids()))
        with pytest.raises(pkg.SvoError):
            ctx.window()
    finally:
        ctx.close()
        ref.close()


def _step_from_cleared_table(ctx, oracle, P1, P2, frame):
    """One step; the table read after it must be the twin's update of an EMPTY table by the step's tracks.  Returns the pose
    the step started from and the tracks' ids."""
    pose_a = ctx.get_pose().copy()
    rc, rec = ctx.add_frame(*frame)
    assert rc == 0 and rec["ok"] == 1
    t1l, t1r, t2r, t2l = ctx.last_tracks()[:4]
    ids, _ = ctx.last_track_ids()
    tri = oracle.triangulate(P1, P2, t1l, t1r)
    want = WR.update(WR.empty(), 3, t1l, t1r, t2l, t2r, ids, tri, pose_a, pose_a @ rec["T_rel_inv"].reshape(4, 4))
    got = ctx.window()
    assert want["n"] == 2 and want["m"] > 100                                        # (a table that was kept would hold 3 frames)
    assert (got["n"], got["m"]) == (want["n"], want["m"])
    for k in ("ids", "seen", "obs_left", "obs_right"):
        assert got[k].tobytes() == want[k][:want["m"]].tobytes(), k
    return pose_a, ids


def test_every_restart_clears_the_table(pkg, oracle, seq9):
    """T1, the twin of the keyframe's K1 test: svo_set_pose, svo_set_track_carry, svo_set_window_ba and svo_reset each make the
    next step start from a cleared table; across the first two the track ids run on from the chain's counter."""
    seq, frames = seq9
    P1, P2 = (np.asarray(p, np.float64).reshape(3, 4) for p in seq.proj())
    ctx = _ctx(pkg, seq, 3)
    try:
        hi = -1                                                                      # the largest id the chain has given out
        for fr in frames[:4]:
            ctx.add_frame(*fr)
            hi = max(hi, int(ctx.frame_track_ids()[0].max()))
        assert ctx.window()["n"] == 3
        T = np.eye(4)
        T[:3, 3] = [1.0, 2.0, 3.0]
        breaks = ((4, lambda: ctx.set_pose(T)), (5, lambda: ctx.set_track_carry(True, 3.0, 0)), (6, lambda: ctx.set_window_ba(3, 4, 2, 1.0, 10)))
        for f, restart in breaks:
            listed = ctx.frame_track_ids()[0]                                         # every id of the list the next pair tracks from
            restart()
            pose_a, ids = _step_from_cleared_table(ctx, oracle, P1, P2, frames[f])
            if f == 4:
                assert pose_a.tobytes() == T.tobytes()
            if f in (4, 5):
                assert (np.diff(ids) > 0).all() and np.isin(ids, listed).all()       # the tracks kept their ids, in ascending order
                new = np.setdiff1d(ctx.frame_track_ids()[0], listed)
                assert len(new) > 0 and new.min() > hi                               # and the counter went on: no id is given twice
            hi = max(hi, int(ctx.frame_track_ids()[0].max()))
        ctx.reset()
        ctx.add_frame(*frames[0])
        with pytest.raises(pkg.SvoError):
            ctx.window()
        pose_a, _ = _step_from_cleared_table(ctx, oracle, P1, P2, frames[1])
        assert pose_a.tobytes() == np.eye(4).tobytes()
    finally:
        ctx.close()


def test_fused_switch_rules(pkg, seq9):
    seq, frames = seq9
    c = pkg.Context(416, 128, device=0, P1=seq.proj()[0], P2=seq.proj()[1])
    orb = pkg.Context(416, 128, device=0, track_mode=pkg.MODE_ORB, orb_nlevels=3, orb_nfeatures=300)
    try:
        with pytest.raises(pkg.SvoError, match=r"\(-4\)"):                             # SVO_ERR_STATE: track carry is off
            c.set_window_ba(3)
        c.set_track_carry(True, 3.0, 0)
        for kw in (dict(frames=1), dict(frames=9), dict(rounds=0), dict(iters=101), dict(sigma_px=0.0), dict(min_obs=0)):
            with pytest.raises(pkg.SvoError, match=r"\(-1\)"):
                c.set_window_ba(**dict(dict(frames=3), **kw))
        with pytest.raises(pkg.SvoError, match=r"\(-1\)"):
            orb.set_window_ba(3)
        c.set_window_ba(3)
        with pytest.raises(pkg.SvoError, match=r"\(-4\)"):
            c.set_track_carry(False)
        c.streams_create(2)
        L, R = frames[0]
        with pytest.raises(pkg.SvoError, match=r"\(-4\)"):
            c.streams_step([0, 1], np.stack([L, L]), np.stack([R, R]))
        c.set_window_ba(0)
        c.set_track_carry(False)
    finally:
        c.close()
        orb.close()
