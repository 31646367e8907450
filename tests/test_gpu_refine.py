"""The pose refinement stage on the GPU (svo_set_pose_refine / svo_refine_pose / svo_get_refine_result, csrc/refine.hip)
against tests/_refine_ref.py, the numpy restatement of its rules.

Bars: status, n_active and the active flags equal; rvec / tvec / R within 1e-9 absolute (TIGHT, the bar of the LM refit: the
same class of computation -- double sums in another order, device sin / cos / sqrt; the reference's own spread under a
reordering of the points is ~1e-15); info within 1e-9 of its largest entry; the iteration count only bounded."""
import numpy as np
import pytest

import _refine_cases as RC
import _refine_ref as RR
import _rigs
from test_gpu_parity_pose import TIGHT
from test_refine_ref import fixture_ok

pytestmark = pytest.mark.gpu

ORB_KW = dict(min_move2=0.05 ** 2, max_move2=100.0)
ERR_ARG = -1


@pytest.fixture(scope="module")
def tc():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def stage_ctx(pkg):
    c = pkg.Context(416, 128, device=0, max_keypoints=4096)
    c.set_pose_refine("off", rounds=RC.ROUNDS, iters=RC.ITERS)      # the stage call uses the settings even while the mode is off
    yield c
    c.close()


def _check_result(got, run, n, d, what=""):
    """A GPU record against a reference run."""
    print(f"{what}: status {got['status']} active {got['n_active']}/{n} iters {got['iters']} (ref {run['iters']}) "
          f"|dt| {np.abs(got['tvec'] - run['t']).max():.1e} |dr| {np.abs(got['rvec'] - run['rvec']).max():.1e} "
          f"ref exits {[e['exit'] for e in run['log']]}")
    assert got["status"] == run["status"] and got["n_points"] == n and got["views"] == d // 2, what
    assert got["n_active"] == run["n_active"] and np.array_equal(got["active"], run["active"]), what
    assert np.abs(got["rvec"] - run["rvec"]).max() <= TIGHT, what
    assert np.abs(got["tvec"] - run["t"]).max() <= TIGHT, what
    assert np.abs(got["R"] - run["R"]).max() <= TIGHT, what
    top = np.abs(run["info"]).max()
    assert np.abs(got["info"] - run["info"]).max() <= TIGHT * top, what
    assert np.array_equal(got["info"], got["info"].T)
    for k in ("cost_first", "cost_last"):
        assert abs(got[k] - run[k]) <= TIGHT * max(1.0, abs(run[k])), (what, k)


@pytest.mark.parametrize("rig,n,kind,d", RC.stage_cases())
def test_stage_call_equals_reference(stage_ctx, tc, rig, n, kind, d):
    """svo_refine_pose on host and on device inputs: 30 % outliers, some points behind the camera, all points behind it."""
    c, run = RC.ref_run(rig, n, kind, d)
    if kind != "all_behind":
        assert fixture_ok(run)                      # (also asserted, for every case, on the CPU: tests/test_refine_ref.py)
    xr = c["xr"] if d == 4 else None
    for device in (False, True):
        X, xl, xrd = c["X"], c["xl"], xr
        if device:
            X, xl = tc.from_numpy(X).cuda(), tc.from_numpy(xl).cuda()
            xrd = tc.from_numpy(xr).cuda() if xr is not None else None
        got = stage_ctx.refine_pose(X, xl, xrd, c["P1"], c["P2"], c["rvec0"], c["t0"])
        _check_result(got, run, n, d, f"{rig} n={n} {kind} d={d} {'device' if device else 'host'}")
        assert got["iters"] <= RC.ROUNDS * RC.ITERS
        assert np.array_equal(got["pnp_rvec"], c["rvec0"]) and np.array_equal(got["pnp_tvec"], c["t0"])
        if kind == "all_behind":
            # KEPT_PNP: the PnP pose is handed back bit for bit
            assert got["status"] == RR.KEPT_PNP and got["n_active"] == 0
            assert np.array_equal(got["rvec"], c["rvec0"]) and np.array_equal(got["tvec"], c["t0"])
        elif n > 6:
            assert got["status"] == RR.APPLIED


@pytest.mark.parametrize("rig,n,kind,d", RC.DEFAULT_CASES)
def test_stage_call_equals_reference_at_default_settings(stage_ctx, tc, rig, n, kind, d):
    """svo_refine_pose with the default 4 rounds x 10 iterations.  fixture_ok cannot hold here (the Huber rounds are cut off by the
    cap from 10 cm off); these fixtures are ones on which the reference reproduces itself to a tenth of the bar instead."""
    c, run, spread = RC.default_run(rig, n, kind, d)
    assert spread <= 0.1 * TIGHT and all(e["margin"] >= 1e-6 for e in run["log"])
    stage_ctx.set_pose_refine("off")
    try:
        assert stage_ctx.pose_refine() == ("off", 4, 10, 1.0, 6)
        xr = c["xr"] if d == 4 else None
        for device in (False, True):
            args = [c["X"], c["xl"], xr]
            if device:
                args = [tc.from_numpy(a).cuda() if a is not None else None for a in args]
            got = stage_ctx.refine_pose(*args, c["P1"], c["P2"], c["rvec0"], c["t0"])
            _check_result(got, run, n, d, f"defaults {rig} n={n} d={d} {'device' if device else 'host'}")
            assert got["status"] == RR.APPLIED and got["iters"] <= 40
    finally:
        stage_ctx.set_pose_refine("off", rounds=RC.ROUNDS, iters=RC.ITERS)


def test_binding_refuses_tensors_it_would_misread(pkg, stage_ctx, tc):
    c, _ = RC.ref_run("R0", 64, "outliers", 4)
    X, xl, xr = (tc.from_numpy(c[k]).cuda() for k in ("X", "xl", "xr"))
    a = (c["P1"], c["P2"], c["rvec0"], c["t0"])
    for bad in ((X.double(), xl, xr), (X, xl.double(), xr), (X, xl, xr[::2]), (X, xl[:, [1, 0]].t().contiguous().t(), xr),
                (X, xl, xr.cpu()), (X[:10], xl, xr)):
        with pytest.raises(pkg.SvoError):
            stage_ctx.refine_pose(*bad, *a)


def test_stage_call_min_inliers_and_empty_input(stage_ctx):
    c, run = RC.ref_run("R0", 6, "outliers", 4)
    assert run["status"] == RR.APPLIED and run["n_active"] == 6
    stage_ctx.set_pose_refine("off", rounds=RC.ROUNDS, iters=RC.ITERS, min_inliers=7)
    try:
        got = stage_ctx.refine_pose(c["X"], c["xl"], c["xr"], c["P1"], c["P2"], c["rvec0"], c["t0"])
        assert got["status"] == RR.KEPT_PNP and got["n_active"] == 6
        assert np.array_equal(got["rvec"], c["rvec0"]) and np.array_equal(got["tvec"], c["t0"])
        got = stage_ctx.refine_pose(np.zeros((0, 3), np.float32), np.zeros((0, 2), np.float32), None, c["P1"], c["P2"],
                                    c["rvec0"], c["t0"])
        assert got["status"] == RR.KEPT_PNP and got["n_points"] == 0 and got["n_active"] == 0 and got["views"] == 1
    finally:
        stage_ctx.set_pose_refine("off", rounds=RC.ROUNDS, iters=RC.ITERS)


def test_setter_round_trip_and_bad_arguments(pkg):
    c = pkg.Context(416, 128, device=0)
    assert c.pose_refine() == ("off", 4, 10, 1.0, 6)                # the defaults: off
    c.set_pose_refine("reproj", rounds=3, iters=7, sigma_px=0.5, min_inliers=9)
    assert c.pose_refine() == ("reproj", 3, 7, 0.5, 9)
    for bad in (dict(mode=2), dict(mode=-1), dict(rounds=0), dict(rounds=17), dict(iters=0), dict(iters=101), dict(sigma=0.0),
                dict(sigma=-1.0), dict(sigma=float("nan")), dict(sigma=float("inf")), dict(min_inliers=0)):
        a = dict(mode=1, rounds=4, iters=10, sigma=1.0, min_inliers=6)
        a.update(bad)
        rc = c.lib.svo_set_pose_refine(c.h, a["mode"], a["rounds"], a["iters"], a["sigma"], a["min_inliers"])
        assert rc == ERR_ARG, bad
        assert c.lib.svo_last_error(c.h)
        assert c.pose_refine() == ("reproj", 3, 7, 0.5, 9), bad     # nothing changed
    with pytest.raises(pkg.SvoError):
        c.set_pose_refine("g2o")
    with pytest.raises(pkg.SvoError):
        c.refine_result(0)                                           # no fused launch yet
    c.set_pose_refine("off")
    assert c.pose_refine() == ("off", 4, 10, 1.0, 6)
    c.close()


# ---- fused steps -------------------------------------------------------------------------------------------------------
CONFIGS = {"lk_R0": ("R0", False), "lk_R3": ("R3", False), "orb_R0": ("R0", True)}
# The renderer's seed per configuration, and why fixture_ok is not what these fixtures are held to.  fixture_ok asks that every
# round of the reference's run ends through the |xi| < 1e-10 exit.  On tracked pairs (CPU oracle's tracks, 40 seeds, 120 pairs per
# configuration) it holds for 1 / 3 / 11 of 120 pairs (LK R0 / LK R3 / ORB) at the default 10 iterations, 28 / 25 / 21 at 20 and
# 81 / 72 / 42 at 40 -- so at 40 iterations 13 / 9 / 2 seeds have it on all three pairs.  But on EVERY one of those seeds it is
# lost again when the start pose moves by 1e-16 .. 1e-13 (12 starts per pair): whether the last accepted step of a round is
# shorter than 1e-10 is decided by the last bits of the PnP pose, which the GPU's LM refit shares with no CPU run.  It is a coin
# per run, not a property of the fixture, and it does not imply agreement either (seeds that have it end up to 1.7e-9 apart).
# What it is there for is asked directly, and strictly tighter than the comparison bar (_reference below): started 1e-15 .. 1e-9
# away from the PnP pose (eight starts), the reference must end within 1e-10 -- a tenth of the bar -- with the same flags.  Of the
# nine pairs of seed 11 two do not (1.1e-9 in LK mode, 4e-9 in ORB mode, for starts 1e-15 apart; the kernel differed from the
# reference by exactly those figures there).  The seeds below are the first from 11 on whose three pairs all reproduce to 2e-11
# over 24 starts up to 1e-8 away (found with the CPU oracle's tracks, which equal the GPU's bit for bit).
SEQ_SEED = {"lk_R0": 17, "lk_R3": 13, "orb_R0": 129}
ENTRIES = ("track_batch", "add_frame", "streams_step", "ingest_track_batch")
POSE_FIELDS = ("rvec", "tvec", "R", "T_rel_inv", "pose", "ok", "fail_stage")
_FRAMES, _REF = {}, {}


def _frames(synth, tc, config):
    if config not in _FRAMES:
        seq = synth.StereoSequence(width=416, height=128, n_frames=4, seed=SEQ_SEED[config], device=tc.device("cuda", 0),
                                   **_rigs.RIGS[CONFIGS[config][0]])
        _FRAMES[config] = (seq, [tuple(x.cpu().numpy() for x in seq.render(t)) for t in range(4)])
    return _FRAMES[config]


def _run_entry(c, tc, entry, frames, want_refine):
    """One pass over the 4 frames: a list of (chain id, record, tracks, refine result or None) per tracked pair, in order."""
    out = []

    def item(chain, rec, tracks, pair):
        out.append((chain, rec.copy(), tracks, c.refine_result(pair) if want_refine else None))

    if entry in ("track_batch", "ingest_track_batch"):
        L = tc.stack([tc.from_numpy(f[0]) for f in frames]).cuda()
        R = tc.stack([tc.from_numpy(f[1]) for f in frames]).cuda()
        res = c.track_batch(L, R) if entry == "track_batch" else c.ingest_track_batch(L, R)
        for p in range(3):
            item(0, res[p], c.batch_tracks(p), p)
    elif entry == "add_frame":
        c.reset()
        rc, _ = c.add_frame(*frames[0])
        assert rc == 0
        for t in range(1, 4):
            _, rec = c.add_frame(*frames[t])
            item(0, rec, c.last_tracks(), 0)
    else:
        c.streams_reset(-1)
        ids = [1, 0]
        for t in range(4):
            res = c.streams_step(ids, [frames[t][0]] * 2, [frames[t][1]] * 2)
            if t == 0:
                assert all(r["ok"] == 1 and r["n_prev_kps"] == 0 for r in res)
                if want_refine:                     # an init item has no PnP: not refined
                    assert c.refine_result(0)["status"] == RR.SKIPPED and c.refine_result(1)["n_points"] == 0
                continue
            for i in range(2):
                item(ids[i], res[i], c.streams_tracks(i), i)
    return out


def _gates(cfg, R, t, n_inliers, m):
    """finalize_pair's gates on a pose (src/tracking.cpp:491, 308, 311): the fail stage, 0 when every gate passes."""
    if n_inliers / m < cfg.inlier_rate:
        return 3
    sy = np.float32(np.sqrt(R[0, 0] * R[0, 0] + R[1, 0] * R[1, 0]))
    if float(sy) >= 1e-6:
        e = (np.arctan2(R[2, 1], R[2, 2]), np.arctan2(-R[2, 0], float(sy)), np.arctan2(R[1, 0], R[0, 0]))
    else:
        e = (np.arctan2(-R[1, 2], R[1, 1]), np.arctan2(-R[2, 0], float(sy)), 0.0)
    if not all(float(abs(np.float32(v))) < 0.1 for v in e):
        return 4
    n2 = float(t @ t)
    return 0 if (n2 < cfg.max_move2 and n2 > cfg.min_move2) else 5


def _reference(c, P1, P2, rec, tracks, orb):
    """The reference's refinement of one off-run pair: svo_triangulate of its t1 tracks, its t2 observations, its PnP pose."""
    t1l, t1r, t2r, t2l, _ = tracks
    key = (t1l.tobytes(), t1r.tobytes(), t2r.tobytes(), t2l.tobytes(), rec["R"].tobytes(), rec["tvec"].tobytes(), orb)
    if key not in _REF:
        X = c.triangulate(P1, P2, t1l, t1r)
        a = (X, t2l, None if orb else t2r, P1, P2, rec["R"].reshape(3, 3), rec["tvec"])
        run = RR.refine(*a)
        _REF[key] = (run, RC.self_spread(*a, run))
    return _REF[key]


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_fused_steps_equal_reference(pkg, synth, tc, config, entry):
    """Stage off, on, off again through one fused entry point: the off records frame the reference's inputs, the on records
    carry its refined pose (gates and chain recomputed here), everything else stays byte for byte."""
    rig, orb = CONFIGS[config]
    seq, frames = _frames(synth, tc, config)
    P1, P2 = (np.asarray(p, np.float64).reshape(3, 4) for p in seq.proj())
    kw = dict(track_mode=pkg.MODE_ORB, **ORB_KW) if orb else {}
    c = pkg.Context(416, 128, device=0, P1=P1.reshape(12), P2=P2.reshape(12), max_batch=3, **kw)
    if entry == "streams_step":
        c.streams_create(2)
    if entry == "ingest_track_batch":
        c.ingest_create(416, 128, "nearest")
    off = _run_entry(c, tc, entry, frames, False)
    with pytest.raises(pkg.SvoError):
        c.refine_result(0)                           # the stage was off for that launch
    c.set_pose_refine("reproj")
    on = _run_entry(c, tc, entry, frames, True)
    c.set_pose_refine("off")
    again = _run_entry(c, tc, entry, frames, False)
    assert len(off) == len(on) == len(again) == (6 if entry == "streams_step" else 3)
    for (_, a, ta, _), (_, b, tb, _) in zip(off, again):
        assert a.tobytes() == b.tobytes(), "switching the stage off again does not restore the records"
        assert all(x.tobytes() == y.tobytes() for x, y in zip(ta, tb))
    poses, applied = {}, 0
    for k, ((chain, a, ta, _), (_, g, tg, rr)) in enumerate(zip(off, on)):
        what = f"{config} {entry} pair {k}"
        assert a["ok"] == 1, what                    # the sequences track: nothing below is vacuous
        for name in a.dtype.names:
            if name not in POSE_FIELDS:
                assert np.asarray(a[name]).tobytes() == np.asarray(g[name]).tobytes(), (what, name)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(ta, tg)), what     # tracks and the RANSAC mask stay RANSAC's
        run, spread = _reference(c, P1, P2, a, ta, orb)
        m = len(ta[0])
        # the fixture's precondition (SEQ_SEED above): no flag hangs on a last-bit difference, and the reference reproduces itself
        assert all(e["margin"] >= 1e-6 for e in run["log"]), (what, run["log"])
        assert spread <= 0.1 * TIGHT, (what, spread)
        print(f"{what}: reference's own spread {spread:.1e}, fixture_ok {fixture_ok(run)}")
        _check_result(rr, run, m, 2 if orb else 4, what)
        assert rr["iters"] <= 4 * 10
        assert np.array_equal(rr["pnp_rvec"], a["rvec"]) and np.array_equal(rr["pnp_tvec"], a["tvec"]), what
        applied += run["status"] == RR.APPLIED
        R, t = run["R"], run["t"]
        fail = _gates(c.cfg, R, t, int(a["n_inliers"]), m)
        assert int(g["fail_stage"]) == fail and int(g["ok"]) == (fail == 0), what
        assert np.abs(g["rvec"] - run["rvec"]).max() <= TIGHT and np.abs(g["tvec"] - t).max() <= TIGHT, what
        assert np.abs(g["R"].reshape(3, 3) - R).max() <= TIGHT, what
        T = np.eye(4)
        if fail == 0:
            T[:3, :3], T[:3, 3] = R.T, -R.T @ t
        assert np.abs(g["T_rel_inv"].reshape(4, 4) - T).max() <= TIGHT, what
        poses[chain] = poses.get(chain, np.eye(4)) @ T
        assert np.abs(g["pose"].reshape(4, 4) - poses[chain]).max() <= TIGHT, what
        if run["status"] == RR.APPLIED:
            assert not np.array_equal(g["tvec"], a["tvec"]), what                 # the record really carries another pose
    print(f"{config} {entry}: {applied} of {len(on)} pairs refined")
    # LK mode hands the stage ~1000 tracks, 65-75 % of them RANSAC inliers: every pair is refined.  ORB mode's 50-90 matches
    # hold 14-22 inliers: whether enough points end active is the data's business, the comparison above holds either way
    assert orb or applied == len(on)
    c.close()


def test_timing_reports_refine_only_while_enabled(pkg, synth, tc):
    seq, frames = _frames(synth, tc, "lk_R0")
    P1, P2 = seq.proj()
    c = pkg.Context(416, 128, device=0, P1=P1, P2=P2, max_batch=3)
    c.enable_timing(True)
    _run_entry(c, tc, "track_batch", frames, False)
    assert "refine" not in dict(c.get_timing())
    c.set_pose_refine("reproj")
    _run_entry(c, tc, "track_batch", frames, True)
    t = dict(c.get_timing())
    assert "refine" in t and "pnp" in t and t["refine"] > 0
    c.close()
