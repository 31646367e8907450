"""The pose stage's bundle-adjustment mode on the GPU (svo_set_pose_refine_ba / svo_refine_ba /
svo_get_refine_points, csrc/ba.hip) against tests/_ba_ref.py, the numpy twin of its rules.

Bars, as tests/test_gpu_refine.py: status, n_active and the active flags equal; rvec / tvec / R and the points within 1e-9
absolute (TIGHT); info within 1e-9 of its largest entry and symmetric; the iteration count only bounded.  Every fixture is one
on which the twin reproduces itself to a tenth of that bar and on which no classification or accept decision is near a tie
(tests/test_ba_ref.py checks the stage-call fixtures on the CPU, the fused test its own pairs here): the runs are rounds of two
iterations, because from the third step of a round on the accept test is decided by rounding and a far point's depth, a flat
direction of the cost, is reproducible to ~1e-7 m only (_ba_cases.ROUNDS)."""
import numpy as np
import pytest

import _ba_cases as BC
import _ba_ref as BA
import _refine_ref as RR
from test_gpu_parity_pose import TIGHT
from test_gpu_refine import CONFIGS, ORB_KW, POSE_FIELDS, _frames, _gates

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tc():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def stage_ctx(pkg):
    c = pkg.Context(416, 128, device=0, max_keypoints=4096)
    c.set_pose_refine("off", **BC.settings(64))                     # the stage call uses the settings whatever the mode
    yield c
    c.close()


def _check_result(got, X, run, n, d, what="", pose_bar=TIGHT, point_bar=TIGHT, info_bar=TIGHT):
    """A GPU record and its points against a twin run."""
    dx = np.abs(X - run["X"]).max() if n else 0.0
    print(f"{what}: status {got['status']} active {got['n_active']}/{n} iters {got['iters']} (twin {run['iters']}) "
          f"|dt| {np.abs(got['tvec'] - run['t']).max():.1e} |dr| {np.abs(got['rvec'] - run['rvec']).max():.1e} |dX| {dx:.1e} "
          f"twin exits {[e['exit'] for e in run['log']]}")
    assert got["status"] == run["status"] and got["n_points"] == n and got["views"] == d // 2 - 2, what
    assert got["n_active"] == run["n_active"] and np.array_equal(got["active"], run["active"]), what
    assert np.abs(got["rvec"] - run["rvec"]).max() <= pose_bar, what
    assert np.abs(got["tvec"] - run["t"]).max() <= pose_bar, what
    assert np.abs(got["R"] - run["R"]).max() <= pose_bar, what
    assert X.shape == (n, 3) and X.dtype == np.float64 and dx <= point_bar, what
    top = np.abs(run["info"]).max()
    assert np.abs(got["info"] - run["info"]).max() <= info_bar * top, what
    assert np.array_equal(got["info"], got["info"].T), what
    for k in ("cost_first", "cost_last"):
        assert abs(got[k] - run[k]) <= TIGHT * max(1.0, abs(run[k])), (what, k)


def _stage_args(c, d):
    return [c["X0"], c["x1l"], c["x1r"], c["xl"], c["xr"] if d == 8 else None]


@pytest.mark.parametrize("rig,n,kind,d", BC.stage_cases())
def test_stage_call_equals_twin(stage_ctx, tc, rig, n, kind, d):
    """svo_refine_ba on host and on device inputs: 30 % outliers, some points behind the camera, all points behind it."""
    c, run = BC.ref_run(rig, n, kind, d)
    kw = BC.settings(n)
    stage_ctx.set_pose_refine("off", **kw)
    for device in (False, True):
        args = _stage_args(c, d)
        if device:
            args = [tc.from_numpy(a).cuda() if a is not None else None for a in args]
        got = stage_ctx.refine_ba(*args, c["P1"], c["P2"], c["rvec0"], c["t0"])
        _check_result(got, got["X"], run, n, d, f"{rig} n={n} {kind} d={d} {'device' if device else 'host'}")
        assert got["iters"] <= kw["rounds"] * kw["iters"]
        assert np.array_equal(got["pnp_rvec"], c["rvec0"]) and np.array_equal(got["pnp_tvec"], c["t0"])
        inactive = got["active"] == 0
        assert np.array_equal(got["X"][inactive], c["X0"][inactive].astype(np.float64))      # never moved, or returned
        if kind == "all_behind":
            # KEPT_PNP: the PnP pose is handed back bit for bit
            assert got["status"] == RR.KEPT_PNP and got["n_active"] == 0
            assert np.array_equal(got["rvec"], c["rvec0"]) and np.array_equal(got["tvec"], c["t0"])
        elif n > 6:
            assert got["status"] == RR.APPLIED


def _stage_both(stage_ctx, tc, c, d, run, what, **bars):
    """svo_refine_ba on host and on device inputs against one twin run; the GPU records."""
    out = []
    for device in (False, True):
        args = _stage_args(c, d)
        if device:
            args = [tc.from_numpy(a).cuda() if a is not None else None for a in args]
        got = stage_ctx.refine_ba(*args, c["P1"], c["P2"], c["rvec0"], c["t0"])
        _check_result(got, got["X"], run, len(c["X0"]), d, f"{what} d={d} {'device' if device else 'host'}", **bars)
        out.append(got)
    return out


@pytest.mark.parametrize("d", [6, 8])
def test_stage_call_rejects_a_step_and_retries(stage_ctx, tc, d):
    """The reject branch of the LM loop: from 1 m and 3 degrees off a step raises the cost by a tenth of itself or more (d = 6:
    the first one, at lambda = 1e-4), is discarded -- the trial buffer holds it, the accepted points stand -- and the retry at
    10 lambda is accepted (tests/test_ba_ref.py asserts that of the twin's run).  Every decision is far from a tie, so the
    iteration count is compared too."""
    c = BC.far_case(d)
    run = BC.run_twin(c, d, **BC.FAR_KW)
    assert "rejected" in [s[0] for s in run["log"][0]["steps"]]
    stage_ctx.set_pose_refine("off", **BC.FAR_KW)
    try:
        for got in _stage_both(stage_ctx, tc, c, d, run, "far start"):
            assert got["iters"] == run["iters"] == 4 and got["status"] == RR.APPLIED
    finally:
        stage_ctx.set_pose_refine("off", **BC.settings(64))


@pytest.mark.parametrize("d", [6, 8])
def test_stage_call_ends_through_the_short_step_exit(stage_ctx, tc, d):
    """The |xi| < 1e-10, max |dX| < 1e-9 exit (and with it the max |dX| reduction across lanes and waves, which feeds nothing
    else): on the scene with exact pixels the round ends after four accepted steps of a cap of twelve, as the twin's does."""
    c = BC.exact_case()
    run = BC.run_twin(c, d, **BC.EXACT_KW)
    assert run["log"][0]["exit"] == "xi" and run["iters"] == 4
    stage_ctx.set_pose_refine("off", **BC.EXACT_KW)
    try:
        for got in _stage_both(stage_ctx, tc, c, d, run, "exact pixels"):
            assert got["iters"] == 4 and got["status"] == RR.APPLIED and got["n_active"] == 70
            assert np.abs(got["tvec"] - c["t_true"]).max() <= TIGHT and np.abs(got["X"] - c["X0"]).max() <= TIGHT
    finally:
        stage_ctx.set_pose_refine("off", **BC.settings(64))


@pytest.mark.parametrize("rig,n,kind,d", BC.DEFAULT_CASES)
def test_stage_call_at_default_settings(stage_ctx, tc, rig, n, kind, d):
    """4 rounds x 10 iterations, where the last steps of a round are ties that rounding decides: status and flags equal, pose,
    points and info within bars of ten times the twin's own spread over eight starts (_ba_cases.DEFAULT_*_BAR: 2e-9, 2e-6,
    2e-6 relative; measured 1.8e-10, 1.5e-7; tests/test_ba_ref.py asserts the spread on these very fixtures)."""
    c, run = BC.default_run(rig, n, kind, d)
    stage_ctx.set_pose_refine("off")
    try:
        assert stage_ctx.pose_refine() == ("off", 4, 10, 1.0, 6)
        for got in _stage_both(stage_ctx, tc, c, d, run, f"defaults {rig} n={n}", pose_bar=BC.DEFAULT_POSE_BAR,
                               point_bar=BC.DEFAULT_POINT_BAR, info_bar=BC.DEFAULT_INFO_BAR):
            assert got["status"] == RR.APPLIED and got["iters"] <= 40
    finally:
        stage_ctx.set_pose_refine("off", **BC.settings(64))


def test_stage_call_min_inliers_and_empty_input(stage_ctx):
    c, run = BC.ref_run("R0", 6, "outliers", 8)
    assert run["status"] == RR.APPLIED and run["n_active"] == 6
    stage_ctx.set_pose_refine("off", min_inliers=7, **BC.settings(6))                         # n + 1
    try:
        got = stage_ctx.refine_ba(*_stage_args(c, 8), c["P1"], c["P2"], c["rvec0"], c["t0"])
        assert got["status"] == RR.KEPT_PNP and got["n_active"] == 6
        assert np.array_equal(got["rvec"], c["rvec0"]) and np.array_equal(got["tvec"], c["t0"])
        assert np.abs(got["R"] - RR.rodrigues(c["rvec0"])).max() <= TIGHT
        assert np.array_equal(got["X"], c["X0"].astype(np.float64))                            # ... and the triangulation with it
        z3, z2 = np.zeros((0, 3), np.float32), np.zeros((0, 2), np.float32)
        for x2r, views in ((z2, 2), (None, 1)):
            got = stage_ctx.refine_ba(z3, z2, z2, z2, x2r, c["P1"], c["P2"], c["rvec0"], c["t0"])
            assert got["status"] == RR.KEPT_PNP and got["n_points"] == 0 and got["n_active"] == 0 and got["views"] == views
            assert got["X"].shape == (0, 3)
            assert np.array_equal(got["rvec"], c["rvec0"]) and np.array_equal(got["tvec"], c["t0"])
    finally:
        stage_ctx.set_pose_refine("off", **BC.settings(64))


def test_binding_refuses_tensors_it_would_misread(pkg, stage_ctx, tc):
    """What test_gpu_refine.py's test of the same name lists, for each of the observation arrays, the two new ones included."""
    c, _ = BC.ref_run("R0", 64, "outliers", 8)
    stage_ctx.set_pose_refine("off", **BC.settings(64))
    good = [tc.from_numpy(a).cuda() for a in _stage_args(c, 8)]
    a = (c["P1"], c["P2"], c["rvec0"], c["t0"])
    assert stage_ctx.refine_ba(*good, *a)["n_points"] == 64
    bad_obj = [good[0].double(), good[0][:10]]
    for bad in bad_obj:
        with pytest.raises(pkg.SvoError):
            stage_ctx.refine_ba(bad, *good[1:], *a)
    for k in (1, 2, 3, 4):
        x = good[k]
        for bad in (x.double(), x[::2], x[:, [1, 0]].t().contiguous().t(), x.cpu(), x[:10]):
            args = list(good)
            args[k] = bad
            with pytest.raises(pkg.SvoError):
                stage_ctx.refine_ba(*args, *a)
    for k in (1, 2, 3):                              # only img2_right may be absent
        args = list(good)
        args[k] = None
        with pytest.raises(pkg.SvoError):
            stage_ctx.refine_ba(*args, *a)


def test_setter_accepts_and_reports_ba(pkg):
    c = pkg.Context(416, 128, device=0)
    c.set_pose_refine("ba", rounds=3, iters=7, sigma_px=0.5, min_inliers=9)
    assert c.pose_refine() == ("ba", 3, 7, 0.5, 9)
    for mode in (2, 3):                              # svo_set_pose_refine itself goes on refusing every mode but OFF and REPROJ
        assert c.lib.svo_set_pose_refine(c.h, mode, 4, 10, 1.0, 6) == -1 and c.pose_refine() == ("ba", 3, 7, 0.5, 9)
    for bad in (dict(rounds=0), dict(rounds=17), dict(iters=0), dict(iters=101), dict(sigma=0.0), dict(min_inliers=0)):
        a = dict(rounds=4, iters=10, sigma=1.0, min_inliers=6)
        a.update(bad)
        assert c.lib.svo_set_pose_refine_ba(c.h, a["rounds"], a["iters"], a["sigma"], a["min_inliers"]) == -1, bad
        assert c.pose_refine() == ("ba", 3, 7, 0.5, 9), bad
    with pytest.raises(pkg.SvoError):
        c.refine_points(0)                           # no fused launch yet
    c.set_pose_refine("off")
    assert c.pose_refine() == ("off", 4, 10, 1.0, 6)
    c.close()


# ---- fused steps -------------------------------------------------------------------------------------------------------
ENTRIES = ("track_batch", "track_batch_overlap", "add_frame", "streams_step")
# The ba mode's settings in these tests: the two Huber rounds, two iterations each.  A tracked pair starts at the PnP pose,
# within the noise of the optimum already: measured on these sequences, the steps of rounds 0 and 1 change the cost by 1e-2 ..
# 1e-4 of itself, those of a third and fourth round by 1e-7 .. 1e-14 -- ties that rounding decides (_ba_cases.ROUNDS).  The
# reproj mode keeps its defaults.
FUSED_KW = dict(rounds=2, iters=BC.ITERS)
_REF = {}


def _run_entry(pkg, c, tc, entry, frames, mode):
    """One pass over the 4 frames: (chain id, record, tracks, refine result or None, points or None) per tracked pair."""
    out = []

    def item(chain, rec, tracks, pair):
        rr = c.refine_result(pair) if mode != "off" else None
        out.append((chain, rec.copy(), tracks, rr, c.refine_points(pair) if mode == "ba" else None))

    if entry in ("track_batch", "track_batch_overlap"):
        L = tc.stack([tc.from_numpy(f[0]) for f in frames]).cuda()
        R = tc.stack([tc.from_numpy(f[1]) for f in frames]).cuda()
        if entry == "track_batch":
            res = c.track_batch(L, R)
        else:
            dres = tc.zeros((3, pkg.STEP_DTYPE.itemsize), dtype=tc.uint8, device="cuda")
            c.track_batch(L, R, results=dres)
            c.sync()
            res = np.frombuffer(dres.cpu().numpy().tobytes(), dtype=pkg.STEP_DTYPE)
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
                if mode == "ba":                     # an init item has no PnP: nothing adjusted, no points
                    assert c.refine_result(0)["status"] == RR.SKIPPED and c.refine_points(1).shape == (0, 3)
                continue
            for i in range(2):
                item(ids[i], res[i], c.streams_tracks(i), i)
    return out


def _twin(c, P1, P2, rec, tracks, orb):
    """The twin's adjustment of one off-run pair: svo_triangulate of its t1 tracks, all its observations, its PnP pose."""
    t1l, t1r, t2r, t2l, _ = tracks
    key = (t1l.tobytes(), t1r.tobytes(), t2r.tobytes(), t2l.tobytes(), rec["R"].tobytes(), rec["tvec"].tobytes(), orb)
    if key not in _REF:
        X = c.triangulate(P1, P2, t1l, t1r)
        a = (X, t1l, t1r, t2l, None if orb else t2r, P1, P2, rec["R"].reshape(3, 3))
        run = BA.refine_ba(*a, rec["tvec"], **FUSED_KW)
        again = BA.refine_ba(*a, rec["tvec"] + 1e-15 * np.random.default_rng(1).standard_normal(3), **FUSED_KW)
        same = np.array_equal(run["active"], again["active"]) and run["status"] == again["status"]
        spread = max(np.abs(run["t"] - again["t"]).max(), np.abs(run["rvec"] - again["rvec"]).max(),
                     np.abs(run["X"] - again["X"]).max()) if same else np.inf
        _REF[key] = (run, spread)
    return _REF[key]


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_fused_steps_equal_twin(pkg, synth, tc, config, entry):
    """off -> ba -> reproj -> off through one fused entry point.  The off records frame the twin's inputs; the ba records carry
    its adjusted pose (gates and chain recomputed here) and refine_points its points; everything else stays byte for byte; and
    in off and reproj the context gives what a context that never saw the ba mode gives."""
    rig, orb = CONFIGS[config]
    seq, frames = _frames(synth, tc, config)
    P1, P2 = (np.asarray(p, np.float64).reshape(3, 4) for p in seq.proj())
    kw = dict(track_mode=pkg.MODE_ORB, **ORB_KW) if orb else {}

    def make():
        c = pkg.Context(416, 128, device=0, P1=P1.reshape(12), P2=P2.reshape(12), max_batch=3, **kw)
        if entry == "streams_step":
            c.streams_create(2)
        if entry == "track_batch_overlap":
            c.set_overlap(True)
        return c

    c = make()
    runs = {}
    for mode in ("off", "ba", "reproj", "off again"):
        c.set_pose_refine(mode.split()[0], **(FUSED_KW if mode == "ba" else {}))
        runs[mode] = _run_entry(pkg, c, tc, entry, frames, mode.split()[0])
        if mode != "ba":
            with pytest.raises(pkg.SvoError):
                c.refine_points(0)                   # that launch was not made in ba mode
    f = make()
    fresh = {"off": _run_entry(pkg, f, tc, entry, frames, "off")}
    f.set_pose_refine("reproj")
    fresh["reproj"] = _run_entry(pkg, f, tc, entry, frames, "reproj")
    f.close()
    off, on = runs["off"], runs["ba"]
    assert len(off) == len(on) == (6 if entry == "streams_step" else 3)
    for mode, ref in (("off", fresh["off"]), ("off again", fresh["off"]), ("reproj", fresh["reproj"])):
        for (_, a, ta, ra, _), (_, b, tb, rb, _) in zip(runs[mode], ref):
            assert a.tobytes() == b.tobytes(), f"{mode}: the records differ from a fresh context's"
            assert all(x.tobytes() == y.tobytes() for x, y in zip(ta, tb)), mode
            if ra is not None:
                assert all(np.asarray(ra[k]).tobytes() == np.asarray(rb[k]).tobytes() for k in ra), mode
    poses, applied = {}, 0
    for k, ((chain, a, ta, _, _), (_, g, tg, rr, X)) in enumerate(zip(off, on)):
        what = f"{config} {entry} pair {k}"
        assert a["ok"] == 1, what                    # the sequences track: nothing below is vacuous
        for name in a.dtype.names:
            if name not in POSE_FIELDS:
                assert np.asarray(a[name]).tobytes() == np.asarray(g[name]).tobytes(), (what, name)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(ta, tg)), what     # tracks and the RANSAC mask stay RANSAC's
        run, spread = _twin(c, P1, P2, a, ta, orb)
        m = len(ta[0])
        print(f"{what}: twin's own spread {spread:.1e}, log {run['log']}")
        # the fixture's precondition: no decision hangs on a last-bit difference, and the twin reproduces itself
        assert all(e["margin"] >= 1e-6 and e["accept_margin"] >= 1e-6 for e in run["log"]), (what, run["log"])
        assert spread <= 0.1 * TIGHT, (what, spread)
        _check_result(rr, X, run, m, 6 if orb else 8, what)
        assert rr["iters"] <= FUSED_KW["rounds"] * FUSED_KW["iters"]
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
    print(f"{config} {entry}: {applied} of {len(on)} pairs adjusted")
    assert orb or applied == len(on)
    c.close()



# Measured with the twin alone on the three pairs of the lk_R0 sequence (the CPU oracle's tracks, which equal the GPU's), four
# starts 1e-15 .. 1e-9 apart, at the default 4 x 10: flags equal; tvec up to 1.1e-9, rvec 5.9e-11, points 1.7e-7 apart.  The
# bars are ten times that.
FUSED_DEFAULT_POSE_BAR, FUSED_DEFAULT_POINT_BAR, FUSED_DEFAULT_INFO_BAR = 1e-8, 2e-6, 2e-6


def test_fused_steps_at_default_settings(pkg, synth, tc):
    """svo_track_batch in ba mode at the default 4 rounds x 10 iterations against the twin fed the off run's tracks and PnP
    records: status and flags equal; records, refine_result and refine_points within the bars above."""
    seq, frames = _frames(synth, tc, "lk_R0")
    P1, P2 = (np.asarray(p, np.float64).reshape(3, 4) for p in seq.proj())
    c = pkg.Context(416, 128, device=0, P1=P1.reshape(12), P2=P2.reshape(12), max_batch=3)
    off = _run_entry(pkg, c, tc, "track_batch", frames, "off")
    c.set_pose_refine("ba")
    assert c.pose_refine() == ("ba", 4, 10, 1.0, 6)
    on = _run_entry(pkg, c, tc, "track_batch", frames, "ba")
    for k, ((_, a, ta, _, _), (_, g, tg, rr, X)) in enumerate(zip(off, on)):
        what = f"defaults lk_R0 track_batch pair {k}"
        assert a["ok"] == 1 and all(x.tobytes() == y.tobytes() for x, y in zip(ta, tg)), what
        t1l, t1r, t2r, t2l, _ = ta
        run = BA.refine_ba(c.triangulate(P1, P2, t1l, t1r), t1l, t1r, t2l, t2r, P1, P2, a["R"].reshape(3, 3), a["tvec"])
        assert all(e["margin"] >= 1e-6 for e in run["log"]), (what, run["log"])
        _check_result(rr, X, run, len(t1l), 8, what, pose_bar=FUSED_DEFAULT_POSE_BAR, point_bar=FUSED_DEFAULT_POINT_BAR,
                      info_bar=FUSED_DEFAULT_INFO_BAR)
        assert rr["status"] == RR.APPLIED and rr["iters"] <= 40
        assert np.abs(g["rvec"] - run["rvec"]).max() <= FUSED_DEFAULT_POSE_BAR, what
        assert np.abs(g["tvec"] - run["t"]).max() <= FUSED_DEFAULT_POSE_BAR, what
        assert np.abs(g["R"].reshape(3, 3) - run["R"]).max() <= FUSED_DEFAULT_POSE_BAR, what
    c.close()
