"""The numpy twin of the bundle-adjustment mode (tests/_ba_ref.py) checked against mathematics and
against scipy: it is the reference of tests/test_gpu_ba.py, the oracle has no such stage."""
import numpy as np
import pytest
from scipy.optimize import least_squares

import _ba_cases as BC
import _ba_ref as BA
import _refine_cases as RC
import _refine_ref as RR
import _rigs
from test_gpu_parity_pose import TIGHT


def _scene(n, seed, rig):
    rng = np.random.default_rng(seed)
    P1, P2 = (np.asarray(p, np.float64).reshape(3, 4) for p in _rigs.matrices(rig))
    X = np.stack([rng.uniform(-8, 8, n), rng.uniform(-3, 3, n), rng.uniform(5, 40, n)], 1).astype(np.float32).astype(np.float64)
    return rng, P1, P2, X


def _observe(P1, P2, X, R, t):
    """Exact pixels of X in the four images: t1_left, t1_right, t2_left, t2_right."""
    out = []
    for Z in (X, X @ R.T + t):
        for M, p4 in BA.views_of(P1, P2):
            h = Z @ M.T + p4
            out.append(h[:, :2] / h[:, 2:3])
    return out


def _residuals(p, obs, views, R0, t0):
    """All residuals as a function of (xi, X): the pose is exp(xi) (R0, t0)."""
    E, Vr = RR.se3_exp(p[:6])
    r, _, proj, _, _ = BA.evaluate(p[6:].reshape(-1, 3), obs, views, E @ R0, E @ t0 + Vr)
    assert proj.all()
    return r.ravel()


def _jacobian(p, obs, views, R0, t0):
    """The dense Jacobian of _residuals from the twin's analytic blocks (at xi = 0 relative to the pose p stands for: the
    pose columns are those of a further left-multiplied exp(xi'), which is what a solver needs at a stationary point)."""
    E, Vr = RR.se3_exp(p[:6])
    _, _, _, Jx, Jp = BA.evaluate(p[6:].reshape(-1, 3), obs, views, E @ R0, E @ t0 + Vr)
    n, d = Jx.shape[:2]
    J = np.zeros((n * d, 6 + 3 * n))
    for i in range(n):
        J[i * d:(i + 1) * d, :6] = Jp[i]
        J[i * d:(i + 1) * d, 6 + 3 * i:9 + 3 * i] = Jx[i]
    return J


@pytest.mark.parametrize("d", [6, 8])
def test_jacobians_match_central_differences(d):
    rng, P1, P2, X = _scene(12, 3, "R3")
    R, t = RC.true_pose()
    obs = [o + rng.standard_normal(o.shape) for o in _observe(P1, P2, X, R, t)][:d // 2]
    views = BA.views_of(P1, P2)
    _, _, proj, Jx, Jp = BA.evaluate(X, obs, views, R, t)
    assert proj.all() and not Jp[:, :4].any()
    p0, eps = np.concatenate([np.zeros(6), X.ravel()]), 1e-6
    for k in range(6 + 3):
        num = np.zeros((12, d))
        for i in range(12 if k >= 6 else 1):           # the pose columns in one go, a point's columns point by point
            dp = np.zeros_like(p0)
            dp[k if k < 6 else 6 + 3 * i + (k - 6)] = eps
            diff = ((_residuals(p0 + dp, obs, views, R, t) - _residuals(p0 - dp, obs, views, R, t)) / (2 * eps)).reshape(12, d)
            if k < 6:
                num = diff
            else:
                num[i] = diff[i]
        J = Jp[:, :, k] if k < 6 else Jx[:, :, k - 6]
        # central differences: truncation ~1e-9, rounding |r| 2^-52 / eps ~ 1e-7 for |r| ~ 1e3 px
        assert np.abs(num - J).max() <= 1e-6 * max(1.0, np.abs(J).max()), k


@pytest.mark.parametrize("d", [6, 8])
def test_noiseless_data_recover_the_pose_and_leave_the_points(d):
    _, P1, P2, X = _scene(80, 11, "R3")
    R, t = RC.true_pose()
    o = _observe(P1, P2, X, R, t)
    R0, t0 = RC.start_pose()
    run = BA.refine_ba(X, o[0], o[1], o[2], o[3] if d == 8 else None, P1, P2, R0, t0)
    assert run["status"] == BA.APPLIED and run["n_active"] == 80 and run["views"] == d // 2 - 2
    assert np.abs(run["R"] - R).max() < 1e-9 and np.abs(run["t"] - t).max() < 1e-9
    assert np.abs(run["X"] - X).max() < 1e-9
    assert run["iters"] <= 4 * 10 and run["cost_last"] < 1e-12 < run["cost_first"]


def _clean_case(d):
    c = BC.make_case("R0", 64, "outliers", seed=BC.SEED0 + 7, noise=0.3)
    c2 = RC.make_case("R0", 64, "outliers", seed=BC.SEED0 + 7, outlier_share=0.0)          # the same draw without the gross outliers
    c.update(xl=c2["xl"], xr=c2["xr"])
    return c


@pytest.mark.parametrize("d", [6, 8])
def test_optimum_equals_scipy_least_squares(d):
    """On a clean 64-point case every point ends active, so the last (plain) rounds minimise sum |r|^2: the optimum of
    scipy.optimize.least_squares on the same residuals over (xi, X), run to convergence from the twin's start.
    Measured, twin against scipy ('lm' with the analytic Jacobian, xtol = ftol = gtol = 1e-15): pose 5.6e-15 / 1.9e-12
    (d = 6 / 8), points 5.7e-12 / 1.0e-8 -- the depth of a far point is a flat direction (d^2 cost / dz^2 ~ 0.1 at 40 m) in
    which either solver stops where the cost no longer changes in double, ~1e-8; the bars are ten times the larger figure of
    each.  (With scipy's finite-difference Jacobian the figures are 1.7e-8 and 1.6e-6: its error, not the twin's.)"""
    c = _clean_case(d)
    run = BC.run_twin(c, d, rounds=6, iters=30)
    assert run["status"] == BA.APPLIED and run["active"].all()
    obs = [np.asarray(c[k], np.float64) for k in ("x1l", "x1r", "xl", "xr")][:d // 2]
    views = BA.views_of(c["P1"], c["P2"])
    R0 = RR.rodrigues(c["rvec0"])
    p0 = np.concatenate([np.zeros(6), c["X0"].astype(np.float64).ravel()])
    sol = least_squares(_residuals, p0, args=(obs, views, R0, c["t0"]), jac=_jacobian, method="lm", xtol=1e-15, ftol=1e-15, gtol=1e-15, max_nfev=20000)
    E, Vr = RR.se3_exp(sol.x[:6])
    dpose = max(np.abs(E @ R0 - run["R"]).max(), np.abs(E @ c["t0"] + Vr - run["t"]).max())
    dX = np.abs(sol.x[6:].reshape(-1, 3) - run["X"]).max()
    print(f"d = {d}: twin against scipy: pose {dpose:.1e}, points {dX:.1e}; cost {run['cost_last']:.12g} vs {2 * sol.cost:.12g}")
    assert dpose <= 2e-11 and dX <= 1e-7
    assert run["cost_last"] <= 2 * sol.cost * (1 + 1e-12)


@pytest.mark.parametrize("d", [6, 8])
def test_info_is_the_schur_complement_of_the_full_normal_matrix(d):
    """info against the dense route: the full (6 + 3 n)^2 matrix J^T J over the active points, assembled from the residuals'
    Jacobian, and numpy's Schur complement of its point block."""
    c, run = BC.ref_run("R3", 65, "outliers", d)
    obs = [np.asarray(c[k], np.float64) for k in ("x1l", "x1r", "xl", "xr")][:d // 2]
    act = run["active"] == 1
    X = run["X_ref"][act]
    _, _, proj, Jx, Jp = BA.evaluate(X, [o[act] for o in obs], BA.views_of(c["P1"], c["P2"]), run["R_ref"], run["t_ref"])
    m = int(act.sum())
    assert proj.all() and m == run["n_active"] > 20
    J = np.zeros((m * d, 6 + 3 * m))
    for i in range(m):
        J[i * d:(i + 1) * d, :6] = Jp[i]
        J[i * d:(i + 1) * d, 6 + 3 * i:9 + 3 * i] = Jx[i]
    N = J.T @ J
    S = N[:6, :6] - N[:6, 6:] @ np.linalg.solve(N[6:, 6:], N[6:, :6])
    assert np.abs(run["info"] - S).max() <= 1e-9 * np.abs(S).max()
    assert np.abs(run["info"] - run["info"].T).max() <= 1e-12 * np.abs(S).max()
    # eliminating the points can only take information away from the pose
    full = Jp.reshape(-1, 6).T @ Jp.reshape(-1, 6)
    assert np.linalg.eigvalsh(full - run["info"]).min() >= -1e-9 * np.abs(full).max()


def test_outliers_end_inactive_and_return_to_their_triangulation():
    c, run = BC.ref_run("R0", 257, "outliers", 8)
    assert run["status"] == BA.APPLIED
    assert (run["active"][c["outlier"]] == 0).all() and (run["active"][~c["outlier"]] == 1).all()
    assert np.array_equal(run["X"][c["outlier"]], c["X0"][c["outlier"]].astype(np.float64))
    assert np.abs(run["t"] - c["t_true"]).max() < 0.02 and np.abs(run["R"] - c["R_true"]).max() < 1e-3
    moved = np.abs(run["X"][~c["outlier"]] - c["X0"][~c["outlier"]]).max(1)
    assert (moved > 0).all()


@pytest.mark.parametrize("d", [6, 8])
def test_all_points_behind_the_camera_keep_pnp(d):
    c, run = BC.ref_run("R0", 64, "all_behind", d)
    assert run["status"] == BA.KEPT_PNP and run["n_active"] == 0 and not run["active"].any()
    assert np.array_equal(run["t"], c["t0"]) and np.array_equal(run["R"], RR.rodrigues(c["rvec0"]))
    assert not run["info"].any() and np.array_equal(run["X"], c["X0"].astype(np.float64))


@pytest.mark.parametrize("rig,n,kind,d", BC.stage_cases())
def test_gpu_fixtures_meet_the_precondition(rig, n, kind, d):
    """Every fixture tests/test_gpu_ba.py hands to svo_refine_ba: started 1e-15 apart the twin reproduces itself to a tenth of
    the comparison bar, and no classification or accept decision hangs on the rounding (_ba_cases.fixture_ok)."""
    c, run = BC.ref_run(rig, n, kind, d)
    if kind == "all_behind":
        assert run["status"] == BA.KEPT_PNP and run["n_active"] == 0       # nothing is projectable: no decision depends on rounding
        return
    spread = BC.ref_spread(rig, n, kind, d)
    assert BC.fixture_ok(run, spread, TIGHT), (spread, run["log"])
    clean = ~c["outlier"] & ~c["behind"]
    assert (run["active"][clean] == 1).all() and not run["active"][~clean].any()
    assert run["iters"] <= BC.ROUNDS * BC.ITERS


def test_translation_bias_of_both_modes_is_reported():
    """Monte Carlo over the noise: the mean SIGNED error of the forward translation (t_z, true value -0.85 m) of the reproj twin
    (points held at their noisy triangulation) and of the ba twin on the same draws.  Printed, not asserted: whether holding
    the points fixed biases the translation is what the figure is for."""
    err = {"reproj": [], "ba": []}
    for k in range(24):
        c = BC.make_case("R0", 150, "outliers", seed=BC.SEED0 + 5000 + k)
        R0 = RR.rodrigues(c["rvec0"])
        a = RR.refine(c["X0"], c["xl"], c["xr"], c["P1"], c["P2"], R0, c["t0"])
        b = BA.refine_ba(c["X0"], c["x1l"], c["x1r"], c["xl"], c["xr"], c["P1"], c["P2"], R0, c["t0"])
        assert a["status"] == RR.APPLIED and b["status"] == BA.APPLIED
        err["reproj"].append(a["t"] - c["t_true"])
        err["ba"].append(b["t"] - c["t_true"])
    for k, v in err.items():
        v = np.array(v)
        print(f"{k:6s}: mean signed t error {v.mean(0)} m, its standard error {v.std(0, ddof=1) / np.sqrt(len(v))}, "
              f"rms {np.sqrt((v * v).sum(1).mean()):.4f} m")


# ---- the fixtures of tests/test_gpu_ba.py that take the reject branch, the short-step exit and the default settings ----------
@pytest.mark.parametrize("d", [6, 8])
def test_far_start_fixture_rejects_a_step_decisively(d):
    """One round of four iterations from 1 m and 3 degrees off: a step is rejected because the cost rises by a tenth of itself
    or more (d = 6: the first step, at lambda = 1e-4), the retry is accepted, no decision is near a tie, and started 1e-15
    apart the twin reproduces itself to a tenth of the bar (the run is not converged: a start 1e-9 away ends 3e-9 away)."""
    c = BC.far_case(d)
    run = BC.run_twin(c, d, **BC.FAR_KW)
    # (the decisions the cost takes: the log also names the trial -- the third of d = 6, the second of d = 8 -- that is rejected
    # before the cost is asked, because a point is not projectable at it)
    steps = [s for s in run["log"][0]["steps"] if s[0] != "unprojectable"]
    assert len(steps) == 3 and len(run["log"][0]["steps"]) == 4
    k = [s[0] for s in steps].index("rejected")
    assert k == (0 if d == 6 else 1) and steps[k + 1][0] == "accepted"
    assert all(m >= 0.1 for _, m in steps) and run["log"][0]["margin"] >= 1e-6
    assert run["status"] == BA.APPLIED and run["iters"] == 4 and run["log"][0]["exit"] == "iters"
    assert BC.self_spread(c, d, run, starts=(1e-15, 1e-14), per=2, **BC.FAR_KW) <= 0.1 * TIGHT


@pytest.mark.parametrize("d", [6, 8])
def test_exact_fixture_ends_through_the_short_step_exit(d):
    """The scene with exact pixels: four accepted steps, each lowering the cost by more than 0.999 of itself, the last one short
    -- the round ends through the |xi| < 1e-10, max |dX| < 1e-9 exit well before its cap of 12; the same from eight other
    starts; the true pose and the points are recovered to 1e-12."""
    c = BC.exact_case()
    run = BC.run_twin(c, d, **BC.EXACT_KW)
    assert run["log"][0]["exit"] == "xi" and run["iters"] == 4 and run["status"] == BA.APPLIED and run["n_active"] == 70
    assert [s[0] for s in run["log"][0]["steps"]] == ["accepted"] * 4 and all(m > 0.999 for _, m in run["log"][0]["steps"])
    assert np.abs(run["t"] - c["t_true"]).max() < 1e-12 and np.abs(run["X"] - c["X0"]).max() < 1e-12
    rng = np.random.default_rng(2)
    for eps in (1e-15, 1e-13, 1e-11, 1e-9):
        for _ in range(2):
            r = BC.run_twin(c, d, t0=c["t0"] + eps * rng.standard_normal(3), **BC.EXACT_KW)
            assert r["iters"] == 4 and r["log"][0]["exit"] == "xi"
    assert BC.self_spread(c, d, run, starts=(1e-15, 1e-12, 1e-9), per=2, **BC.EXACT_KW) <= 0.1 * TIGHT


@pytest.mark.parametrize("rig,n,kind,d", BC.DEFAULT_CASES)
def test_default_setting_fixtures_spread_is_what_the_bars_assume(rig, n, kind, d):
    """4 rounds x 10 iterations: eight starts 1e-15 .. 1e-9 apart end with the same flags and status, and a tenth of
    _ba_cases.DEFAULT_POSE_BAR / DEFAULT_POINT_BAR apart at most (the figures measured are in _ba_cases)."""
    c, run = BC.default_run(rig, n, kind, d)
    assert run["status"] == BA.APPLIED and all(e["margin"] >= 1e-6 for e in run["log"])
    rng = np.random.default_rng(1)
    for eps in (1e-15, 1e-13, 1e-11, 1e-9):
        for _ in range(2):
            r = BC.run_twin(c, d, t0=c["t0"] + eps * rng.standard_normal(3), rounds=4, iters=10)
            assert np.array_equal(r["active"], run["active"]) and r["status"] == run["status"]
            assert max(np.abs(r["t"] - run["t"]).max(), np.abs(r["rvec"] - run["rvec"]).max()) <= 0.1 * BC.DEFAULT_POSE_BAR
            assert np.abs(r["X"] - run["X"]).max() <= 0.1 * BC.DEFAULT_POINT_BAR
            assert np.abs(r["info"] - run["info"]).max() <= 0.1 * BC.DEFAULT_INFO_BAR * np.abs(run["info"]).max()


# ---- the fixtures of tests/test_gpu_refine_edges.py: each meets the precondition and reaches the path it is named after ------
def _report(what, key, run, spread):
    print(f"{what}: seed offset {BC.EDGE_SEED_OFFSET.get(key, 0)}, classification margin {min(e['margin'] for e in run['log']):.1e}, "
          f"accept margin {min(e['accept_margin'] for e in run['log']):.1e}, self-spread {spread:.1e}, "
          f"exits {[e['exit'] for e in run['log']]}, active {run['n_active']}")


@pytest.mark.parametrize("rig,n,kind,d", BC.rig_cases())
def test_rig_fixtures_meet_the_precondition_and_catch_the_mistake_they_exist_for(rig, n, kind, d):
    """R1 (fy = 0.85 fx) and R2 (K2 != K1) at 4 x 2.  The twin with P1[1, 1] := P1[0, 0] (R1) or with the left 3 x 3 of P2
    replaced by K1 R_rl (R2) must end more than 1e3 x the bar away in pose, or with another flag: otherwise the fixture could
    not catch the kernel or the argument fill that makes that mistake."""
    c, run, spread = BC.edge_run(rig, n, kind, d)
    _report(f"{rig} n={n} {kind} d={d}", (rig, n, kind, d), run, spread)
    assert BC.edge_ok(run, spread, TIGHT), (spread, run["log"])
    clean = ~c["outlier"] & ~c["behind"]
    # (tau is the 95 % point: a clean point in twenty is cut by design; no outlier and no point behind the camera survives)
    assert run["status"] == BA.APPLIED and run["active"][clean].mean() >= 0.9 and not run["active"][~clean].any()
    assert c["P1"][1, 1] != c["P1"][0, 0] or not np.array_equal(c["P2"][:, :3], c["P1"][:, :3])
    wrong = BC.run_twin(BC.wrong_intrinsics(c), d)
    dpose = max(np.abs(wrong["t_ref"] - run["t_ref"]).max(), np.abs(wrong["rvec_ref"] - run["rvec_ref"]).max())
    flips = int((wrong["active"] != run["active"]).sum())
    print(f"    with the mistake: pose {dpose:.1e} away, {flips} of {n} flags differ")
    assert dpose > 1e3 * TIGHT or flips > 0


@pytest.mark.parametrize("rig,n,kind,d,sigma", BC.sigma_cases())
def test_sigma_fixtures_meet_the_precondition_and_depend_on_sigma(rig, n, kind, d, sigma):
    """sigma 0.5 / 0.75 / 2: the twin's info differs from its sigma = 1 run of the same data by more than the info bar (the
    1 / sigma^2 scale is a tested quantity), the costs likewise, and at sigma = 0.5 the final flags differ too."""
    c, run, spread = BC.edge_run(rig, n, kind, d, sigma=sigma)
    _report(f"sigma={sigma} {rig} n={n} {kind} d={d}", (rig, n, kind, d, sigma), run, spread)
    assert BC.edge_ok(run, spread, TIGHT), (spread, run["log"])
    assert run["status"] == BA.APPLIED
    one = BC.run_twin(c, d)
    top = np.abs(run["info"]).max()
    dinfo, flips = np.abs(run["info"] - one["info"]).max() / top, int((run["active"] != one["active"]).sum())
    print(f"    against sigma = 1: info {dinfo:.1e} of its largest entry away, {flips} flags differ, "
          f"cost_first {run['cost_first']:.6g} vs {one['cost_first']:.6g}")
    assert dinfo > 1e3 * TIGHT
    assert abs(run["cost_first"] - one["cost_first"]) > 1e3 * TIGHT * one["cost_first"]
    if sigma == 0.5:
        assert flips > 0


@pytest.mark.parametrize("kw", BC.LAMBDA_KW, ids=lambda k: f"{k['rounds']}x{k['iters']}")
@pytest.mark.parametrize("d", [6, 8])
def test_lambda_fixture_leaves_through_the_lambda_exit_at_an_exact_tie(d, kw):
    """The exact scene started at the true pose: every residual and the cost are exactly 0, fifteen trials per round are not
    BELOW it, the rounds leave through lambda > 1e10 before their cap, and the start comes back bit for bit -- which is what
    entitles the GPU test to ask the kernel for the same."""
    c = BC.lambda_case()
    run = BC.run_twin(c, d, **kw)
    assert run["iters"] == 15 * kw["rounds"] < kw["rounds"] * kw["iters"]
    assert all(e["exit"] == "lambda" and e["steps"] == [] for e in run["log"])           # (cost 0: no relative margin to log)
    assert run["status"] == BA.APPLIED and run["n_active"] == 70 and run["cost_first"] == 0.0 and run["cost_last"] == 0.0
    assert np.array_equal(run["t"], c["t0"]) and np.array_equal(run["rvec"], np.zeros(3)) and np.array_equal(run["R"], np.eye(3))
    assert np.array_equal(run["X"], c["X0"].astype(np.float64))
    r, cc, proj, _, _ = BA.evaluate(c["X0"].astype(np.float64), [np.asarray(c[k], np.float64) for k in ("x1l", "x1r", "xl", "xr")][:d // 2],
                                    BA.views_of(c["P1"], c["P2"]), np.eye(3), c["t0"])
    assert proj.all() and not r.any()


@pytest.mark.parametrize("d", [6, 8])
def test_near_fixture_rejects_a_trial_for_an_unprojectable_point_alone(d):
    """_ba_cases.near_case: at least one trial is rejected because an active point is not projectable at it; in one such
    rejection every bad point lies outside wave 0 of its stride ((i mod 256) >= 64) and the trial cost over the other points is
    BELOW the standing cost -- the bad count alone decides, and a count summed over wave 0 alone would accept; every depth is
    1e-6 m or more from the cut; all other decisions meet fixture_ok."""
    c = BC.near_case(d)
    run = BC.run_twin(c, d, **BC.NEAR_KW)
    spread = BC.self_spread(c, d, run, **BC.NEAR_KW)
    un = BC.unprojectable_steps(run)
    for rd, k, s in un:
        print(f"d={d} round {rd} step {k}: bad {s[2].tolist()}, cost over the rest {s[3][0]:.6g} against {s[4][0]:.6g} standing, "
              f"nearest depth {s[1]:.1e} m from the cut")
    _report(f"near d={d} seed {BC.NEAR_SEED[d]}", None, run, spread)
    print(f"    steps {[(s[0], float(s[1])) for s in run['log'][0]['steps']]}")
    assert un and BC.near_ok(run, spread, TIGHT)
    assert any((s[2] % 256 >= 64).all() and s[3] < s[4] for _, _, s in un)
    assert run["status"] == BA.APPLIED and run["iters"] == 6 and [s[0] for s in run["log"][0]["steps"]].count("accepted") >= 2
    # the bad points are active, projectable at the accepted estimate, and among the near ones or the outliers' victims
    assert all(len(s[2]) > 0 for _, _, s in un)


@pytest.mark.parametrize("variant", BC.NONFINITE)
@pytest.mark.parametrize("rig,d", [("R0", 6), ("R0", 8), ("R3", 6), ("R3", 8)])
def test_nonfinite_fixtures_take_the_paths_the_twin_defines(rig, d, variant):
    c, run, spread = BC.nonfinite_run(rig, d, variant)
    i = c["spoiled"]
    _report(f"{variant} {rig} d={d} point {i}", None, run, spread)
    assert BC.edge_ok(run, spread, TIGHT), (spread, run["log"])
    assert run["n_active"] == 45 and run["active"][i] == 0 and run["iters"] == 8
    assert np.isfinite(run["info"]).all() and np.isfinite(run["t_ref"]).all() and np.isfinite(run["rvec_ref"]).all()
    if variant in ("nan_X", "inf_Z"):
        # never projectable, never active: the run is that of the other 64 points
        assert run["status"] == BA.APPLIED and np.isfinite(run["cost_first"])
        assert run["X"][i].tobytes() == c["X0"][i].astype(np.float64).tobytes()
    else:
        # active in round 0, whose cost is not finite and whose trials all fail; dropped at the first re-classification; the
        # later rounds run clean on 45 points -- and cost_first keeps the PnP pose
        assert run["status"] == BA.KEPT_PNP and not np.isfinite(run["cost_first"]) and np.isfinite(run["cost_last"])
        assert (np.isnan(run["cost_first"])) == variant.startswith("nan")
        assert not any(s[0] == "accepted" for s in run["log"][0]["steps"])
        assert all(any(s[0] == "accepted" for s in e["steps"]) for e in run["log"][1:])
        assert np.array_equal(run["t"], c["t0"]) and run["X"].tobytes() == c["X0"].astype(np.float64).tobytes()
        assert np.abs(run["t_ref"] - c["t_true"]).max() < 0.03
