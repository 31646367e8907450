"""The numpy restatement of the pose refinement stage (tests/_refine_ref.py, rules R1-R7 of DESIGN.md section 5e) checked
against mathematics: it is the reference of tests/test_gpu_refine.py, the oracle has no such stage."""
import numpy as np
import pytest
from scipy.spatial.transform import Rotation

import _refine_cases as RC
import _refine_ref as RR
import _rigs


def fixture_ok(ref_run):
    """The precondition of every fixture a GPU test compares on: at no re-classification a projectable point within
    1e-6 tau of the threshold (a flag could flip on a last-bit difference), and every round ended through the
    |xi| < 1e-10 exit (the pose every round hands on is converged, not cut off by the iteration cap or by lambda)."""
    return all(e["exit"] == "xi" and e["margin"] >= 1e-6 for e in ref_run["log"])


def _random_scene(n, seed, rig):
    rng = np.random.default_rng(seed)
    P1, P2 = _rigs.matrices(rig)
    X = np.stack([rng.uniform(-8, 8, n), rng.uniform(-3, 3, n), rng.uniform(5, 40, n)], 1)
    return rng, np.asarray(P1, np.float64).reshape(3, 4), np.asarray(P2, np.float64).reshape(3, 4), X


def _observe(P1, P2, X, R, t):
    vs = RR.views_of(P1, P2, 4)
    Y = X @ R.T + t
    out = []
    for M, p4 in vs:
        h = Y @ M.T + p4
        out.append(h[:, :2] / h[:, 2:3])
    return out


@pytest.mark.parametrize("seed", [3, 4])
def test_jacobian_matches_central_differences(seed):
    """R3 for both views, view R on a general (unrectified, unequal cameras) rig."""
    rng = np.random.default_rng(seed)
    P1, P2, X = _rigs.general_matrices(seed)
    R = Rotation.from_rotvec((0.02, -0.05, 0.03)).as_matrix()
    t = np.array([0.1, -0.05, 0.7])
    Y = X @ R.T + t
    X = X[(Y[:, 2] > 0.3) & ((Y @ P2[2, :3]) + P2[2, 3] > 0.3)][:12]       # in front of both views at this pose
    assert len(X) == 12
    obs = [o + rng.standard_normal(o.shape) for o in _observe(P1, P2, X, R, t)]
    views = RR.views_of(P1, P2, 4)
    r0, _, proj, J = RR.evaluate(X, obs, views, R, t)
    assert proj.all()
    eps = 1e-6
    for k in range(6):
        xi = np.zeros(6)
        xi[k] = eps
        Ep, Vp = RR.se3_exp(xi)
        Em, Vm = RR.se3_exp(-xi)
        rp = RR.evaluate(X, obs, views, Ep @ R, Ep @ t + Vp, jac=False)[0]
        rm = RR.evaluate(X, obs, views, Em @ R, Em @ t + Vm, jac=False)[0]
        num = (rp - rm) / (2 * eps)
        # central differences: truncation O(eps^2 |d3r|) ~ 1e-9, rounding |r| 2^-52 / eps ~ 1e-7 for |r| ~ 1e3 px
        assert np.abs(num - J[:, :, k]).max() <= 1e-6 * max(1.0, np.abs(J[:, :, k]).max())


def test_exponential_and_logarithm():
    for scale in (1e-12, 1e-6, 0.3, 2.0):
        phi = scale * np.array([0.6, -0.48, 0.64])          # |phi| = scale < pi
        E, _ = RR.se3_exp(np.concatenate([np.zeros(3), phi]))
        assert np.abs(E - Rotation.from_rotvec(phi).as_matrix()).max() < 1e-14
        assert np.abs(RR.so3_log(E) - phi).max() < 1e-13 * max(1.0, scale)
        assert np.abs(RR.rodrigues(phi) - E).max() < 1e-14
    # V(phi) rho against the series
    xi = np.array([0.3, -0.2, 0.5, 0.01, -0.02, 0.015])
    _, Vr = RR.se3_exp(xi)
    K = RR.hat(xi[3:])
    V, term = np.zeros((3, 3)), np.eye(3)
    for k in range(14):                                      # V = sum K^k / (k + 1)!
        V += term
        term = term @ K / (k + 2)
    assert np.abs(Vr - V @ xi[:3]).max() < 1e-12


@pytest.mark.parametrize("d", [2, 4])
def test_noiseless_points_recover_the_pose(d):
    _, P1, P2, X = _random_scene(80, 11, "R3")
    R, t = RC.true_pose()
    xl, xr = _observe(P1, P2, X, R, t)
    R0, t0 = RC.start_pose()
    run = RR.refine(X, xl, xr if d == 4 else None, P1, P2, R0, t0)
    assert run["status"] == RR.APPLIED and run["n_active"] == 80 and run["views"] == d // 2
    assert np.abs(run["R"] - R).max() < 1e-9 and np.abs(run["t"] - t).max() < 1e-9
    assert np.abs(run["rvec"] - Rotation.from_matrix(R).as_rotvec()).max() < 1e-9
    assert run["iters"] <= 4 * 10 and run["cost_last"] < 1e-12 < run["cost_first"]


@pytest.mark.parametrize("d", [2, 4])
@pytest.mark.parametrize("n", [65, 257])
def test_outliers_end_inactive_clean_points_active(n, d):
    c, run = RC.ref_run("R0", n, "outliers", d)
    assert c["outlier"].sum() == int(0.3 * n)
    assert run["status"] == RR.APPLIED
    assert (run["active"][c["outlier"]] == 0).all() and (run["active"][~c["outlier"]] == 1).all()
    # ... and the pose is at the noise level: 0.3 px over >= 45 points at <= 40 m
    assert np.abs(run["t"] - c["t_true"]).max() < 0.02 and np.abs(run["R"] - c["R_true"]).max() < 1e-3


def test_two_views_add_information():
    """info(d = 4) - info(d = 2) at one pose over the full point set is a sum of J^T J terms: positive semi-definite."""
    c = RC.make_case("R3", 257, "outliers")
    X = c["X"].astype(np.float64)
    obs = [c["xl"].astype(np.float64), c["xr"].astype(np.float64)]
    J4 = RR.evaluate(X, obs, RR.views_of(c["P1"], c["P2"], 4), c["R0"], c["t0"])[3]
    J2 = RR.evaluate(X, obs[:1], RR.views_of(c["P1"], c["P2"], 2), c["R0"], c["t0"])[3]
    I4 = np.einsum("nda,ndb->ab", J4, J4)
    I2 = np.einsum("nda,ndb->ab", J2, J2)
    ev = np.linalg.eigvalsh(I4 - I2)
    assert ev.min() >= -1e-9 * np.abs(np.linalg.eigvalsh(I4)).max()


@pytest.mark.parametrize("d", [2, 4])
def test_all_points_behind_the_camera_keep_pnp(d):
    c, run = RC.ref_run("R0", 64, "all_behind", d)
    assert run["status"] == RR.KEPT_PNP and run["n_active"] == 0 and not run["active"].any()
    assert np.array_equal(run["t"], c["t0"]) and np.array_equal(run["R"], RR.rodrigues(c["rvec0"]))
    assert not run["info"].any()


def test_five_points_keep_pnp():
    _, P1, P2, X = _random_scene(5, 17, "R0")
    R, t = RC.true_pose()
    xl, xr = _observe(P1, P2, X, R, t)
    R0, t0 = RC.start_pose()
    run = RR.refine(X, xl, xr, P1, P2, R0, t0, min_inliers=6)
    assert run["status"] == RR.KEPT_PNP and run["n_active"] == 5
    assert np.array_equal(run["R"], R0) and np.array_equal(run["t"], t0)
    assert np.abs(run["R_ref"] - R).max() < 1e-8            # the refinement itself converged; it is the count that refuses it
    assert RR.refine(X, xl, xr, P1, P2, R0, t0, min_inliers=5)["status"] == RR.APPLIED


def test_point_order_does_not_matter():
    c, run = RC.ref_run("R0", 255, "outliers", 4)
    perm = np.random.default_rng(1).permutation(255)
    run2 = RR.refine(c["X"], c["xl"], c["xr"], c["P1"], c["P2"], RR.rodrigues(c["rvec0"]), c["t0"], rounds=RC.ROUNDS, iters=RC.ITERS,
                     perm=perm)
    assert np.array_equal(run["active"], run2["active"])
    assert np.abs(run["R"] - run2["R"]).max() < 1e-12 and np.abs(run["t"] - run2["t"]).max() < 1e-12
    assert np.abs(run["info"] - run2["info"]).max() <= 1e-12 * np.abs(run["info"]).max()


@pytest.mark.parametrize("rig,n,kind,d", RC.stage_cases())
def test_gpu_fixtures_meet_the_precondition(rig, n, kind, d):
    """Every fixture tests/test_gpu_refine.py hands to svo_refine_pose."""
    c, run = RC.ref_run(rig, n, kind, d)
    if kind == "all_behind":
        # nothing is projectable: H = 0, every solve fails, no round can take a step -- and no decision depends on rounding
        assert not RR.evaluate(c["X"].astype(np.float64), [c["xl"].astype(np.float64)], RR.views_of(c["P1"], c["P2"], 2),
                               RR.rodrigues(c["rvec0"]), c["t0"])[2].any()
        assert run["status"] == RR.KEPT_PNP
        return
    assert fixture_ok(run), run["log"]
    clean = ~c["outlier"] & ~c["behind"]
    assert (run["active"][clean] == 1).all() and not run["active"][~clean].any()
    assert run["iters"] <= RC.ROUNDS * RC.ITERS


@pytest.mark.parametrize("rig,n,kind,d", RC.DEFAULT_CASES)
def test_default_setting_fixtures_reproduce_themselves(rig, n, kind, d):
    """The stage-call fixtures of tests/test_gpu_refine.py at the default 4 x 10 iterations: fixture_ok cannot hold there (the
    Huber rounds are cut off by the cap), so the reference must reproduce itself on them to a tenth of the 1e-9 bar."""
    c, run, spread = RC.default_run(rig, n, kind, d)
    assert run["status"] == RR.APPLIED and run["iters"] <= 40
    assert all(e["margin"] >= 1e-6 for e in run["log"]), run["log"]
    assert spread <= 1e-10, spread
    assert (run["active"][~c["outlier"]] == 1).all() and not run["active"][c["outlier"]].any()


# ---- the fixtures of tests/test_gpu_refine_edges.py: each meets the precondition and reaches the path it is named after ------
TIGHT = 1e-9                                     # the bar of the GPU comparison (tests/test_gpu_parity_pose.py)


def _report(what, key, run, spread):
    print(f"{what}: seed offset {RC.EDGE_SEED_OFFSET.get(key, 0)}, classification margin {min(e['margin'] for e in run['log']):.1e}, "
          f"self-spread {spread:.1e}, exits {[e['exit'] for e in run['log']]}, active {run['n_active']}")


@pytest.mark.parametrize("rig,n,kind,d", RC.rig_cases())
def test_rig_fixtures_meet_the_precondition_and_catch_the_mistake_they_exist_for(rig, n, kind, d):
    """R1 (fy = 0.85 fx) and R2 (K2 != K1).  The reference with P1[1, 1] := P1[0, 0] (R1) or with the left 3 x 3 of P2 replaced
    by K1 R_rl (R2; the one-view cases never read P2 and are held to R1's mistake only where it applies) must end more than
    1e3 x the bar away in pose, or with another flag."""
    c, run, spread = RC.edge_run(rig, n, kind, d)
    _report(f"{rig} n={n} {kind} d={d}", (rig, n, kind, d), run, spread)
    assert fixture_ok(run) and RC.edge_ok(run, spread), (spread, run["log"])
    clean = ~c["outlier"] & ~c["behind"]
    assert run["status"] == RR.APPLIED and (run["active"][clean] == 1).all() and not run["active"][~clean].any()
    if rig == "R2" and d == 2:
        return                                   # view L alone: K2 is not an input
    wrong = RC.run_ref(RC.wrong_intrinsics(c), d)
    dpose = max(np.abs(wrong["t_ref"] - run["t_ref"]).max(), np.abs(wrong["rvec_ref"] - run["rvec_ref"]).max())
    flips = int((wrong["active"] != run["active"]).sum())
    print(f"    with the mistake: pose {dpose:.1e} away, {flips} of {n} flags differ")
    assert dpose > 1e3 * TIGHT or flips > 0


@pytest.mark.parametrize("rig,n,kind,d,sigma", RC.sigma_cases())
def test_sigma_fixtures_meet_the_precondition_and_depend_on_sigma(rig, n, kind, d, sigma):
    c, run, spread = RC.edge_run(rig, n, kind, d, sigma=sigma)
    _report(f"sigma={sigma} {rig} n={n} {kind} d={d}", (rig, n, kind, d, sigma), run, spread)
    assert fixture_ok(run) and RC.edge_ok(run, spread), (spread, run["log"])
    assert run["status"] == RR.APPLIED
    one = RC.run_ref(c, d)
    top = np.abs(run["info"]).max()
    dinfo, flips = np.abs(run["info"] - one["info"]).max() / top, int((run["active"] != one["active"]).sum())
    print(f"    against sigma = 1: info {dinfo:.1e} of its largest entry away, {flips} flags differ")
    assert dinfo > 1e3 * TIGHT and abs(run["cost_first"] - one["cost_first"]) > 1e3 * TIGHT * one["cost_first"]
    if sigma == 0.5:
        assert flips > 0


@pytest.mark.parametrize("kw", RC.LAMBDA_KW, ids=lambda k: f"{k['rounds']}x{k['iters']}")
@pytest.mark.parametrize("d", [2, 4])
def test_lambda_fixture_leaves_through_the_lambda_exit_at_an_exact_tie(d, kw):
    c = RC.lambda_case()
    run = RC.run_ref(c, d, **kw)
    assert run["iters"] == 15 * kw["rounds"] < kw["rounds"] * kw["iters"]
    assert all(e["exit"] == "lambda" and e["steps"] == [] for e in run["log"])
    assert run["status"] == RR.APPLIED and run["n_active"] == 70 and run["cost_first"] == 0.0 and run["cost_last"] == 0.0
    assert np.array_equal(run["t"], c["t0"]) and np.array_equal(run["rvec"], np.zeros(3)) and np.array_equal(run["R"], np.eye(3))


@pytest.mark.parametrize("d", [2, 4])
def test_near_fixture_rejects_a_trial_for_an_unprojectable_point_alone(d):
    """_refine_cases.near_case: a rejection in which every bad point lies outside wave 0 of its stride and the trial cost over
    the other points is BELOW the standing cost; the bad points are the ones the true pose has behind the camera."""
    c = RC.near_case(d)
    run = RC.run_ref(c, d, **RC.NEAR_KW)
    spread = RC.edge_spread(c, d, run, **RC.NEAR_STARTS, **RC.NEAR_KW)
    un = RC.unprojectable_steps(run)
    for rd, k, s in un:
        print(f"d={d} round {rd} step {k}: bad {s[2].tolist()}, cost over the rest {s[3][0]:.6g} against {s[4][0]:.6g} standing, "
              f"nearest depth {s[1]:.1e} m from the cut")
    _report(f"near d={d} seed {RC.NEAR_SEED[d]}", None, run, spread)
    print(f"    accept margin {run['log'][0]['accept_margin']:.1e}, steps {[(s[0], float(s[1])) for s in run['log'][0]['steps']]}")
    assert un and RC.near_ok(run, spread)
    assert all(set(s[2]) <= set(c["through"]) and (s[2] % 256 >= 64).all() for _, _, s in un)
    assert run["status"] == RR.APPLIED and run["iters"] == 6 and [s[0] for s in run["log"][0]["steps"]].count("accepted") >= 2


@pytest.mark.parametrize("variant", RC.NONFINITE)
@pytest.mark.parametrize("rig,d", [("R0", 2), ("R0", 4), ("R3", 2), ("R3", 4)])
def test_nonfinite_fixtures_take_the_paths_the_reference_defines(rig, d, variant):
    c, run, spread = RC.nonfinite_run(rig, d, variant)
    i = c["spoiled"]
    _report(f"{variant} {rig} d={d} point {i}", None, run, spread)
    assert RC.edge_ok(run, spread, exits=("xi", "lambda")), (spread, run["log"])
    assert run["n_active"] == 45 and run["active"][i] == 0
    assert np.isfinite(run["info"]).all() and np.isfinite(run["t_ref"]).all() and np.isfinite(run["rvec_ref"]).all()
    if variant in ("nan_X", "inf_Z"):
        assert run["status"] == RR.APPLIED and np.isfinite(run["cost_first"])
    else:
        # round 0: the cost is not finite, fifteen solves or trials fail, lambda exit; the point goes at the re-classification
        assert run["status"] == RR.KEPT_PNP and not np.isfinite(run["cost_first"]) and np.isfinite(run["cost_last"])
        assert run["log"][0]["exit"] == "lambda" and not any(s[0] == "accepted" for s in run["log"][0]["steps"])
        assert run["log"][1]["exit"] == "xi" and np.array_equal(run["t"], c["t0"])
        assert np.abs(run["t_ref"] - c["t_true"]).max() < 0.03
