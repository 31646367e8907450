"""The degenerate PnP cases of tests/_pnp_cases.py reach what they are meant to reach -- shown on the CPU oracle alone
(no GPU): NaN hypotheses on exactly coplanar minimal sets, a search that runs out or stops late, a refit that runs to its
20-iteration cap on data that does not determine the pose and converges on the rest.  tests/test_gpu_pnp_degenerate.py
then holds the HIP solver to the oracle on the same cases; the class a case falls in (failed / converged / capped)
decides its bar there, so the classes are pinned here."""
import numpy as np
import pytest

import _pnp_cases as pc

FX, FY, CX, CY = pc.K[0, 0], pc.K[1, 1], pc.K[0, 2], pc.K[1, 2]


def _five(oracle, kind, seed=pc.SEED):
    X, x, r, t = pc.make(kind, 5, seed, 0)
    return X.astype(np.float64), x.astype(np.float64)


def test_generator_shapes_types_and_planarity(oracle):
    for case in pc.CASES:
        kind, n, n_out = case
        X, x, r, t = pc.make_case(case, triangulate=oracle.triangulate)
        assert X.shape == (n, 3) and X.dtype == np.float32 and x.shape == (n, 2) and x.dtype == np.float32
        assert np.isfinite(X).all() and np.isfinite(x).all()
        X2, x2, _, _ = pc.make_case(case, triangulate=oracle.triangulate)
        assert X2.tobytes() == X.tobytes() and x2.tobytes() == x.tobytes()          # a case is a function of its id
        if kind == "wall":
            assert (X[:, 2] == np.float32(12)).all()                                # exactly planar in float32
        if kind == "ground":
            assert (X[:, 1] == np.float32(1.65)).all()
        if kind.startswith("wall_off_"):
            assert (X[:, 2] != np.float32(12)).sum() == min(int(kind[9:]), n)
        if kind == "wall_tri":
            assert 0 < np.ptp(X[:, 2]) < 1e-3                                       # near-planar: float32 pixels through the baseline
        if kind == "dups":
            assert len(np.unique(X, axis=0)) <= max(3, n // 8)
        if kind in ("far", "mixedfar"):
            assert X[:, 2].max() / X[:, 2].min() > (50 if kind == "mixedfar" and n > 6 else 1)
    # the box is the existing scene of test_gpu_parity_pose.py::_scene, to float32
    rng = np.random.default_rng(3)
    scene = np.stack([rng.uniform(-8, 8, 64), rng.uniform(-2, 1.6, 64), rng.uniform(5, 40, 64)], 1).astype(np.float32)
    assert np.array_equal(pc.make("box", 64, 3, 20)[0], scene)
    with pytest.raises(ValueError):
        pc.make("wall_tri", 6, 1, 0)


def test_cost_is_the_float64_sum_of_squared_residuals():
    X, x, r, t = pc.make("box", 65, 3, 0, noise=0.0)
    from scipy.spatial.transform import Rotation
    R = Rotation.from_rotvec(r).as_matrix()
    mask = np.ones(65, np.uint8)
    assert pc.cost(X, x, mask, R, t) < 65 * 2 * (2e-4) ** 2            # float32 pixels: half an ulp of ~1200 px is 6e-5
    xs = x.copy()
    xs[3] += np.float32([3, -4])
    assert abs(pc.cost(X, xs, mask, R, t) - 25.0) < 1e-2
    mask[3] = 0
    assert pc.cost(X, xs, mask, R, t) < 65 * 2 * (2e-4) ** 2


def test_epnp_is_nan_on_coplanar_five_and_finite_on_line_and_duplicates(oracle):
    """Five points with one constant coordinate: the third principal extent of the set is 0, the control points coincide
    and the restated EPnP (as upstream's) divides by it -- R and t are non-finite.  Collinear and
    duplicated points are degenerate too, but stay finite."""
    for kind in pc.PLANAR_KINDS:
        pws, us = _five(oracle, kind)
        R, t = oracle.epnp(pws, us, FX, FY, CX, CY)
        assert not np.isfinite(R).any() and not np.isfinite(t).any(), kind
    pws, us = _five(oracle, "line")
    R, t = oracle.epnp(pws, us, FX, FY, CX, CY)
    assert np.isfinite(R).all() and np.isfinite(t).all()
    pws, us = _five(oracle, "box")
    pws[1], us[1] = pws[0], us[0]
    R, t = oracle.epnp(pws, us, FX, FY, CX, CY)
    assert np.isfinite(R).all() and np.isfinite(t).all()


@pytest.mark.parametrize("case", [c for c in pc.CASES if c[0] in pc.PLANAR_KINDS], ids=pc.case_id)
def test_exactly_planar_sets_fail_after_the_whole_search(oracle, case):
    ref = pc.reference(oracle, case)["ref"]
    assert ref["ok"] == 0 and ref["ransac_iters"] == 500 and ref["best_iter"] == -1
    assert ref["n_inliers"] == 0 and not ref["mask"].any()


def test_wall_with_three_points_off_it_stops_late(oracle):
    """257 points, 3 off the plane: only a subset holding one of them gives a finite hypothesis, so the adaptive stop
    fires past the first 64-hypothesis phase of an LK-mode context and inside the 512 of an ORB-mode one (seed 7: 104
    iterations, the winner the last of them)."""
    ref = pc.reference(oracle, ("wall_off_3", 257, 80))["ref"]
    assert ref["ok"] == 1 and 64 < ref["ransac_iters"] < 500, ref["ransac_iters"]


@pytest.mark.parametrize("case", [c for c in pc.CASES if c[0] in pc.CAPPED_KINDS and c[1] > 6], ids=pc.case_id)
def test_pose_free_families_run_the_refit_to_its_cap(oracle, case):
    ref = pc.reference(oracle, case)["ref"]
    assert ref["ok"] == 1 and ref["lm_iters"] == 20
    S, kept = pc.sensitivity(oracle, case)
    assert kept >= pc.MIN_KEPT, kept                       # the bar of the GPU test rests on these reruns
    assert 0 < S < 1


@pytest.mark.parametrize("case", [c for c in pc.CASES if c[0] not in pc.CAPPED_KINDS] + pc.EDGE_CASES, ids=pc.case_id)
def test_other_families_converge_before_the_cap(oracle, case):
    """box, tilted, wall_tri, dups, mixedfar -- and far and the walls with points off them, which the GPU test holds to
    the converged-case bar as well."""
    assert pc.reference(oracle, case)["ref"]["lm_iters"] < 20


@pytest.mark.parametrize("case", pc.CASES + pc.EDGE_CASES, ids=pc.case_id)
def test_refit_does_not_raise_the_cost_and_outputs_are_finite(oracle, case):
    c = pc.reference(oracle, case)
    ref = c["ref"]
    if not ref["ok"]:
        assert np.array_equal(ref["R"], np.eye(3)) and not ref["tvec"].any() and not ref["rvec"].any()
        return
    assert all(np.isfinite(ref[k]).all() for k in ("R", "tvec", "rvec"))
    assert np.isfinite(c["cost_start"]) and c["cost_ref"] <= c["cost_start"]
    assert ref["n_inliers"] == int(ref["mask"].sum()) >= 5


@pytest.mark.parametrize("case", pc.EDGE_CASES, ids=pc.case_id)
def test_box_edge_puts_one_point_exactly_on_the_inlier_threshold(oracle, case):
    """The moved point is an inlier of the winner by equality alone: its float squared distance to the winner's float
    projection IS 0.25f, the oracle counts it, and one float32 ulp further out it does not and nothing else changes --
    a scorer that tests "<" instead of "<=" loses one inlier."""
    X, x, r, t, j = pc.make_edge_case(oracle, case)
    ref = pc.reference(oracle, case)["ref"]
    assert pc.reference(oracle, ("box",) + tuple(case[1:]))["ref"]["mask"][j] == 0
    assert ref["ok"] == 1 and ref["mask"][j] == 1
    idx = pc.ransac_subset(oracle, case[1], ref["best_iter"])
    R, tt = pc.hypothesis(oracle, X, x, idx)
    err = pc.reproj_err2_f32(R, tt, X, x)
    assert j not in idx and err[j] == np.float32(0.25) and np.array_equal(err <= np.float32(0.25), ref["mask"].astype(bool))
    xo = x.copy()
    xo[j, 0] = np.nextafter(xo[j, 0], np.float32(np.inf))
    out = oracle.pnp_ransac(X, xo, pc.K)
    assert out["mask"][j] == 0 and out["best_iter"] == ref["best_iter"] and out["n_inliers"] == ref["n_inliers"] - 1


def test_reference_restores_the_refit_knob(oracle):
    pc.reference(oracle, ("box", 65, 20))
    assert oracle.set_opencv_compat(oracle.COMPAT_PNP_REFIT, 0) == 0


def test_four_coplanar_points_are_solved_by_p3p(oracle):
    """n == 4 takes P3P, which has no trouble with a plane: the oracle solves the eight walls of the GPU test."""
    for seed in range(8):
        X, x, r, t = pc.make("wall", 4, seed, 0)
        ref = oracle.pnp_ransac(X, x, pc.K)
        assert ref["ok"] == 1 and ref["n_inliers"] == 4 and np.isfinite(ref["tvec"]).all(), seed


def test_no_case_brings_the_refit_within_its_cholesky_pivot_criterion(oracle):
    """A finding, pinned so that it is not forgotten: through the stage call none of these families hands the refit a
    damped system whose smallest Cholesky pivot is within 1e-10 of its diagonal entry -- the criterion at which the device
    leaves the Cholesky route for the SVD one.  lambda only falls below 1e-10 after eight accepted steps in a row, and a
    refit that slow is not reached from a RANSAC winner: the converging families stop after 3-5 steps at lambda >= 1e-7,
    the capped ones alternate accepted and rejected steps (lambda >= 1e-10; the nearest is line at 65 points, 2e-9).  An
    exactly collinear or coincident set never gets that far: EPnP yields no model and the call fails.  So the device's
    fallback decision is not exercised by data here, only the SVD route itself, forced by SVO_REFIT_SVD=1 (DESIGN.md
    section 5).  The twin that measures this is validated by reproducing the oracle's lm_iters in every case."""
    nearest = {}
    for case in pc.CASES + pc.EDGE_CASES:
        tr = pc.refit_trace(oracle, case)
        if tr is None:
            continue
        iters, solves = tr
        assert iters == pc.reference(oracle, case)["ref"]["lm_iters"], case
        nearest[case] = min(r for _, r in solves)
    assert len(nearest) >= 40
    worst = min(nearest, key=nearest.get)
    print("nearest to the pivot criterion:", pc.case_id(worst), nearest[worst])
    assert nearest[worst] > 1e-10, (worst, nearest[worst])
    assert worst[0] in pc.CAPPED_KINDS and nearest[worst] < 1e-6
