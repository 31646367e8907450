"""GPU parity of the stage call Context.pnp_ransac on the point sets of tests/_pnp_cases.py (run with -m gpu): exactly
planar, near-planar, collinear, clustered, duplicated and far / mixed-depth object points, and the ordinary box at the
point counts around the wave (64), scoring-chunk / refit-stride (256) and two-chunk (512) boundaries -- plus the box
with one image point exactly ON the inlier threshold of the winning hypothesis (box_edge: "<=" against "<").  What each family
does to the CPU oracle is pinned by tests/test_pnp_cases.py; here the HIP solver is held to the oracle, on an LK-mode
context (first RANSAC phase: 64 hypotheses) and an ORB-mode one (512), from host memory and -- the 257-point cases --
from device tensors.

Bars.  Every case: ok, ransac_iters, best_iter, n_inliers and the mask EQUAL the oracle's (a NaN hypothesis scores 0
on both sides and never wins).  ok == 0: R = I, rvec = tvec = 0.  Converged cases (oracle lm_iters < 20): the bars of
test_gpu_parity_pose.py::_check_pnp unchanged -- lm_iters equal, pose relfro <= 1e-9, rvec to 1e-9.  Capped cases
(oracle lm_iters == 20: line, nearline, cluster -- the data does not determine the pose, so a pose bar means nothing):
the pose is finite and R orthonormal to 1e-12, the refit did not raise the cost of the RANSAC winner, and the final
cost is within S of the oracle's, S being the oracle's OWN sensitivity to one float32 ulp of one input coordinate
(_pnp_cases.sensitivity; margin 1x: one float32 ulp of input is nine orders of magnitude above double rounding, so a
solver route or reduction order that moves the cost further decides the answer instead of the data).

SVO_PNP_PARITY_JSON=<path> makes the module write every measured figure there (profiles/pnp_degenerate_parity.json is
such a record); by default nothing is written."""
import json
import os

import numpy as np
import pytest

import _pnp_cases as pc

pytestmark = pytest.mark.gpu

K = pc.K
POSE_TOL = 1e-4          # north_star: pose within 1e-4 relative Frobenius
TIGHT = 1e-9
_RECORD = {}


def relfro(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(np.asarray(b)), 1e-300)


@pytest.fixture(scope="module")
def tc():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def ctxs(pkg, tc):
    c = {"lk": pkg.Context(416, 128, device=0),
         "orb": pkg.Context(416, 128, device=0, track_mode=pkg.MODE_ORB, min_move2=0.0, max_move2=1e9)}
    yield c
    for v in c.values():
        v.close()


@pytest.fixture(scope="module", autouse=True)
def _parity_record():
    yield
    path = os.environ.get("SVO_PNP_PARITY_JSON")
    if path and _RECORD:
        with open(path, "w") as f:
            json.dump(dict(bars=dict(converged_pose_relfro=TIGHT, capped="|cost_gpu - cost_oracle| / cost_oracle <= S (1x)"),
                           cases=_RECORD), f, indent=1, sort_keys=True)
            f.write("\n")


def _note(case, mode, route, src, **figures):
    _RECORD.setdefault(pc.case_id(case), {})["%s/%s/%s" % (mode, route, src)] = figures


def _check_case(oracle, case, got, mode, route, src):
    c = pc.reference(oracle, case)
    ref = c["ref"]
    capped = bool(ref["ok"]) and ref["lm_iters"] == 20
    fig = dict(ok=int(got["ok"]), ransac_iters=int(got["ransac_iters"]), best_iter=int(got["best_iter"]),
               n_inliers=int(got["n_inliers"]), lm_iters=int(got["lm_iters"]), lm_iters_oracle=int(ref["lm_iters"]),
               discrete_equal=bool(pc.same_discrete(dict(got, lm_iters=ref["lm_iters"]), ref)),
               cls="failed" if not ref["ok"] else "capped" if capped else "converged")
    if ref["ok"] and got["ok"]:
        T_g = np.hstack([got["R"], got["tvec"][:, None]])
        T_r = np.hstack([ref["R"], ref["tvec"][:, None]])
        fig["relfro"] = float(relfro(T_g, T_r))
        fig["rvec_maxdiff"] = float(np.abs(got["rvec"] - ref["rvec"]).max())
        cost_gpu = pc.cost(c["X"], c["x"], ref["mask"], got["R"], got["tvec"])
        fig.update(cost_gpu=cost_gpu, cost_oracle=c["cost_ref"], cost_start=c["cost_start"],
                   cost_reldiff=abs(cost_gpu - c["cost_ref"]) / c["cost_ref"])
        if capped:
            fig["S"], fig["kept"] = pc.sensitivity(oracle, case)
    _note(case, mode, route, src, **fig)
    print(pc.case_id(case), mode, route, src, fig)

    # every case: the discrete outcome is the oracle's
    assert got["ok"] == ref["ok"]
    assert got["ransac_iters"] == ref["ransac_iters"] and got["best_iter"] == ref["best_iter"]
    assert got["n_inliers"] == ref["n_inliers"]
    assert np.array_equal(got["mask"], ref["mask"])
    if not ref["ok"]:
        assert np.array_equal(got["R"], np.eye(3)) and not got["tvec"].any() and not got["rvec"].any()
        assert got["lm_iters"] == 0
        return
    if not capped:
        assert got["lm_iters"] == ref["lm_iters"]
        assert fig["relfro"] <= POSE_TOL
        assert fig["relfro"] <= TIGHT
        assert fig["rvec_maxdiff"] <= TIGHT
        return
    assert all(np.isfinite(got[k]).all() for k in ("R", "tvec", "rvec"))
    assert np.abs(got["R"].T @ got["R"] - np.eye(3)).max() <= 1e-12
    assert fig["cost_gpu"] <= c["cost_start"] * (1 + 1e-12)
    assert fig["kept"] >= pc.MIN_KEPT
    assert fig["cost_reldiff"] <= fig["S"], (fig["cost_reldiff"], fig["S"])


def _run(ctx, tc, c, src):
    if src == "dev":
        return ctx.pnp_ransac(tc.from_numpy(c["X"].copy()).cuda(), tc.from_numpy(c["x"].copy()).cuda(), K)
    return ctx.pnp_ransac(c["X"], c["x"], K)


@pytest.mark.parametrize("mode", ["lk", "orb"])
@pytest.mark.parametrize("case", pc.CASES + pc.EDGE_CASES, ids=pc.case_id)
def test_pnp_ransac_parity_on_degenerate_and_boundary_sets(ctxs, oracle, tc, case, mode):
    c = pc.reference(oracle, case)
    _check_case(oracle, case, _run(ctxs[mode], tc, c, "host"), mode, "chol", "host")
    if case[1] == 257:
        _check_case(oracle, case, _run(ctxs[mode], tc, c, "dev"), mode, "chol", "dev")


# ... and the two converged cases that come nearest the 1e-9 pose bar on the default route: far at 6 points (9.3e-10 by
# Cholesky, 1.1e-10 by SVD: cond(A) * 2^-52 of the solve shows) and tilted at 255 points (3.1e-10 on either route: the
# reduction order, carried through a stop decided at the fifth step)
_SVD_CASES = ([c for c in pc.CASES if c[0] in pc.CAPPED_KINDS] + [(k, 257, 80) for k in ("tilted", "far", "wall_tri")]
              + [("far", 6, 0), ("tilted", 255, 80)])


@pytest.mark.parametrize("mode", ["lk", "orb"])
@pytest.mark.parametrize("case", _SVD_CASES, ids=pc.case_id)
def test_refit_svd_route_meets_the_same_bars(ctxs, oracle, tc, monkeypatch, case, mode):
    """SVO_REFIT_SVD=1 sends every solve of the refit down the reference's SVD route (the route the Cholesky pivot test
    hands rank-deficient systems to): the capped families and the three worst-conditioned converged ones must meet
    their bars on it as well."""
    monkeypatch.setenv("SVO_REFIT_SVD", "1")
    _check_case(oracle, case, _run(ctxs[mode], tc, pc.reference(oracle, case), "host"), mode, "svd", "host")


@pytest.mark.parametrize("mode", ["lk", "orb"])
def test_four_coplanar_points_take_the_p3p_kernel(ctxs, oracle, mode):
    """n == 4 on the wall: P3P has no trouble with a plane.  The bars of
    test_gpu_parity_pose.py::test_pnp_ransac_four_points_take_the_p3p_kernel."""
    for seed in range(8):
        X, x, r, t = pc.make("wall", 4, seed, 0)
        ref = oracle.pnp_ransac(X, x, K)
        got = ctxs[mode].pnp_ransac(X, x, K)
        assert got["ok"] == ref["ok"] and got["n_inliers"] == ref["n_inliers"] and got["ransac_iters"] == ref["ransac_iters"], seed
        assert np.array_equal(got["mask"], ref["mask"]), seed
        assert ref["ok"] == 1, seed                                   # pinned on the CPU by tests/test_pnp_cases.py
        assert got["n_inliers"] == 4 and abs(got["lm_iters"] - ref["lm_iters"]) <= 1, seed
        assert np.abs(got["tvec"] - ref["tvec"]).max() <= 1e-6 * max(1.0, np.abs(ref["tvec"]).max()), seed
        assert np.abs(got["rvec"] - ref["rvec"]).max() <= 1e-6, seed
