"""The oracle's geometry on general stereo rigs (CPU), against independent float64 references.

Bit-exact HIP-vs-oracle parity cannot see a fault copied into both sides (a row of P1 read for P2, fx used for fy), so
here the oracle meets references that share no code with it, on tests/_rigs.py's R0 (KITTI, the control), R1
(anisotropic), R2 (unequal cameras), R3 (unrectified) and random full 3x4 P1 / P2:
  * triangulation against a numpy DLT (null vector by np.linalg.svd, dehomogenised), noisy and exact correspondences,
    the exact ones also against the planted points;
  * RANSAC on planted sets with outliers: the inlier mask equals the planted inlier set, the pose is near the planted
    one, and the LM refit is a stationary point of the float64 reprojection error over the returned inliers (separate
    fx and fy);
  * the 4-point P3P and the 5+-point EPnP branches with fx != fy."""
import numpy as np
import pytest
from scipy.optimize import least_squares
from scipy.spatial.transform import Rotation

import _rigs

RIGS = ["R0", "R1", "R2", "R3"]


def _scene(n, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(-8, 8, n), rng.uniform(-2, 1.6, n), rng.uniform(5, 40, n)], 1)


def _project(P, X):
    x = (P @ np.c_[X, np.ones(len(X))].T).T
    return x[:, :2] / x[:, 2:3]


def dlt(P1, P2, x1, x2):
    """Linear triangulation in float64: per point the right singular vector of A's smallest singular value."""
    out = np.zeros((len(x1), 3))
    for i, ((u1, v1), (u2, v2)) in enumerate(zip(np.asarray(x1, np.float64), np.asarray(x2, np.float64))):
        A = np.stack([u1 * P1[2] - P1[0], v1 * P1[2] - P1[1], u2 * P2[2] - P2[0], v2 * P2[2] - P2[1]])
        Xh = np.linalg.svd(A)[2][-1]
        out[i] = Xh[:3] / Xh[3]
    return out


def _cases():
    for name in RIGS:
        P1, P2 = _rigs.matrices(name)
        yield name, P1, P2, _scene(300, len(name) + ord(name[-1]))
    for seed in (1, 2):
        P1, P2, X = _rigs.general_matrices(seed)
        yield f"general{seed}", P1, P2, X


CASES = list(_cases())


@pytest.mark.parametrize("name,P1,P2,X", CASES, ids=[c[0] for c in CASES])
def test_triangulate_against_numpy_dlt(oracle, name, P1, P2, X):
    """The oracle's float32 points against the float64 DLT of the same float32 pixels: within float32 rounding of the
    result (rel. 1e-5 of the point's norm; measured <= 1.5e-7 on every case), for exact and noisy correspondences.  Exact
    ones also give back the planted points, to what float32 pixels allow."""
    rng = np.random.default_rng(7)
    x1e, x2e = _project(P1, X).astype(np.float32), _project(P2, X).astype(np.float32)
    for noise in (0.0, 0.4):
        x1 = (x1e + rng.normal(scale=noise, size=x1e.shape)).astype(np.float32)
        x2 = (x2e + rng.normal(scale=noise, size=x2e.shape)).astype(np.float32)
        got = oracle.triangulate(P1, P2, x1, x2).astype(np.float64)
        want = dlt(P1, P2, x1, x2)
        err = np.linalg.norm(got - want, axis=1) / np.linalg.norm(want, axis=1)
        assert err.max() <= 1e-5, (name, noise, err.max())
        if noise == 0.0:
            rel = np.linalg.norm(got - X, axis=1) / np.linalg.norm(X, axis=1)
            assert np.median(rel) <= 2e-5 and rel.max() <= 2e-3, (name, np.median(rel), rel.max())


def _K(P1):
    return np.asarray(P1, np.float64)[:, :3].copy()


def _planted(K, n, n_out, seed, noise):
    X = _scene(n, seed)
    rng = np.random.default_rng(seed + 1000)
    r = rng.normal(size=3) * 0.03
    t = np.array([rng.uniform(-0.1, 0.1), rng.uniform(-0.05, 0.05), rng.uniform(-1.2, -0.6)])
    R = Rotation.from_rotvec(r).as_matrix()
    x = _project(K @ np.c_[R, t], X) + rng.normal(scale=noise, size=(n, 2))
    out = np.sort(rng.choice(n, n_out, replace=False))
    x[out] += rng.uniform(5, 40, (n_out, 2)) * rng.choice([-1, 1], (n_out, 2))
    inl = np.ones(n, np.uint8)
    inl[out] = 0
    return X.astype(np.float32), x.astype(np.float32), r, t, inl


def residuals(p, K, X, x):
    """float64 reprojection residuals (u - u_obs, v - v_obs) of pose p = (rvec, tvec), fx and fy separate."""
    R = Rotation.from_rotvec(p[:3]).as_matrix()
    Xc = X @ R.T + p[3:]
    u = K[0, 0] * Xc[:, 0] / Xc[:, 2] + K[0, 2]
    v = K[1, 1] * Xc[:, 1] / Xc[:, 2] + K[1, 2]
    return np.concatenate([u - x[:, 0], v - x[:, 1]])


# (n, n_out, seed): 25 % and 40 % outliers at 400 points, and a small set
PLANTED = [(400, 100, 31), (400, 160, 32), (60, 15, 33)]


@pytest.mark.parametrize("n,n_out,seed", PLANTED)
@pytest.mark.parametrize("name", ["R0", "R1"])
def test_pnp_ransac_mask_pose_and_lm_stationarity(oracle, name, n, n_out, seed):
    """Noise 0.02 px, 25x below reprojError 0.5: every planted inlier is within the threshold of the planted pose (and
    of any pose that fits them), every outlier is moved by 5-40 px -> the mask must be the planted set.
    Pose bound: with 0.02 px noise the refit lands within 2e-4 rad / 2e-3 m of the planted pose (measured worst over
    these sets: 2.1e-5 rad, 1.05e-4 m -- the bounds hold a 10x margin).
    Stationarity: scipy's least_squares (float64 trust region, finite-difference Jacobian) started at the returned
    pose moves it by less than 1e-9 rad / 1e-8 m and lowers the cost by less than 1e-9 relative (measured: at most
    7e-13 rad, 2e-11 m, 5e-13).  A refit whose Jacobian used fx for the y rows on R1 stops 7e-8-3e-7 rad, 3e-7-1e-6 m
    and 1.6e-6-8e-6 of the cost away from the minimum.
    Only K = P1[:, :3] enters the solver: R2 and R3 share R0's K1, so R0 and R1 are the distinct cases."""
    K = _K(_rigs.matrices(name)[0])
    X, x, r, t, inl = _planted(K, n, n_out, seed, 0.02)
    res = oracle.pnp_ransac(X, x, K)
    assert res["ok"] == 1
    assert np.array_equal(res["mask"], inl), (name, int((res["mask"] != inl).sum()))
    assert res["n_inliers"] == inl.sum()
    dr = np.linalg.norm(Rotation.from_matrix(res["R"] @ Rotation.from_rotvec(r).as_matrix().T).as_rotvec())
    assert dr <= 2e-4 and np.abs(res["tvec"] - t).max() <= 2e-3, (name, dr, np.abs(res["tvec"] - t).max())
    m = res["mask"].astype(bool)
    Xi, xi = X[m].astype(np.float64), x[m].astype(np.float64)
    p0 = np.r_[res["rvec"], res["tvec"]]
    sol = least_squares(residuals, p0, args=(K, Xi, xi), method="trf", xtol=1e-15, ftol=1e-15, gtol=1e-15,
                        x_scale="jac")
    c0 = 0.5 * np.sum(residuals(p0, K, Xi, xi) ** 2)
    assert sol.cost <= c0 * (1 + 1e-12)
    assert (c0 - sol.cost) <= 1e-9 * c0, (name, c0, sol.cost)
    assert np.abs(sol.x[:3] - p0[:3]).max() <= 1e-9 and np.abs(sol.x[3:] - p0[3:]).max() <= 1e-8, (name, sol.x - p0)


@pytest.mark.parametrize("name", ["R0", "R1"])
def test_p3p_and_epnp_branches_with_fx_ne_fy(oracle, name):
    """n = 4 takes the P3P kernel (one model from all four points, LM refit), n >= 5 EPnP; exact projections through the
    rig's K give back the planted pose.  On R1 (fy = 0.85 fx) a solver that used fx for y would miss it by far."""
    K = _K(_rigs.matrices(name)[0])
    ok4 = 0
    for seed in range(12):
        X, x, r, t, _ = _planted(K, 4, 0, 200 + seed, 0.0)
        res = oracle.pnp_ransac(X, x, K)
        if res["ok"]:
            ok4 += 1
            assert res["n_inliers"] == 4 and res["ransac_iters"] == 1
            assert np.abs(res["tvec"] - t).max() < 1e-3 and np.abs(res["rvec"] - r).max() < 1e-4, (name, seed)
            assert np.abs(residuals(np.r_[res["rvec"], res["tvec"]], K, X.astype(np.float64), x.astype(np.float64))).max() < 1e-3
    assert ok4 >= 10
    for n in (5, 6, 12, 40):
        X, x, r, t, _ = _planted(K, n, 0, 300 + n, 0.0)
        res = oracle.pnp_ransac(X, x, K)
        assert res["ok"] == 1 and res["n_inliers"] == n, (name, n)
        assert np.abs(res["tvec"] - t).max() < 1e-3 and np.abs(res["rvec"] - r).max() < 1e-4, (name, n)
        if n >= 6:
            Re, te = oracle.epnp(X, x, K[0, 0], K[1, 1], K[0, 2], K[1, 2])
            R = Rotation.from_rotvec(r).as_matrix()
            assert np.allclose(Re, R, atol=1e-4) and np.allclose(te, t, atol=1e-3), (name, n)
