"""Planted-pose PnP inputs that leave general position: exactly planar, near-planar, collinear, clustered, duplicated
and far / mixed-depth object points, plus the ordinary box at the point counts where the kernels change lanes, waves
and chunks.  numpy and scipy only -- no GPU, no oracle: tests/test_pnp_cases.py shows on the CPU oracle that each
family reaches the branch it is meant to reach, tests/test_gpu_pnp_degenerate.py compares the HIP solver with the
oracle on them.

Every case starts from the same three draws of default_rng(seed) as tests/test_gpu_parity_pose.py::_scene
(a ~ U(-8,8), b ~ U(-2,1.6), z ~ U(5,40)) and the planted pose of its _planted (default_rng(seed + 100): rvec ~
N(0, 0.03), t = (+-0.1, +-0.05, -1.2..-0.6), pixel noise, then the outliers).  What a family adds beyond a, b, z
(which points leave the wall, per-point scales, the jitter of a near-line) comes from default_rng(seed + 200), so the
pose stream is the same for every family.  The object points are rounded to float32 BEFORE they are projected: the
image points belong to the float32 points the solver is given ("exactly planar in float32" stays exact)."""
import numpy as np
from scipy.spatial.transform import Rotation

K = np.array([[718.856, 0, 607.193], [0, 718.856, 185.216], [0, 0, 1.0]])
P1 = np.hstack([K, np.zeros((3, 1))])
P2 = np.hstack([K, K @ np.array([[-0.537], [0], [0]])])

SEED = 7
COUNTS = [(5, 0), (6, 0), (63, 20), (64, 20), (65, 20), (255, 80), (256, 80), (257, 80), (511, 160), (512, 160), (513, 160)]
FEW_COUNTS = [(6, 0), (65, 20), (257, 80)]
ALL_COUNT_KINDS = ("box", "tilted")
OTHER_KINDS = ("wall", "ground", "wall_off_1", "wall_off_3", "wall_off_10", "wall_tri", "far", "mixedfar", "dups",
               "line", "nearline", "cluster")
PLANAR_KINDS = ("wall", "ground")                          # exactly coplanar: every EPnP hypothesis is NaN
CAPPED_KINDS = ("line", "nearline", "cluster")             # the data does not determine the pose: the refit runs to its cap
CONVERGING_KINDS = ("box", "tilted", "wall_tri", "dups", "mixedfar")

# (kind, n, n_out) of every case; the seed of a case is SEED unless SEEDS names another (with the reason)
CASES = [(k, n, o) for k in ALL_COUNT_KINDS for n, o in COUNTS] + [(k, n, o) for k in OTHER_KINDS for n, o in FEW_COUNTS]
# `line`: with seed 7 the 257-point refit converges in 3 iterations (the SVD solve's singular-value threshold drops the
# free rotation about the line) and the 65-point case keeps 5 of its 8 one-ulp reruns; seed 11 runs both to the cap and
# keeps 8 and 7 (seeds 7..14 tried: 9, 11 and 13 reach the cap at both counts, 9 keeps 3 of 8 at 65 points).
SEEDS = {("line", n, o): 11 for n, o in FEW_COUNTS}


def case_id(case):
    return "%s-%d-%d" % case


def seed_of(case):
    return SEEDS.get(tuple(case), SEED)


def project(P, X):
    x = (P @ np.hstack([X, np.ones((len(X), 1))]).T).T
    return x[:, :2] / x[:, 2:3]


def _points(kind, n, seed, triangulate):
    rng = np.random.default_rng(seed)
    a, b, z = rng.uniform(-8, 8, n), rng.uniform(-2, 1.6, n), rng.uniform(5, 40, n)
    ex = np.random.default_rng(seed + 200)
    one = np.ones(n)
    if kind == "box":
        X = np.stack([a, b, z], 1)
    elif kind in ("wall", "wall_tri") or kind.startswith("wall_off_"):
        X = np.stack([a, b, 12 * one], 1)
        if kind.startswith("wall_off_"):
            k = min(int(kind[len("wall_off_"):]), n)
            off = ex.choice(n, k, replace=False)
            X[off, 2] += ex.uniform(-6, 6, k)
    elif kind == "ground":
        X = np.stack([a, 1.65 * one, z], 1)
    elif kind == "tilted":
        X = np.stack([a, b, 12 + 0.5 * a + 0.25 * b], 1)
    elif kind == "far":
        X = np.stack([a, b, z], 1) * ex.uniform(100, 500, n)[:, None]
    elif kind == "mixedfar":
        X = np.stack([a, b, z], 1)
        X[n // 2:] *= ex.uniform(100, 500, n - n // 2)[:, None]
    elif kind == "dups":
        X = np.stack([a, b, z], 1)[ex.integers(0, max(3, n // 8), n)]
    elif kind in ("line", "nearline"):
        X = np.stack([a, 0.1 * a + 0.5, 12 + 0.5 * a], 1)
        if kind == "nearline":
            X[:, 1:] += ex.normal(scale=1e-3, size=(n, 2))
    elif kind == "cluster":
        X = np.array([0.5, -0.2, 9.0]) + ex.normal(scale=1e-3, size=(n, 3))
    else:
        raise ValueError("unknown kind %r" % (kind,))
    X = X.astype(np.float32)
    if kind == "wall_tri":
        # the wall as a stereo front end would hand it over: seen by both cameras (float32 pixels, no pixel noise) and
        # triangulated -- near-planar, the Z spread is the float32 rounding of the pixels carried through the baseline
        if triangulate is None:
            raise ValueError("wall_tri needs triangulate=(P1, P2, x1, x2) -> X; the tests pass oracle.triangulate")
        Xd = X.astype(np.float64)
        X = np.ascontiguousarray(triangulate(P1, P2, project(P1, Xd).astype(np.float32), project(P2, Xd).astype(np.float32)),
                                 np.float32).reshape(n, 3)
    return X


def make(kind, n, seed, n_out, noise=0.02, triangulate=None):
    """-> X (n,3) float32, x (n,2) float32, rvec, t: object points of family `kind`, their images under the planted
    pose with `noise` px of Gaussian noise, `n_out` of them displaced by 5-40 px per axis."""
    X = _points(kind, n, seed, triangulate)
    rng = np.random.default_rng(seed + 100)
    r = rng.normal(size=3) * 0.03
    t = np.array([rng.uniform(-0.1, 0.1), rng.uniform(-0.05, 0.05), rng.uniform(-1.2, -0.6)])
    R = Rotation.from_rotvec(r).as_matrix()
    x = project(np.hstack([K @ R, (K @ t)[:, None]]), X.astype(np.float64)) + rng.normal(scale=noise, size=(n, 2))
    out = rng.choice(n, n_out, replace=False)
    x[out] += rng.uniform(5, 40, (n_out, 2)) * rng.choice([-1, 1], (n_out, 2))
    return X, x.astype(np.float32), r, t


def make_case(case, triangulate=None):
    kind, n, n_out = case
    return make(kind, n, seed_of(case), n_out, triangulate=triangulate)


def cost(X, x, mask, R, t):
    """Sum of squared reprojection residuals (px^2, float64) of the points selected by `mask` under (R, t)."""
    m = np.asarray(mask).astype(bool)
    Xc = np.asarray(X, np.float64)[m] @ np.asarray(R, np.float64).T + np.asarray(t, np.float64)
    p = Xc @ K.T
    d = p[:, :2] / p[:, 2:3] - np.asarray(x, np.float64)[m]
    return float((d * d).sum())


def ulp_nudged(X, mask, rng):
    """A copy of X with the Z of one randomly chosen inlier moved to the next float32 above it."""
    i = int(rng.choice(np.flatnonzero(mask)))
    Xp = np.array(X, np.float32, copy=True)
    Xp[i, 2] = np.nextafter(Xp[i, 2], np.float32(np.inf))
    return Xp


# ---- the oracle's side of a case, computed once per session and shared (the oracle module is handed in: this file
# imports neither it nor the package) -----------------------------------------------------------------------------
DISCRETE = ("ok", "ransac_iters", "best_iter", "n_inliers", "lm_iters")
_REF, _SENS = {}, {}


def same_discrete(a, b):
    return all(a[k] == b[k] for k in DISCRETE) and np.array_equal(a["mask"], b["mask"])


def reference(oracle, case):
    """dict(X, x, rvec, t, ref, cost_start, cost_ref) of a case: `ref` is oracle.pnp_ransac's result; cost_start is the
    cost of the RANSAC winner before the refit (a second oracle run with COMPAT_PNP_REFIT = 1, which returns the
    winner unrefined; the knob is restored), cost_ref the oracle's final cost, both over the oracle's mask (None when
    ok == 0).  The arrays are read-only."""
    case = tuple(case)
    if case not in _REF:
        if case[0] == "box_edge":
            X, x, r, t, _ = make_edge_case(oracle, case)
        else:
            X, x, r, t = make_case(case, triangulate=oracle.triangulate)
        ref = oracle.pnp_ransac(X, x, K)
        c0 = c1 = None
        if ref["ok"]:
            old = oracle.set_opencv_compat(oracle.COMPAT_PNP_REFIT, 1)
            try:
                start = oracle.pnp_ransac(X, x, K)
            finally:
                oracle.set_opencv_compat(oracle.COMPAT_PNP_REFIT, old)
            assert start["lm_iters"] == 0 and np.array_equal(start["mask"], ref["mask"])
            c0 = cost(X, x, ref["mask"], start["R"], start["tvec"])
            c1 = cost(X, x, ref["mask"], ref["R"], ref["tvec"])
        for a in (X, x, ref["mask"], ref["R"], ref["rvec"], ref["tvec"]):
            a.setflags(write=False)
        _REF[case] = dict(X=X, x=x, rvec=r, t=t, ref=ref, cost_start=c0, cost_ref=c1)
    return _REF[case]


# ---- `box_edge`: the box with ONE image point moved exactly onto the inlier threshold of the winning hypothesis ----
# The threshold test is "float squared distance <= (float)(0.5 * 0.5)"; random data never lands on it (the distance
# is a sum of squares of float32 pixel differences: only (+-0.5, 0) and (0, +-0.5) give 0.25f), so the box cases cannot
# tell "<=" from "<".  The winner of the oracle's search is rebuilt here -- its subset from the cv::RNG(-1) stream,
# its (R, t) from oracle.epnp on that subset, bit for bit what the search computed -- an outlier outside the subset is
# projected with it the way computeError does (double, stored to float), and its image point is set to (px + 0.5, py):
# both representable, so the float distance is 0.25f exactly and the point is an inlier by equality alone.
EDGE_CASES = [("box_edge", 65, 20), ("box_edge", 257, 80)]


def ransac_subset(oracle, n, it):
    """The five indices getSubset draws for iteration `it` of an n-point search (n > 5)."""
    draws, pos = oracle.rng_sequence(16 * (it + 1) + 64), 0
    for _ in range(it + 1):
        idx = []
        while len(idx) < 5:
            if pos == len(draws):
                draws = oracle.rng_sequence(2 * len(draws))
            j = draws[pos] % n
            pos += 1
            if j not in idx:
                idx.append(j)
    return idx


def hypothesis(oracle, X, x, idx):
    """(R, t) of the EPnP hypothesis on the points idx, from the inputs solvePnP(EPNP) hands it."""
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    pws = X[idx].astype(np.float64)
    m = x[idx].astype(np.float64)
    xn = ((m[:, 0] - cx) * (1. / fx)).astype(np.float32).astype(np.float64)      # undistortPoints: float out
    yn = ((m[:, 1] - cy) * (1. / fy)).astype(np.float32).astype(np.float64)
    return oracle.epnp(pws, np.stack([xn * fx + cx, yn * fy + cy], 1), fx, fy, cx, cy)


def projected_f32(R, t, X):
    """cvProjectPoints2 in double (sums left to right), stored to float."""
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    Xd = X.astype(np.float64)
    p = [R[i, 0] * Xd[:, 0] + R[i, 1] * Xd[:, 1] + R[i, 2] * Xd[:, 2] + t[i] for i in range(3)]
    z = np.where(p[2] != 0, 1. / np.where(p[2] != 0, p[2], 1.), 1.)
    return np.stack([((p[0] * z) * fx + cx).astype(np.float32), ((p[1] * z) * fy + cy).astype(np.float32)], 1)


def reproj_err2_f32(R, t, X, x):
    """PnPRansacCallback::computeError: the float squared distance to the float projection."""
    d = x.astype(np.float32) - projected_f32(R, t, X)
    s = np.float32(0) + d[:, 0] * d[:, 0]
    return s + d[:, 1] * d[:, 1]


def make_edge_case(oracle, case):
    """-> X, x, rvec, t, j: the box case of the same (n, n_out) and seed with image point j on the winner's threshold."""
    _, n, n_out = case
    X, x0, r, t = make("box", n, seed_of(case), n_out)
    box = oracle.pnp_ransac(X, x0, K)
    # The moved point can hand the search to another hypothesis (one inlier more somewhere else too): move it onto the
    # NEW winner's threshold then, and take the first outlier, from the last index down, for which that settles -- the
    # winner stays, and one float32 ulp further out the point is lost and nothing else changes.
    for j in [i for i in range(n - 1, -1, -1) if not box["mask"][i]]:
        x, ref = x0.copy(), box
        for _ in range(4):
            idx = ransac_subset(oracle, n, ref["best_iter"])
            if j in idx:
                break
            R, tt = hypothesis(oracle, X, x, idx)
            assert np.array_equal(reproj_err2_f32(R, tt, X, x) <= np.float32(0.25), ref["mask"].astype(bool)), \
                "the rebuilt winner is not the search's"
            x[j] = projected_f32(R, tt, X)[j] + np.float32([0.5, 0])
            assert reproj_err2_f32(R, tt, X, x)[j] == np.float32(0.25)
            new = oracle.pnp_ransac(X, x, K)
            if new["best_iter"] == ref["best_iter"]:
                xo = x.copy()
                xo[j, 0] = np.nextafter(xo[j, 0], np.float32(np.inf))
                out = oracle.pnp_ransac(X, xo, K)
                if (new["mask"][j] == 1 and out["mask"][j] == 0 and out["best_iter"] == new["best_iter"]
                        and out["n_inliers"] == new["n_inliers"] - 1):
                    return X, x, r, t, j
                break
            ref = new
    raise AssertionError("no outlier of %s settles on the winner's threshold" % (case_id(case),))


N_RERUNS, MIN_KEPT = 8, 6


def sensitivity(oracle, case):
    """(S, kept): the oracle's own sensitivity to ONE float32 ulp of input.  Eight reruns, each with one randomly
    chosen inlier's Z moved to the next float32 (default_rng(seed + 300)); the reruns whose discrete fields and mask
    equal the unperturbed ones are kept, and S is the largest relative change of their final cost, evaluated on the
    unperturbed points and mask."""
    case = tuple(case)
    if case not in _SENS:
        c = reference(oracle, case)
        rng = np.random.default_rng(seed_of(case) + 300)
        rel = []
        for _ in range(N_RERUNS):
            rp = oracle.pnp_ransac(ulp_nudged(c["X"], c["ref"]["mask"], rng), c["x"], K)
            if same_discrete(rp, c["ref"]):
                rel.append(abs(cost(c["X"], c["x"], c["ref"]["mask"], rp["R"], rp["tvec"]) - c["cost_ref"]) / c["cost_ref"])
        _SENS[case] = (max(rel) if rel else 0.0, len(rel))
    return _SENS[case]


# ---- which solver route would the refit take?  A numpy twin of the refit's control flow (CvLevMarq on 6 parameters as
# oracle/pnp.c restates it: lambda = 10^k, accept / reject / stop rules) that records, for every damped system it solves,
# the smallest Cholesky pivot relative to its diagonal entry -- the quantity the device's chol_solve6_d compares with
# 1e-10 before it hands the system to the SVD route.  Not bit-exact (numpy sums, LAPACK SVD); it is validated by
# reproducing the oracle's lm_iters, and used to say how near a case comes to the criterion.
def _lm_project(oracle, param, X, m, jac):
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    R, dR = oracle.rodrigues_vec2mat(param[:3], jac=True)
    P = X @ R.T + param[3:]
    z = 1.0 / P[:, 2]
    x, y = P[:, 0] * z, P[:, 1] * z
    err = np.stack([x * fx + cx - m[:, 0], y * fy + cy - m[:, 1]], 1).reshape(-1)
    if not jac:
        return err, None
    J = np.zeros((2 * len(X), 6))
    for j in range(3):
        d0 = X @ dR[j].reshape(3, 3).T
        J[0::2, j] = fx * z * (d0[:, 0] - x * d0[:, 2])
        J[1::2, j] = fy * z * (d0[:, 1] - y * d0[:, 2])
    J[0::2, 3], J[0::2, 5] = fx * z, -fx * x * z
    J[1::2, 4], J[1::2, 5] = fy * z, -fy * y * z
    return err, J


def _min_pivot_ratio(A):
    L, worst = np.zeros((6, 6)), np.inf
    for i in range(6):
        for j in range(i + 1):
            s = A[i, j] - L[i, :j] @ L[j, :j]
            if i == j:
                worst = min(worst, s / A[i, i])
                L[i, i] = np.sqrt(s) if s > 0 else np.nan
            else:
                L[i, j] = s / L[j, j]
    return worst if worst == worst else -np.inf


def refit_trace(oracle, case):
    """(lm_iters, [(lambda exponent, smallest pivot / diagonal)] per solve) of the twin's refit from the oracle's
    RANSAC winner over the oracle's mask; None when the case has no solution."""
    c = reference(oracle, case)
    if not c["ref"]["ok"]:
        return None
    old = oracle.set_opencv_compat(oracle.COMPAT_PNP_REFIT, 1)
    try:
        start = oracle.pnp_ransac(c["X"], c["x"], K)
    finally:
        oracle.set_opencv_compat(oracle.COMPAT_PNP_REFIT, old)
    m = c["ref"]["mask"].astype(bool)
    X, img = c["X"][m].astype(np.float64), c["x"][m].astype(np.float64)
    param = np.concatenate([start["rvec"], start["tvec"]])
    lam10, iters, solves = -3, 0, []
    while True:
        err, J = _lm_project(oracle, param, X, img, True)
        JtJ, Jte, prev = J.T @ J, J.T @ err, param.copy()
        if iters == 0:
            prev_norm = np.linalg.norm(err)
        while True:
            A = JtJ.copy()
            A[np.diag_indices(6)] *= 1 + 10.0 ** lam10
            solves.append((lam10, _min_pivot_ratio(A)))
            U, W, Vt = np.linalg.svd(A)                         # cv::solve(DECOMP_SVD): singular values <= 2 eps sum(W) dropped
            keep = W > np.finfo(float).eps * 2 * W.sum()
            param = prev - (Vt[keep].T * ((U[:, keep].T @ Jte) / W[keep])).sum(1)
            norm = np.linalg.norm(_lm_project(oracle, param, X, img, False)[0])
            if norm > prev_norm and lam10 < 16:
                lam10 += 1
                continue
            if norm > prev_norm:
                lam10 += 1
            lam10 = max(lam10 - 1, -16)
            iters += 1
            prev_norm = norm
            break
        if iters >= 20 or np.linalg.norm(param - prev) / np.linalg.norm(prev) < 1.1920928955078125e-07:
            return iters, solves
