"""Two-view robust pose refinement (rules R1-R7) restated in numpy float64.

The reference of tests/test_refine_ref.py and tests/test_gpu_refine.py: no project imports, no oracle.
State (R, t) with Y = R X + t; left-multiplicative update (R, t) <- exp(xi) (R, t), xi = (rho, phi).
View L projects with [K1 | 0], K1 = (fx, fy, cx, cy) of P1 (skew and 4th column ignored); view R with the full P2.
"""
import math

import numpy as np

TAU2, TAU4 = 5.991, 9.488              # chi-square 95 % points, 2 and 4 degrees of freedom
MIN_DEPTH = 1e-6
APPLIED, KEPT_PNP, SKIPPED = 0, 1, 2


def mm(A, B):
    """A @ B by elementwise products and ordered sums (no BLAS: the same roundings on every machine)."""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    if B.ndim == 1:
        return (A * B[None, :]).sum(1)
    return (A[:, :, None] * B[None, :, :]).sum(1)


def rows_times(X, M):
    """X M^T for rows X (n, 3) and a 3x3 M, column by column."""
    return X[:, 0:1] * M[None, :, 0] + X[:, 1:2] * M[None, :, 1] + X[:, 2:3] * M[None, :, 2]


def hat(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def se3_exp(xi):
    """(E, V rho): closed form; the series form below |phi| < 1e-10."""
    rho, phi = np.asarray(xi[:3], np.float64), np.asarray(xi[3:], np.float64)
    th2 = phi[0] * phi[0] + phi[1] * phi[1] + phi[2] * phi[2]
    th = math.sqrt(th2)
    if th < 1e-10:
        A, B, C = 1.0, 0.5, 1.0 / 6.0
    else:
        sh = math.sin(0.5 * th)
        A = math.sin(th) / th
        B = 2.0 * sh * sh / th2
        C = (th - math.sin(th)) / (th2 * th)
    K = hat(phi)
    K2 = mm(K, K)
    E = np.eye(3) + A * K + B * K2
    V = np.eye(3) + B * K + C * K2
    return E, mm(V, rho)


def rodrigues(rvec):
    """Rotation matrix of a rotation vector (cv::Rodrigues)."""
    r = np.asarray(rvec, np.float64)
    th = math.sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2])
    if th < 2.220446049250313e-16:
        return np.eye(3)
    k = r / th
    c, s = math.cos(th), math.sin(th)
    return c * np.eye(3) + (1.0 - c) * np.outer(k, k) + s * hat(k)


def so3_log(R):
    """Rotation vector of a rotation matrix."""
    v = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s = math.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    c = 0.5 * (R[0, 0] + R[1, 1] + R[2, 2] - 1.0)
    th = math.atan2(s, c)
    if s >= 1e-5:
        return v * (th / s)
    if c > 0:
        return v * (th / s) if s >= 1e-10 else v
    # near pi: the axis from the diagonal, signs from the off-diagonal sums (cv::Rodrigues)
    ax = np.sqrt(np.maximum((np.diag(R) + 1.0) * 0.5, 0.0))
    if R[0, 1] < 0:
        ax[1] = -ax[1]
    if R[0, 2] < 0:
        ax[2] = -ax[2]
    if abs(ax[0]) < abs(ax[1]) and abs(ax[0]) < abs(ax[2]) and (R[1, 2] > 0) != (ax[1] * ax[2] > 0):
        ax[2] = -ax[2]
    return ax * (th / math.sqrt(ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2]))


def views_of(P1, P2, d):
    P1 = np.asarray(P1, np.float64).reshape(3, 4)
    ML = np.array([[P1[0, 0], 0.0, P1[0, 2]], [0.0, P1[1, 1], P1[1, 2]], [0.0, 0.0, 1.0]])
    vs = [(ML, np.zeros(3))]
    if d == 4:
        P2 = np.asarray(P2, np.float64).reshape(3, 4)
        vs.append((P2[:, :3].copy(), P2[:, 3].copy()))
    return vs


def evaluate(X, obs, views, R, t, sigma=1.0, jac=True):
    """Residuals r (n, d), c = |r|^2 / sigma^2, projectable flags and Jacobians J (n, d, 6) at (R, t) (R3, R4)."""
    n = X.shape[0]
    Y = rows_times(X, R) + t
    d = 2 * len(views)
    r = np.zeros((n, d))
    J = np.zeros((n, d, 6)) if jac else None
    proj = np.ones(n, bool)
    for v, (M, p4) in enumerate(views):
        h = rows_times(Y, M) + p4
        ok = h[:, 2] > MIN_DEPTH
        proj &= ok
        h2 = np.where(ok, h[:, 2], 1.0)
        u, w = h[:, 0] / h2, h[:, 1] / h2
        r[:, 2 * v] = u - obs[v][:, 0]
        r[:, 2 * v + 1] = w - obs[v][:, 1]
        if jac:
            a = (M[0][None, :] - u[:, None] * M[2][None, :]) / h2[:, None]
            b = (M[1][None, :] - w[:, None] * M[2][None, :]) / h2[:, None]
            J[:, 2 * v, :3] = a
            J[:, 2 * v, 3:] = np.cross(Y, a)          # -a^T [Y]x
            J[:, 2 * v + 1, :3] = b
            J[:, 2 * v + 1, 3:] = np.cross(Y, b)
    r[~proj] = 0.0
    if jac:
        J[~proj] = 0.0
    c = (r * r).sum(1) / (sigma * sigma)
    return r, c, proj, J


def depth_margin(X, views, R, t, active, t1_views=()):
    """The smallest distance of an active point's depth h_3 from the projectability cut, over `views` of Y = R X + t and
    `t1_views` of X itself: how far "not projectable" is from hanging on a last bit."""
    Y = rows_times(X, R) + t
    hs = [rows_times(Z, M)[:, 2] + p4[2] for Z, vs in ((Y, views), (X, t1_views)) for M, p4 in vs]
    # (a NaN depth fails the comparison whatever its bits: it is not near the cut)
    far = [np.abs(h[active] - MIN_DEPTH) for h in hs]
    return min([float(np.min(f[~np.isnan(f)])) for f in far if not np.isnan(f).all()], default=np.inf)


def chol_solve6(A, b):
    """6x6 Cholesky solve, row by row; fails unless every pivot is > 0."""
    L = np.zeros((6, 6))
    for i in range(6):
        for j in range(i + 1):
            s = A[i, j]
            for k in range(j):
                s -= L[i, k] * L[j, k]
            if i == j:
                if not s > 0.0:
                    return False, None
                L[i, i] = np.sqrt(s)
            else:
                L[i, j] = s / L[j, j]
    y = np.zeros(6)
    for i in range(6):
        s = b[i]
        for k in range(i):
            s -= L[i, k] * y[k]
        y[i] = s / L[i, i]
    x = np.zeros(6)
    for i in range(5, -1, -1):
        s = y[i]
        for k in range(i + 1, 6):
            s -= L[k, i] * x[k]
        x[i] = s / L[i, i]
    return True, x


def _sums(r, c, J, active, tau, robust, sigma):
    """cost, H, g over the active set (R5, R6)."""
    w = np.ones_like(c)
    rho = c.copy()
    if robust:
        big = c > tau
        cs = np.where(big, c, 1.0)
        w = np.where(big, np.sqrt(tau / cs), 1.0)
        rho = np.where(big, 2.0 * np.sqrt(tau * cs) - tau, c)
    w = np.where(active, w, 0.0)
    # The cost as an unevaluated pair (hi, lo), hi the correctly rounded sum of the terms and lo what is left of it: "the cost
    # decreases" is decided on the pair.  A plain double sum of ~1000 terms carries ~1e-13 of rounding noise, which decides the
    # accept test for steps below ~1e-9 and with it where the iteration stops; the terms themselves are good to ~1e-16.
    terms = [float(v) for v in rho[active]]
    hi = math.fsum(terms)
    cost = (hi, math.fsum(terms + [-hi]) if math.isfinite(hi) else 0.0)
    is2 = 1.0 / (sigma * sigma)
    # over the ACTIVE set (R5): an inactive point adds an exact zero, also where its residual is not finite (0 * NaN is not 0)
    H = np.where(active[:, None, None], w[:, None, None] * (J[:, :, :, None] * J[:, :, None, :]).sum(1), 0.0).sum(0) * is2
    g = np.where(active[:, None], w[:, None] * (J * r[:, :, None]).sum(1), 0.0).sum(0) * is2
    return cost, H, g


def refine(X, xl, xr, P1, P2, R0, t0, rounds=4, iters=10, sigma=1.0, min_inliers=6, perm=None):
    """R1-R7.  xr None: one view (d = 2).  Returns a dict; 'log' has one entry per round for fixture_ok: its exit, the smallest
    relative distance of a c_i from tau at its re-classification, the smallest relative cost difference over its accept
    decisions and 'steps', those decisions one by one (tests/_ba_ref.py keeps the same log)."""
    X = np.asarray(X, np.float64).reshape(-1, 3)
    n = X.shape[0]
    d = 2 if xr is None else 4
    tau = TAU2 if d == 2 else TAU4
    obs = [np.asarray(xl, np.float64).reshape(-1, 2)]
    if d == 4:
        obs.append(np.asarray(xr, np.float64).reshape(-1, 2))
    if perm is not None:
        X = X[perm]
        obs = [o[perm] for o in obs]
    views = views_of(P1, P2, d)
    R = np.asarray(R0, np.float64).reshape(3, 3).copy()
    t = np.asarray(t0, np.float64).reshape(3).copy()
    r, c, proj, J = evaluate(X, obs, views, R, t, sigma)
    active = proj.copy()
    total = 0
    cost_first = cost = (0.0, 0.0)
    log = []
    for rd in range(rounds):
        robust = rd < 2
        lam = 1e-4
        cost, H, g = _sums(r, c, J, active, tau, robust, sigma)
        if rd == 0:
            cost_first = cost
        how, acc_margin, steps = "iters", np.inf, []
        for _ in range(iters):
            total += 1
            A = H + lam * np.diag(np.diag(H))
            ok, xi = chol_solve6(A, -g)
            accepted = False
            if ok:
                E, Vr = se3_exp(xi)
                Rn, tn = mm(E, R), mm(E, t) + Vr
                rn, cn, pn, Jn = evaluate(X, obs, views, Rn, tn, sigma)
                if np.all(pn[active]):
                    costn, Hn, gn = _sums(rn, cn, Jn, active, tau, robust, sigma)
                    accepted = costn < cost
                    if cost[0] > 0.0:                  # how far the decision is from a tie, relative to the cost itself
                        rel = abs((cost[0] - costn[0]) + (cost[1] - costn[1])) / cost[0]
                        acc_margin = min(acc_margin, rel)
                        steps.append(("accepted" if accepted else "rejected", rel))
                else:
                    # rejected whatever the cost says: an active point is not projectable at the trial pose.  The entry names
                    # those points, the trial cost over the others and how far any active point's depth is from the cut
                    rest = active & pn
                    steps.append(("unprojectable", depth_margin(X, views, Rn, tn, active), np.flatnonzero(active & ~pn),
                                  _sums(rn, cn, Jn, rest, tau, robust, sigma)[0], cost))
            if accepted:
                R, t, r, c, proj, J, cost, H, g = Rn, tn, rn, cn, pn, Jn, costn, Hn, gn
                lam = max(lam / 10.0, 1e-12)
                if math.sqrt(float((xi * xi).sum())) < 1e-10:
                    how = "xi"
                    break
            else:
                lam *= 10.0
                if lam > 1e10:
                    how = "lambda"
                    break
        active = proj & (c <= tau)
        cp = c[proj][~np.isnan(c[proj])]          # (a NaN c_i is cut by the comparison itself, not by its distance from tau)
        near = float(np.min(np.abs(cp - tau))) / tau if len(cp) else np.inf
        log.append({"exit": how, "margin": near, "accept_margin": acc_margin, "steps": steps})
    info = (active.astype(np.float64)[:, None, None] * (J[:, :, :, None] * J[:, :, None, :]).sum(1)).sum(0) / (sigma * sigma)
    n_active = int(active.sum())
    pd, _ = chol_solve6(info, np.zeros(6))
    rvec = so3_log(R)
    finite = bool(np.all(np.isfinite(R)) and np.all(np.isfinite(t)) and np.all(np.isfinite(info)) and np.all(np.isfinite(rvec))
                  and np.isfinite(cost_first[0]) and np.isfinite(cost[0]))
    applied = n_active >= min_inliers and pd and finite
    if perm is not None:
        inv = np.empty(n, np.int64)
        inv[perm] = np.arange(n)
        active = active[inv]
    out = {"status": APPLIED if applied else KEPT_PNP, "n_points": n, "n_active": n_active, "active": active.astype(np.uint8),
           "iters": total, "views": d // 2, "info": info, "cost_first": cost_first[0], "cost_last": cost[0], "log": log,
           "R_ref": R, "t_ref": t, "rvec_ref": rvec}
    if applied:
        out.update(R=R, t=t, rvec=rvec)
    else:
        R0 = np.asarray(R0, np.float64).reshape(3, 3)
        out.update(R=R0.copy(), t=np.asarray(t0, np.float64).reshape(3).copy(), rvec=so3_log(R0))
    return out
