"""Two-frame stereo bundle adjustment restated in numpy float64: the twin of csrc/ba.hip.

The unknowns are the pose (R, t) of rule R2 and one point X_i per track; the residuals are the reprojection errors in the
views of t1 (which see X_i) and of t2 (which see Y_i = R X_i + t).  Views, the SE(3) update, the Huber rounds, the
re-classification and the accept test are those of tests/_refine_ref.py (rules R1, R2, R5, R6); what is new is that every
point is eliminated from the normal equations by its 3 x 3 Schur complement and moved together with the pose.
Residual order per point: t1_left (u, v), t1_right (u, v), t2_left (u, v) and, with d = 8, t2_right (u, v)."""
import math

import numpy as np

import _refine_ref as RR

TAU6, TAU8 = 7.815, 11.070             # chi-square 95 % points, d - 3 = 3 and 5 degrees of freedom (three are the point's)
MIN_DEPTH = RR.MIN_DEPTH
APPLIED, KEPT_PNP, SKIPPED = RR.APPLIED, RR.KEPT_PNP, RR.SKIPPED
XI_EXIT, DX_EXIT = 1e-10, 1e-9


def views_of(P1, P2):
    P1 = np.asarray(P1, np.float64).reshape(3, 4)
    P2 = np.asarray(P2, np.float64).reshape(3, 4)
    ML = np.array([[P1[0, 0], 0.0, P1[0, 2]], [0.0, P1[1, 1], P1[1, 2]], [0.0, 0.0, 1.0]])
    return [(ML, np.zeros(3)), (P2[:, :3].copy(), P2[:, 3].copy())]


def _view(Z, M, p4, o):
    """Projection of the rows Z by [M | p4] against the observations o: ok, residual (n, 2), du/dZ, dw/dZ (R3)."""
    h = RR.rows_times(Z, M) + p4
    ok = h[:, 2] > MIN_DEPTH
    h2 = np.where(ok, h[:, 2], 1.0)
    u, w = h[:, 0] / h2, h[:, 1] / h2
    a = (M[0][None, :] - u[:, None] * M[2][None, :]) / h2[:, None]
    b = (M[1][None, :] - w[:, None] * M[2][None, :]) / h2[:, None]
    return ok, np.stack([u - o[:, 0], w - o[:, 1]], 1), a, b


def evaluate(X, obs, views, R, t, sigma=1.0):
    """obs = [t1_left, t1_right, t2_left(, t2_right)].  Returns r (n, d), c, projectable, Jx (n, d, 3), Jp (n, d, 6)."""
    n, d = X.shape[0], 2 * len(obs)
    Y = RR.rows_times(X, R) + t
    r, Jx, Jp = np.zeros((n, d)), np.zeros((n, d, 3)), np.zeros((n, d, 6))
    proj = np.ones(n, bool)
    for k in range(len(obs)):
        M, p4 = views[k & 1]
        ok, rr, a, b = _view(X if k < 2 else Y, M, p4, obs[k])
        proj &= ok
        r[:, 2 * k:2 * k + 2] = rr
        if k < 2:
            Jx[:, 2 * k], Jx[:, 2 * k + 1] = a, b
        else:
            Jx[:, 2 * k], Jx[:, 2 * k + 1] = RR.rows_times(a, R.T), RR.rows_times(b, R.T)        # a^T R
            Jp[:, 2 * k, :3], Jp[:, 2 * k, 3:] = a, np.cross(Y, a)                              # -a^T [Y]x
            Jp[:, 2 * k + 1, :3], Jp[:, 2 * k + 1, 3:] = b, np.cross(Y, b)
    r[~proj] = 0.0
    Jx[~proj] = 0.0
    Jp[~proj] = 0.0
    c = (r * r).sum(1) / (sigma * sigma)
    return r, c, proj, Jx, Jp


def _weights(c, active, tau, robust):
    w, rho = np.ones_like(c), c.copy()
    if robust:
        big = c > tau
        cs = np.where(big, c, 1.0)
        w = np.where(big, np.sqrt(tau / cs), 1.0)
        rho = np.where(big, 2.0 * np.sqrt(tau * cs) - tau, c)
    return np.where(active, w, 0.0), rho


def _cost(rho, active):
    terms = [float(v) for v in rho[active]]
    hi = math.fsum(terms)
    return (hi, math.fsum(terms + [-hi]) if math.isfinite(hi) else 0.0)


def build(r, c, Jx, Jp, active, tau, robust, sigma, lam):
    """The reduced system at damping lam over the active set, and what the back-substitution needs.
    Returns cost pair, H (6, 6), g (6), sum of diag U (6), and per point (ok, L (n, 6), T (n, 6, 3), y (n, 3))."""
    w, rho = _weights(c, active, tau, robust)
    ws = w / (sigma * sigma)
    V = ws[:, None, None] * (Jx[:, :, :, None] * Jx[:, :, None, :]).sum(1)
    W = ws[:, None, None] * (Jp[:, :, :, None] * Jx[:, :, None, :]).sum(1)
    U = ws[:, None, None] * (Jp[:, :, :, None] * Jp[:, :, None, :]).sum(1)
    gx = ws[:, None] * (Jx * r[:, :, None]).sum(1)
    gp = ws[:, None] * (Jp * r[:, :, None]).sum(1)
    # 3 x 3 Cholesky of V + lam diag V, row by row; a point whose pivots are not all > 0 keeps U and g_p and is not moved
    d0 = V[:, 0, 0] + lam * V[:, 0, 0]
    ok = active & (d0 > 0.0)
    l00 = np.sqrt(np.where(ok, d0, 1.0))
    l10 = V[:, 1, 0] / l00
    d1 = (V[:, 1, 1] + lam * V[:, 1, 1]) - l10 * l10
    ok &= d1 > 0.0
    l11 = np.sqrt(np.where(ok, d1, 1.0))
    l20 = V[:, 2, 0] / l00
    l21 = (V[:, 2, 1] - l20 * l10) / l11
    d2 = ((V[:, 2, 2] + lam * V[:, 2, 2]) - l20 * l20) - l21 * l21
    ok &= d2 > 0.0
    l22 = np.sqrt(np.where(ok, d2, 1.0))
    # T = W L^-T (rows solve L T_p^T = W_p^T), y = L^-1 gx
    T = np.zeros_like(W)
    T[:, :, 0] = W[:, :, 0] / l00[:, None]
    T[:, :, 1] = (W[:, :, 1] - l10[:, None] * T[:, :, 0]) / l11[:, None]
    T[:, :, 2] = ((W[:, :, 2] - l20[:, None] * T[:, :, 0]) - l21[:, None] * T[:, :, 1]) / l22[:, None]
    y = np.zeros_like(gx)
    y[:, 0] = gx[:, 0] / l00
    y[:, 1] = (gx[:, 1] - l10 * y[:, 0]) / l11
    y[:, 2] = ((gx[:, 2] - l20 * y[:, 0]) - l21 * y[:, 1]) / l22
    T[~ok] = 0.0
    y[~ok] = 0.0
    Hi = U - (T[:, :, None, :] * T[:, None, :, :]).sum(3)
    gi = gp - (T * y[:, None, :]).sum(2)
    H, g = Hi[active].sum(0), gi[active].sum(0)
    dU = np.diagonal(U, axis1=1, axis2=2)[active].sum(0)
    L = np.stack([l00, l10, l11, l20, l21, l22], 1)
    return _cost(rho, active), H, g, dU, (ok, L, T, y)


def back_substitute(pts, xi):
    """dX_i = -V*^-1 (gx + W^T xi) = -L^-T (y + T^T xi); 0 for the points that are not moved."""
    ok, L, T, y = pts
    z = y + (T * xi[None, :, None]).sum(1)
    l00, l10, l11, l20, l21, l22 = (L[:, k] for k in range(6))
    d2 = z[:, 2] / l22
    d1 = (z[:, 1] - l21 * d2) / l11
    d0 = ((z[:, 0] - l10 * d1) - l20 * d2) / l00
    dX = -np.stack([d0, d1, d2], 1)
    dX[~ok] = 0.0
    return dX


def chol_ok(A):
    return RR.chol_solve6(A, np.zeros(6))[0]


def refine_ba(X0, t1l, t1r, t2l, t2r, P1, P2, R0, t0, rounds=4, iters=10, sigma=1.0, min_inliers=6):
    """The whole stage.  t2r None: d = 6.  X0 is the float32 triangulation; returns a dict as _refine_ref.refine does, plus
    'X' (n, 3), the points that stand, and 'log', one entry per round: its exit, the smallest relative distance of a c_i
    from tau at its re-classification, the smallest relative cost difference |cost' - cost| / cost over its accept decisions, and
    'steps', those decisions one by one (accepted / rejected, that difference)."""
    X = np.asarray(X0, np.float32).reshape(-1, 3).astype(np.float64)
    n = X.shape[0]
    obs = [np.asarray(o, np.float64).reshape(-1, 2) for o in (t1l, t1r, t2l)]
    if t2r is not None:
        obs.append(np.asarray(t2r, np.float64).reshape(-1, 2))
    d = 2 * len(obs)
    tau = TAU6 if d == 6 else TAU8
    views = views_of(P1, P2)
    R = np.asarray(R0, np.float64).reshape(3, 3).copy()
    t = np.asarray(t0, np.float64).reshape(3).copy()
    Xs = X.copy()
    ev = evaluate(X, obs, views, R, t, sigma)
    active = ev[2].copy()
    total, cost_first, cost, log = 0, (0.0, 0.0), (0.0, 0.0), []
    for rd in range(rounds):
        robust = rd < 2
        lam, how, acc_margin, steps = 1e-4, "iters", np.inf, []
        for it in range(iters):
            total += 1
            r, c, proj, Jx, Jp = ev
            cost_b, H, g, dU, pts = build(r, c, Jx, Jp, active, tau, robust, sigma, lam)
            if it == 0:
                cost = cost_b
                if rd == 0:
                    cost_first = cost
            ok, xi = RR.chol_solve6(H + lam * np.diag(dU), -g)
            accepted = False
            if ok:
                dX = back_substitute(pts, xi)
                E, Vr = RR.se3_exp(xi)
                Rn, tn, Xn = RR.mm(E, R), RR.mm(E, t) + Vr, X + dX
                evn = evaluate(Xn, obs, views, Rn, tn, sigma)
                if np.all(evn[2][active]):
                    costn = _cost(_weights(evn[1], active, tau, robust)[1], active)
                    accepted = costn < cost
                    if cost[0] > 0.0:                  # how far the decision is from a tie, relative to the cost itself
                        rel = abs((cost[0] - costn[0]) + (cost[1] - costn[1])) / cost[0]
                        acc_margin = min(acc_margin, rel)
                        steps.append(("accepted" if accepted else "rejected", rel))
                else:
                    # rejected whatever the cost says: an active point is not projectable at the trial estimate.  The entry
                    # names those points, the trial cost over the others and how far any active point's depth is from the cut
                    rest = active & evn[2]
                    steps.append(("unprojectable", RR.depth_margin(Xn, views[:len(obs) - 2], Rn, tn, active, t1_views=views),
                                  np.flatnonzero(active & ~evn[2]), _cost(_weights(evn[1], rest, tau, robust)[1], rest), cost))
            if accepted:
                R, t, X, ev, cost = Rn, tn, Xn, evn, costn
                lam = max(lam / 10.0, 1e-12)
                step = math.sqrt(float((dX * dX).sum(1).max())) if n else 0.0
                if math.sqrt(float((xi * xi).sum())) < XI_EXIT and step < DX_EXIT:
                    how = "xi"
                    break
            else:
                lam *= 10.0
                if lam > 1e10:
                    how = "lambda"
                    break
        _, c, proj, _, _ = ev
        active = proj & (c <= tau)
        cp = c[proj][~np.isnan(c[proj])]          # (a NaN c_i is cut by the comparison itself, not by its distance from tau)
        near = float(np.min(np.abs(cp - tau))) / tau if len(cp) else np.inf
        if not active.all():
            # a rejected point's position means nothing (under Huber a gross outlier wanders to 1e11 m): it returns to its
            # triangulation, which is also what a later re-admission is judged on
            X = np.where(active[:, None], X, Xs)
            ev = evaluate(X, obs, views, R, t, sigma)
        log.append({"exit": how, "margin": near, "accept_margin": acc_margin, "steps": steps})
    r, c, proj, Jx, Jp = ev
    _, info, _, _, _ = build(r, c, Jx, Jp, active, tau, False, sigma, 0.0)
    n_active = int(active.sum())
    rvec = RR.so3_log(R)
    finite = bool(np.all(np.isfinite(R)) and np.all(np.isfinite(t)) and np.all(np.isfinite(info)) and np.all(np.isfinite(rvec))
                  and np.isfinite(cost_first[0]) and np.isfinite(cost[0]))
    applied = n_active >= min_inliers and chol_ok(info) and finite
    out = {"status": APPLIED if applied else KEPT_PNP, "n_points": n, "n_active": n_active, "active": active.astype(np.uint8),
           "iters": total, "views": len(obs) - 2, "info": info, "cost_first": cost_first[0], "cost_last": cost[0], "log": log,
           "R_ref": R, "t_ref": t, "rvec_ref": rvec, "X_ref": X}
    if applied:
        out.update(R=R, t=t, rvec=rvec, X=X)
    else:
        R0 = np.asarray(R0, np.float64).reshape(3, 3)
        out.update(R=R0.copy(), t=np.asarray(t0, np.float64).reshape(3).copy(), rvec=RR.so3_log(R0), X=Xs)
    return out

