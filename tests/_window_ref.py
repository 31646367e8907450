"""numpy twins of the sliding window (csrc/window.hip).  update(): the landmark table's update (svo_window_update), rules T2-T7 of
include/svo_abi.h on plain arrays, one track at a time; the HIP kernel equals it bit for bit in counts, ids, masks and
observations, and to 1e-12 relative in poses and X (both do the same double operations in the same order).  solve(): the
optimiser over a table (svo_window_ba), rules W1-W8, in float64 with the helpers of tests/_refine_ref.py."""
import math

import numpy as np

import _refine_ref as RR
from _pose_ref import inv_t4

MAX_FRAMES = 8          # SVO_WINDOW_MAX_FRAMES: the fixed stride of a row's observation columns


def empty(cap=0):
    """A cleared table (T1) with room for `cap` rows."""
    return dict(n=0, m=0, poses=np.zeros((MAX_FRAMES, 12)), ids=np.zeros(cap, np.int64), X=np.zeros((cap, 3)),
                seen=np.zeros(cap, np.uint32), active=np.zeros(cap, np.uint32),
                obs_left=np.zeros((cap, MAX_FRAMES, 2), np.float32), obs_right=np.zeros((cap, MAX_FRAMES, 2), np.float32))


def camera_from_world(pose):
    """(R, t) of Y = R X + t from a world-from-camera 4 x 4 chain pose: R = Rw^T, t = -(Rw^T tw), summed left to right."""
    M = inv_t4(pose)                                                # rule T4, the same expression as the keyframe's inv_K
    return M[:3, :3].copy(), M[:3, 3].copy()


def usable_tracks(t1_left, t1_right, t2_left, t2_right, tri):
    """T5: the four observations and the float32 triangulated point are finite."""
    o = [np.asarray(a, np.float32).reshape(-1, 2) for a in (t1_left, t1_right, t2_left, t2_right)]
    ok = np.isfinite(np.asarray(tri, np.float32).reshape(-1, 3)).all(1)
    for a in o:
        ok &= np.isfinite(a).all(1)
    return ok


class Overflow(Exception):
    """T7: the updated table needs more rows than `cap`; args[0] is the number it needs."""


def update(tab, frames, t1_left, t1_right, t2_left, t2_right, ids, tri, pose_a, pose_b, cap=None):
    """One step with ok = 1 on pair a -> b.  tab: dict as empty() makes it (not modified); frames: W; pose_a: frame_pose_
    before the step, pose_b: the record's pose (4 x 4, world from camera).  Returns the new table with `cap` rows of room
    (default: as many as it needs); raises Overflow when it needs more."""
    W = int(frames)
    assert 2 <= W <= MAX_FRAMES
    n, m = int(tab["n"]), int(tab["m"])
    poses = np.array(tab["poses"], np.float64).reshape(MAX_FRAMES, 12).copy()
    rows = [dict(id=int(tab["ids"][r]), X=np.array(tab["X"][r], np.float64), seen=int(tab["seen"][r]), active=int(tab["active"][r]),
                 L=np.array(tab["obs_left"][r], np.float32), R=np.array(tab["obs_right"][r], np.float32)) for r in range(m)]
    if n == 0:                                                    # T2: slot 0 is frame a
        rows = []
        Ra, ta = camera_from_world(pose_a)
        poses[:] = 0
        poses[0, :9], poses[0, 9:] = Ra.ravel(), ta
        n = 1
    elif n == W:                                                  # T3: slide
        poses[:-1] = poses[1:].copy()
        poses[-1] = 0
        kept = []
        for r in rows:
            r["seen"] >>= 1
            r["active"] >>= 1
            for k in ("L", "R"):
                r[k][:-1] = r[k][1:].copy()
                r[k][-1] = 0
            if r["seen"]:
                kept.append(r)
        rows = kept
        n = W - 1
    Rb, tb = camera_from_world(pose_b)                            # T4: frame b is the newest slot
    poses[n, :9], poses[n, 9:] = Rb.ravel(), tb
    poses[n + 1:] = 0
    prev, new = n - 1, n
    n += 1
    Ra, ta = poses[prev, :9].reshape(3, 3), poses[prev, 9:]
    t1l, t1r, t2l, t2r = (np.asarray(a, np.float32).reshape(-1, 2) for a in (t1_left, t1_right, t2_left, t2_right))
    tri = np.asarray(tri, np.float32).reshape(-1, 3)
    ids = np.asarray(ids, np.int64).reshape(-1)
    ok = usable_tracks(t1l, t1r, t2l, t2r, tri)
    by_id = {r["id"]: r for r in rows}
    for k in np.nonzero(ok)[0]:                                   # T5 / T6
        r = by_id.get(int(ids[k]))
        if r is None:
            d = tri[k].astype(np.float64) - ta
            X = np.array([(Ra[0, j] * d[0] + Ra[1, j] * d[1]) + Ra[2, j] * d[2] for j in range(3)])
            r = dict(id=int(ids[k]), X=X, seen=0, active=0, L=np.zeros((MAX_FRAMES, 2), np.float32), R=np.zeros((MAX_FRAMES, 2), np.float32))
            by_id[r["id"]] = r
        if not r["seen"] >> prev & 1:
            r["L"][prev], r["R"][prev] = t1l[k], t1r[k]
        r["L"][new], r["R"][new] = t2l[k], t2r[k]
        r["seen"] |= 1 << prev | 1 << new
    rows = [by_id[i] for i in sorted(by_id)]
    m = len(rows)
    cap = m if cap is None else int(cap)
    if m > cap:
        raise Overflow(m)
    out = empty(cap)
    out["n"], out["m"], out["poses"] = n, m, poses
    for i, r in enumerate(rows):
        out["ids"][i], out["X"][i], out["seen"][i], out["active"][i] = r["id"], r["X"], r["seen"], r["active"]
        out["obs_left"][i], out["obs_right"][i] = r["L"], r["R"]
    return out


def check_invariants(tab):
    """What every table obeys: ids strictly ascending, masks inside the n slots, no empty row, active within seen."""
    n, m = tab["n"], tab["m"]
    ids, seen, active = tab["ids"][:m], tab["seen"][:m], tab["active"][:m]
    assert (np.diff(ids) > 0).all()
    assert (seen != 0).all() and (seen >> np.uint32(n) == 0).all() and (active & ~seen == 0).all()
    assert (tab["poses"][n:] == 0).all()


# ---- the optimiser over a table (svo_window_ba, csrc/window.hip: window_ba_kernel): rules W1-W8 of include/svo_abi.h ------------
TAU = 9.488                      # chi-square 95 % point, 4 degrees of freedom: one stereo observation (W2)
BA_MAX_DIM = 6 * (MAX_FRAMES - 1)
APPLIED, KEPT, SKIPPED = RR.APPLIED, RR.KEPT_PNP, RR.SKIPPED


def slot_masks(mask, n):
    """(m, n) bool of a uint32 mask column."""
    return (np.asarray(mask, np.uint32)[:, None] >> np.arange(n, dtype=np.uint32) & np.uint32(1)).astype(bool)


def ba_evaluate(X, R, t, obs_left, obs_right, views, sigma):
    """Every (landmark, slot): projectable (m, n), r (m, n, 4), c (m, n), A = d pixel / dY (m, n, 4, 3), Y (m, n, 3)."""
    m, n = X.shape[0], R.shape[0]
    proj, r, A, Ys = np.ones((m, n), bool), np.zeros((m, n, 4)), np.zeros((m, n, 4, 3)), np.zeros((m, n, 3))
    for f in range(n):
        Y = RR.rows_times(X, R[f]) + t[f]
        Ys[:, f] = Y
        for v, (M, p4) in enumerate(views):
            o = (obs_left, obs_right)[v][:, f].astype(np.float64)
            h = RR.rows_times(Y, M) + p4
            ok = h[:, 2] > RR.MIN_DEPTH
            proj[:, f] &= ok
            h2 = np.where(ok, h[:, 2], 1.0)
            u, w = h[:, 0] / h2, h[:, 1] / h2
            r[:, f, 2 * v], r[:, f, 2 * v + 1] = u - o[:, 0], w - o[:, 1]
            A[:, f, 2 * v] = (M[0][None, :] - u[:, None] * M[2][None, :]) / h2[:, None]
            A[:, f, 2 * v + 1] = (M[1][None, :] - w[:, None] * M[2][None, :]) / h2[:, None]
    c = (r * r).sum(2) / (sigma * sigma)
    return proj, r, c, A, Ys


def _ba_cost(rho, act):
    terms = [float(v) for v in rho[act]]
    hi = math.fsum(terms)
    return (hi, math.fsum(terms + [-hi]) if math.isfinite(hi) else 0.0)


def _ba_weights(c, act, robust):
    w, rho = np.ones_like(c), c.copy()
    if robust:
        big = c > TAU
        cs = np.where(big, c, 1.0)
        w = np.where(big, np.sqrt(TAU / cs), 1.0)
        rho = np.where(big, 2.0 * np.sqrt(TAU * cs) - TAU, c)
    return np.where(act, w, 0.0), rho


def ba_build(ev, R, act, robust, sigma, lam):
    """The reduced system over the active observations at damping lam (W5).  Returns the cost pair, H (D, D), g (D), the
    diagonal of sum U (D), D = 6 (n - 1), and per landmark (ok, L (m, 6), T (m, n - 1, 6, 3), y (m, 3))."""
    proj, r, c, A, Y = ev
    m, n = c.shape
    w, rho = _ba_weights(c, act, robust)
    ws = w / (sigma * sigma)
    Jx = np.stack([np.stack([RR.rows_times(A[:, f, k], R[f].T) for k in range(4)], 1) for f in range(n)], 1)       # a^T R_f
    Jx, rr = np.where(act[:, :, None, None], Jx, 0.0), np.where(act[:, :, None], r, 0.0)
    V = (ws[:, :, None, None] * (Jx[:, :, :, :, None] * Jx[:, :, :, None, :]).sum(2)).sum(1)
    gx = (ws[:, :, None] * (Jx * rr[:, :, :, None]).sum(2)).sum(1)
    D = 6 * (n - 1)
    Wm, U, gp = np.zeros((m, n - 1, 6, 3)), np.zeros((m, n - 1, 6, 6)), np.zeros((m, n - 1, 6))
    for f in range(1, n):
        Jp = np.zeros((m, 4, 6))
        for k in range(4):
            Jp[:, k, :3], Jp[:, k, 3:] = A[:, f, k], np.cross(Y[:, f], A[:, f, k])                               # -a^T [Y]x
        Jp = np.where(act[:, f, None, None], Jp, 0.0)
        Wm[:, f - 1] = ws[:, f, None, None] * (Jp[:, :, :, None] * Jx[:, f, :, None, :]).sum(1)
        U[:, f - 1] = ws[:, f, None, None] * (Jp[:, :, :, None] * Jp[:, :, None, :]).sum(1)
        gp[:, f - 1] = ws[:, f, None] * (Jp * rr[:, f, :, None]).sum(1)
    any_act = act.any(1)
    d0 = V[:, 0, 0] + lam * V[:, 0, 0]
    ok = any_act & (d0 > 0.0)
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
    T = np.zeros_like(Wm)
    T[..., 0] = Wm[..., 0] / l00[:, None, None]
    T[..., 1] = (Wm[..., 1] - l10[:, None, None] * T[..., 0]) / l11[:, None, None]
    T[..., 2] = ((Wm[..., 2] - l20[:, None, None] * T[..., 0]) - l21[:, None, None] * T[..., 1]) / l22[:, None, None]
    y = np.zeros_like(gx)
    y[:, 0] = gx[:, 0] / l00
    y[:, 1] = (gx[:, 1] - l10 * y[:, 0]) / l11
    y[:, 2] = ((gx[:, 2] - l20 * y[:, 0]) - l21 * y[:, 1]) / l22
    T[~ok] = 0.0
    y[~ok] = 0.0
    H, g, dU = np.zeros((D, D)), np.zeros(D), np.zeros(D)
    for f in range(n - 1):
        sl = slice(6 * f, 6 * f + 6)
        Us = U[any_act, f].sum(0)
        dU[sl] = np.diagonal(Us)
        g[sl] = (gp[any_act, f] - (T[any_act, f] * y[any_act, None, :]).sum(2)).sum(0)
        for e in range(n - 1):
            TT = (T[any_act, f][:, :, None, :] * T[any_act, e][:, None, :, :]).sum(3).sum(0)
            H[sl, 6 * e:6 * e + 6] = (Us if e == f else 0.0) - TT
    L = np.stack([l00, l10, l11, l20, l21, l22], 1)
    return _ba_cost(rho, act), H, g, dU, (ok, L, T, y)


def chol_solve(A, b):
    """Cholesky solve of any size, row by row; fails unless every pivot is > 0."""
    n = len(b)
    L = np.zeros((n, n))
    for i in range(n):
        for j in range(i + 1):
            s = A[i, j] - float(np.dot(L[i, :j], L[j, :j]))
            if i == j:
                if not s > 0.0:
                    return False, None
                L[i, i] = math.sqrt(s)
            else:
                L[i, j] = s / L[j, j]
    y = np.zeros(n)
    for i in range(n):
        y[i] = (b[i] - float(np.dot(L[i, :i], y[:i]))) / L[i, i]
    x = np.zeros(n)
    for i in range(n - 1, -1, -1):
        x[i] = (y[i] - float(np.dot(L[i + 1:, i], x[i + 1:]))) / L[i, i]
    return True, x


def ba_back_substitute(pts, xi):
    """dX_i = -L^-T (y_i + sum_f T_if^T xi_f); 0 for the landmarks that are not moved."""
    ok, L, T, y = pts
    z = y + (T * xi.reshape(1, -1, 6, 1)).sum((1, 2))
    l00, l10, l11, l20, l21, l22 = (L[:, k] for k in range(6))
    e2 = z[:, 2] / l22
    e1 = (z[:, 1] - l21 * e2) / l11
    e0 = ((z[:, 0] - l10 * e1) - l20 * e2) / l00
    dX = -np.stack([e0, e1, e2], 1)
    dX[~ok] = 0.0
    return dX


def solve(tab, P1, P2, rounds=4, iters=5, sigma=1.0, min_obs=10):
    """The optimiser on a table (not modified).  Returns dict(status, n_frames, n_landmarks, n_usable, n_obs, n_active, iters,
    frame_active (8), cost_first, cost_last, info (42, 42), poses (8, 12), X (m, 3), active (m) -- the table's columns as they
    stand afterwards -- and log: per round its exit, the smallest |c - tau| / tau at its re-classification and the smallest
    relative cost difference over its accept decisions, and `steps`: per LM iteration accepted / rejected (by the cost) /
    unprojectable / singular (the factorisation failed))."""
    n, m = int(tab["n"]), int(tab["m"])
    poses0 = np.array(tab["poses"], np.float64).reshape(MAX_FRAMES, 12)
    X0 = np.array(tab["X"][:m], np.float64).reshape(m, 3)
    out = dict(status=SKIPPED, n_frames=n, n_landmarks=m, n_usable=0, n_obs=0, n_active=0, iters=0, frame_active=np.zeros(MAX_FRAMES, np.int32),
               cost_first=0.0, cost_last=0.0, info=np.zeros((BA_MAX_DIM, BA_MAX_DIM)), poses=poses0.copy(), X=X0.copy(),
               active=np.array(tab["active"][:m], np.uint32), log=[])
    if n < 2:
        return out
    P1, P2 = np.asarray(P1, np.float64).reshape(3, 4), np.asarray(P2, np.float64).reshape(3, 4)
    views = [(np.array([[P1[0, 0], 0.0, P1[0, 2]], [0.0, P1[1, 1], P1[1, 2]], [0.0, 0.0, 1.0]]), np.zeros(3)), (P2[:, :3].copy(), P2[:, 3].copy())]
    R, t = poses0[:n, :9].reshape(n, 3, 3).copy(), poses0[:n, 9:].copy()
    oL, oR = np.asarray(tab["obs_left"][:m], np.float32), np.asarray(tab["obs_right"][:m], np.float32)
    seen = slot_masks(tab["seen"][:m], n)
    X = X0.copy()
    D = 6 * (n - 1)

    def settle(act, X):
        usable = act.sum(1) >= 2                                   # W3; a landmark below two returns to its X at entry (W4)
        return act & usable[:, None], np.where(usable[:, None], X, X0)

    ev = ba_evaluate(X, R, t, oL, oR, views, sigma)
    act, X = settle(seen & ev[0], X)
    ev = ba_evaluate(X, R, t, oL, oR, views, sigma)
    total, cost_first, cost = 0, (0.0, 0.0), (0.0, 0.0)
    for rd in range(rounds):
        robust = rd < 2
        lam, how, acc_margin, steps = 1e-4, "iters", np.inf, []
        for it in range(iters):
            total += 1
            cost_b, H, g, dU, pts = ba_build(ev, R, act, robust, sigma, lam)
            if it == 0:
                cost = cost_b
                if rd == 0:
                    cost_first = cost
            ok, xi = chol_solve(H + lam * np.diag(dU), -g)
            accepted, what = False, "singular"
            if ok:
                what = "unprojectable"
                dX = ba_back_substitute(pts, xi)
                Rn, tn = R.copy(), t.copy()
                for f in range(1, n):
                    E, Vr = RR.se3_exp(xi[6 * f - 6:6 * f])
                    Rn[f], tn[f] = RR.mm(E, R[f]), RR.mm(E, t[f]) + Vr
                Xn = X + dX
                evn = ba_evaluate(Xn, Rn, tn, oL, oR, views, sigma)
                if np.all(evn[0][act]):
                    costn = _ba_cost(_ba_weights(evn[2], act, robust)[1], act)
                    accepted = costn < cost
                    what = "accepted" if accepted else "rejected"
                    if cost[0] > 0.0:
                        acc_margin = min(acc_margin, abs((cost[0] - costn[0]) + (cost[1] - costn[1])) / cost[0])
            steps.append(what)
            if accepted:
                R, t, X, ev, cost = Rn, tn, Xn, evn, costn
                lam = max(lam / 10.0, 1e-12)
                step = math.sqrt(float((dX * dX).sum(1).max())) if m else 0.0
                if math.sqrt(float((xi * xi).sum())) < 1e-10 and step < 1e-9:
                    how = "xi"
                    break
            else:
                lam *= 10.0
                if lam > 1e10:
                    how = "lambda"
                    break
        proj, _, c, _, _ = ev
        cand = seen & proj
        with np.errstate(invalid="ignore"):
            act, X = settle(cand & (c <= TAU), X)
        cc = c[cand][~np.isnan(c[cand])]
        near = float(np.min(np.abs(cc - TAU))) / TAU if len(cc) else np.inf
        ev = ba_evaluate(X, R, t, oL, oR, views, sigma)
        out["log"].append({"exit": how, "margin": near, "accept_margin": acc_margin, "steps": steps})
    _, info, _, _, _ = ba_build(ev, R, act, False, sigma, 0.0)
    fa = act.sum(0)
    finite = bool(np.isfinite(R).all() and np.isfinite(t).all() and np.isfinite(X).all() and np.isfinite(info).all()
                  and np.isfinite(cost_first[0]) and np.isfinite(cost[0]))
    applied = bool((fa[1:] >= min_obs).all()) and chol_solve(info, np.zeros(D))[0] and finite
    out["frame_active"][:n] = fa
    out["info"][:D, :D] = info
    out.update(status=APPLIED if applied else KEPT, n_usable=int(act.any(1).sum()), n_obs=int(seen.sum()), n_active=int(act.sum()),
               iters=total, cost_first=cost_first[0], cost_last=cost[0], ref=dict(R=R, t=t, X=X, act=act))
    if applied:
        out["poses"][:n, :9], out["poses"][:n, 9:] = R.reshape(n, 9), t
        out["X"] = X
        out["active"] = (act.astype(np.uint32) << np.arange(n, dtype=np.uint32)).sum(1).astype(np.uint32)
    return out
