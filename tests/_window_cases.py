"""Inputs shared by test_window_ref.py (CPU) and test_gpu_window.py: synthetic chains of tracked pairs for the sliding window's
landmark table.  A chain is a list of steps (tracks, ids, triangulation, pose_a, pose_b); tracks are born under ever larger
ids, die at random, and are unusable now and then (a non-finite observation or triangulated point), which makes the holes, the
late rows (T6) and the rows that drop out at a slide (T3).  t1 of a pair is drawn independently of the t2 before it, so a row
that already holds the older slot's observation shows whether T5's "unless set" is obeyed."""
import numpy as np

import _window_ref as WR

T = 1024                 # lanes of window_update_kernel's one workgroup


def rand_pose(rng, scale=1.0):
    """A world-from-camera 4 x 4: a proper rotation (QR of a random matrix) and a translation."""
    q, r = np.linalg.qr(rng.standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    P = np.eye(4)
    P[:3, :3], P[:3, 3] = q, rng.standard_normal(3) * scale
    return P


def make_pair(rng, ids, bad_rate=0.0):
    """Tracks for the given ascending ids; a share of them unusable, each through one of its 11 floats (NaN or +-inf)."""
    n = len(ids)
    p = dict(ids=np.asarray(ids, np.int64), tri=(rng.standard_normal((n, 3)) * 5 + [0, 0, 20]).astype(np.float32))
    for k in ("t1_left", "t1_right", "t2_left", "t2_right"):
        p[k] = (rng.random((n, 2)) * [416, 128]).astype(np.float32)
    for i in np.nonzero(rng.random(n) < bad_rate)[0]:
        f = int(rng.integers(0, 11))
        v = np.float32([np.nan, np.inf, -np.inf][int(rng.integers(0, 3))])
        if f < 8:
            p[("t1_left", "t1_right", "t2_left", "t2_right")[f // 2]][i, f % 2] = v
        else:
            p["tri"][i, f - 8] = v
    return p


def chain(seed, steps, n0, births, death_rate=0.15, bad_rate=0.05, id0=0, id_step=3):
    """`steps` pairs: n0 tracks at first, `births` more per pair, each dying with death_rate per pair."""
    rng = np.random.default_rng(seed)
    live, nxt, out = [], id0, []
    pose = rand_pose(rng)
    for s in range(steps):
        live = [i for i in live if rng.random() >= death_rate]
        for _ in range(n0 if s == 0 else births):
            nxt += int(rng.integers(1, id_step + 1))
            live.append(nxt)
        nxt_pose = rand_pose(rng)
        out.append(dict(pair=make_pair(rng, live, bad_rate), pose_a=pose, pose_b=nxt_pose))
        pose = nxt_pose
    return out


def apply(tab, frames, step, cap=None):
    p = step["pair"]
    return WR.update(tab, frames, p["t1_left"], p["t1_right"], p["t2_left"], p["t2_right"], p["ids"], p["tri"], step["pose_a"],
                     step["pose_b"], cap)


def table_after(steps, frames, k):
    """The twin's table after the first k steps of a chain, from a cleared one."""
    tab = WR.empty()
    for s in steps[:k]:
        tab = apply(tab, frames, s)
    return tab


def _sized(seed, frames, rows, tracks):
    """A full window (n = W) of exactly `rows` rows with a pair of `tracks` tracks to add; half of the tracks join rows."""
    rng = np.random.default_rng(seed)
    ids = np.cumsum(rng.integers(1, 4, rows)).astype(np.int64) + (1 << 33)            # ids beyond 32 bits
    tab = WR.empty(rows)
    tab["n"], tab["m"], tab["ids"] = frames, rows, ids
    tab["poses"][:frames] = [np.concatenate([WR.camera_from_world(rand_pose(rng))[0].ravel(), rng.standard_normal(3)]) for _ in range(frames)]
    tab["X"][:] = rng.standard_normal((rows, 3))
    tab["seen"][:] = rng.integers(1, 1 << frames, rows)                             # a third of seen == 1 rows leave at the slide
    tab["seen"][::3] = 1
    tab["active"][:] = tab["seen"] & rng.integers(0, 1 << frames, rows).astype(np.uint32)
    for k in ("obs_left", "obs_right"):
        tab[k][:] = (rng.random((rows, WR.MAX_FRAMES, 2)) * 400).astype(np.float32)
        tab[k][(tab["seen"][:, None] >> np.arange(WR.MAX_FRAMES, dtype=np.uint32) & 1) == 0] = 0
    old = rng.choice(ids, min(tracks // 2, rows), replace=False)
    fresh = np.setdiff1d(rng.integers(ids[0] - 50, ids[-1] + 50 + 4 * tracks, 8 * tracks + 8), ids)
    tid = np.sort(np.concatenate([old, rng.choice(fresh, tracks - len(old), replace=False)]))
    step = dict(pair=make_pair(rng, tid, 0.05), pose_a=rand_pose(rng), pose_b=rand_pose(rng))
    return tab, frames, step, None


# name: () -> (table in, frames, step, cap (None: exactly what the result needs))
def _from_chain(seed, frames, k, **kw):
    steps = chain(seed, k + 1, **kw)
    return table_after(steps, frames, k), frames, steps[k], None


def _no_tracks(case):
    return case[0], case[1], dict(case[2], pair=make_pair(np.random.default_rng(9), [])), None


def _all_bad(case):
    return case[0], case[1], dict(case[2], pair=make_pair(np.random.default_rng(10), case[2]["pair"]["ids"], 1.0)), None


UPDATE_CASES = {
    "empty_table": lambda: _from_chain(1, 4, 0, n0=300, births=60),
    "empty_table_no_tracks": lambda: (WR.empty(), 3, dict(pair=make_pair(np.random.default_rng(2), []), pose_a=np.eye(4), pose_b=rand_pose(np.random.default_rng(2))), 1),
    "second_pair_w4": lambda: _from_chain(3, 4, 1, n0=300, births=60),
    "last_before_slide_w4": lambda: _from_chain(4, 4, 2, n0=300, births=60),
    "first_slide_w4": lambda: _from_chain(5, 4, 3, n0=300, births=60, death_rate=0.3),      # nothing drops yet: every row has two slots
    "slide_w4": lambda: _from_chain(5, 4, 4, n0=300, births=60, death_rate=0.3),
    "slide_again_w4": lambda: _from_chain(5, 4, 6, n0=300, births=60, death_rate=0.3),
    "slide_w2": lambda: _from_chain(6, 2, 3, n0=200, births=80, death_rate=0.3),
    "slide_w3_many_bad": lambda: _from_chain(7, 3, 5, n0=300, births=60, bad_rate=0.4),
    "slide_w8": lambda: _from_chain(8, 8, 9, n0=300, births=40),
    "no_tracks_slide": lambda: _no_tracks(_from_chain(9, 3, 4, n0=200, births=50)),
    "all_tracks_bad": lambda: _all_bad(_from_chain(10, 3, 4, n0=200, births=50)),
    "big_ids": lambda: _from_chain(11, 4, 5, n0=300, births=60, id0=(1 << 40), id_step=1 << 20),
}
for _rows, _trk in ((T - 1, 64), (T, 65), (T + 1, 63), (2 * T + 1, T + 1), (63, T - 1), (64, T), (65, 2 * T + 1)):
    UPDATE_CASES["rows_%d_tracks_%d" % (_rows, _trk)] = lambda r=_rows, t=_trk: _sized(100 + r, 5, r, t)


def late_row_case():
    """T6 by hand: id 20 is unusable in the first pair and usable in the second, so its row is made late, between ids 10 and 30."""
    rng = np.random.default_rng(12)
    p0, p1 = make_pair(rng, [10, 20, 30]), make_pair(rng, [10, 20, 30, 40])
    p0["tri"][1, 2] = np.nan
    poses = [rand_pose(rng) for _ in range(3)]
    return [dict(pair=p0, pose_a=poses[0], pose_b=poses[1]), dict(pair=p1, pose_a=poses[1], pose_b=poses[2])]


# ---- tables for the optimiser (svo_window_ba): a camera moving through a cloud of landmarks -------------------------------------
P1 = np.array([[300.0, 0, 208.0, 0], [0, 300.0, 64.0, 0], [0, 0, 1, 0]])
P2 = np.array([[300.0, 0, 208.0, -162.0], [0, 300.0, 64.0, 0], [0, 0, 1, 0]])          # a 0.54 m baseline


def _rot(v):
    th = np.linalg.norm(v)
    if th == 0:
        return np.eye(3)
    k = v / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def scene(seed, n, m, holes=False, outliers=0.0, noise=0.3, start=(0.02, 0.002), once=0, starve=None, starve_left=0, nan_obs=False):
    """A table of n frames and m landmarks.  The truth: the camera advances 0.4 m a frame with a small rotation; landmarks 4-30 m
    ahead; observations are the projections plus `noise` pixels, rounded to float32.  The table starts `start` (metres,
    radians) away from the truth in every slot but the first, its points 2 % off in depth.  holes: seen masks with gaps,
    otherwise contiguous runs; outliers: that share of the observations is 8-40 px off; once: that many landmarks are seen in
    one slot only; starve = f: slot f keeps only `starve_left` observations; nan_obs: one observation is NaN."""
    rng = np.random.default_rng(seed)
    tab = WR.empty(m)
    tab["n"], tab["m"] = n, m
    tab["ids"][:] = np.cumsum(rng.integers(1, 4, m))
    Xw = np.stack([rng.uniform(-6, 6, m), rng.uniform(-2, 2, m), rng.uniform(4 + 0.4 * n, 30, m)], 1)
    Rt = []
    for f in range(n):
        Rf = _rot(np.array([0.002, 0.01, -0.003]) * f)
        Rt.append((Rf, -Rf @ np.array([0.02 * f, 0.0, 0.4 * f])))
    seen = np.zeros((m, n), bool)
    for i in range(m):
        a = int(rng.integers(0, n - 1))
        b = int(rng.integers(a + 2, n + 1))
        seen[i, a:b] = True
        if holes and b - a >= 3 and rng.random() < 0.5:
            seen[i, int(rng.integers(a + 1, b - 1))] = False
    for i in range(once):
        seen[i] = False
        seen[i, int(rng.integers(0, n))] = True
    if starve is not None:
        keep = rng.permutation(np.nonzero(seen[:, starve])[0])[:starve_left]
        seen[:, starve] = False
        seen[keep, starve] = True
        seen[seen.sum(1) == 0, 0] = True
    for f, (Rf, tf) in enumerate(Rt):
        Y = Xw @ Rf.T + tf
        for name, P in (("obs_left", P1), ("obs_right", P2)):
            h = Y @ P[:, :3].T + P[:, 3]
            px = h[:, :2] / h[:, 2:] + rng.standard_normal((m, 2)) * noise
            bad = rng.random(m) < outliers
            px[bad] += rng.uniform(8, 40, (int(bad.sum()), 2)) * rng.choice([-1, 1], (int(bad.sum()), 2))
            tab[name][:, f] = np.where(seen[:, f, None], px, 0).astype(np.float32)
        dr, dt = (rng.standard_normal(3) * start[1], rng.standard_normal(3) * start[0]) if f else (np.zeros(3), np.zeros(3))
        Rs = _rot(dr) @ Rf
        tab["poses"][f, :9], tab["poses"][f, 9:] = Rs.ravel(), tf + dt
    tab["seen"][:] = (seen.astype(np.uint32) << np.arange(n, dtype=np.uint32)).sum(1)
    tab["X"][:] = Xw * (1 + rng.standard_normal((m, 1)) * 0.02)
    if nan_obs:
        i = int(np.nonzero(seen[:, 1])[0][3])
        tab["obs_right"][i, 1, 0] = np.nan
    return tab, dict(Xw=Xw, Rt=Rt)


# name: scene arguments.  Every case has 30 % outlier observations, so that every round still has work to do and no accept
# decision falls near a tie; the seeds are the first ones whose margins test_window_ref.py accepts.  Landmark counts sit
# around the kernel's workgroup size T and around one wave.
BA_SETTINGS = dict(rounds=4, iters=2, sigma=1.0, min_obs=10)
BA_CASES = {
    "n2_Tm1": dict(seed=16, n=2, m=T - 1, outliers=0.3),
    "n3_T_holes": dict(seed=18, n=3, m=T, holes=True, outliers=0.3),
    "n5_Tp1_holes_once": dict(seed=1, n=5, m=T + 1, holes=True, once=5, outliers=0.3),
    "n8_2Tp1_holes": dict(seed=1, n=8, m=2 * T + 1, holes=True, outliers=0.3),
    "n3_63": dict(seed=2, n=3, m=63, outliers=0.3),
    "n4_64_holes": dict(seed=9, n=4, m=64, holes=True, outliers=0.3),
    "n5_65_kept": dict(seed=2, n=5, m=65, outliers=0.3),                                   # slot 0 .. 4 thin: a slot below min_obs
    "slot_below_min_obs": dict(seed=1, n=4, m=300, starve=2, starve_left=4, outliers=0.3),
    "slot_without_observations": dict(seed=1, n=4, m=300, starve=2, starve_left=0, outliers=0.3),
    "nan_observation": dict(seed=15, n=3, m=300, nan_obs=True, outliers=0.3),
    "far_start": dict(seed=3, n=3, m=300, start=(3.0, 0.3), outliers=0.3),
    "far_start_all_cut": dict(seed=1, n=3, m=300, start=(1.0, 0.1), outliers=0.3),
    # round 0: two steps refused as unprojectable, one REJECTED BY THE COST, then -- lambda three decades up -- one accepted
    "reject_then_accept": dict(seed=2, n=3, m=150, start=(1.0, 0.3), outliers=0.1, settings=dict(rounds=2, iters=6)),
}
_BA = {}


def ba_case(name):
    """(table, the twin's outcome), computed once."""
    if name not in _BA:
        tab, _ = scene(**{k: v for k, v in BA_CASES[name].items() if k != "settings"})
        _BA[name] = (tab, WR.solve(tab, P1, P2, **ba_settings(name)))
    return _BA[name]


def ba_settings(name):
    return dict(BA_SETTINGS, **BA_CASES[name].get("settings", {}))
