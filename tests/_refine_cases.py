"""Synthetic fixtures of the pose-refinement tests (CPU reference tests and GPU stage-call tests share them).

A case: float32 points X in the t1 camera frame, float32 observations at t2 in both cameras under a known motion with
0.3 px noise, a share of gross outliers, optionally points behind the camera; the start pose 10 cm and 0.1 degree off."""
import numpy as np
from scipy.spatial.transform import Rotation

import _refine_ref as RR
import _rigs

STAGE_N = (6, 63, 64, 65, 255, 256, 257, 2500)       # lane, wave and workgroup stride edges of pose_refine_kernel
KINDS = ("outliers", "some_behind", "all_behind")
SEED0 = 20240519


def true_pose():
    R = Rotation.from_rotvec((0.004, -0.011, 0.003)).as_matrix()
    return R, np.array([0.03, -0.02, -0.85])


def start_pose():
    """10 cm and 0.1 degree off the true pose."""
    R, t = true_pose()
    dR = Rotation.from_rotvec(np.deg2rad(0.1) * np.array([0.6, -0.48, 0.64])).as_matrix()
    return dR @ R, t + 0.1 * np.array([0.48, 0.6, -0.64])


def project(P, Y):
    h = Y @ P[:, :3].T + P[:, 3]
    return h[:, :2] / h[:, 2:3]


def make_case(rig, n, kind, seed=SEED0, noise=0.3, outlier_share=0.3):
    """Returns a dict with X (n, 3) f32, xl / xr (n, 2) f32, P1 / P2 (3, 4) f64, R0 / t0 / rvec0 and the index sets."""
    P1, P2 = _rigs.matrices(rig)
    rng = np.random.default_rng([seed, n, KINDS.index(kind), sorted(_rigs.RIGS).index(rig)])
    R, t = true_pose()
    K1 = np.zeros((3, 4))
    K1[:, :3] = [[P1[0, 0], 0, P1[0, 2]], [0, P1[1, 1], P1[1, 2]], [0, 0, 1]]
    # points that both cameras see at t2: pixel + depth in the left camera at t2, pulled back to t1
    u = rng.uniform(40, _rigs.W - 40, n)
    v = rng.uniform(20, _rigs.H - 20, n)
    z = rng.uniform(4.0, 40.0, n)
    Y = np.stack([(u - K1[0, 2]) / K1[0, 0] * z, (v - K1[1, 2]) / K1[1, 1] * z, z], 1)
    X = ((Y - t) @ R).astype(np.float32)                        # X = R^T (Y - t)
    behind = np.zeros(n, bool)
    if kind == "all_behind":
        behind[:] = True
    elif kind == "some_behind":
        behind[rng.permutation(n)[:max(1, n // 8)]] = True
    X[behind, 2] = -X[behind, 2] - 3.0                            # at least 1 m behind both cameras at t2
    Y = X.astype(np.float64) @ R.T + t
    Ys = np.where(behind[:, None], Y * [1, 1, -1], Y)            # any finite pixel for the points nobody sees
    xl = project(K1, Ys) + noise * rng.standard_normal((n, 2))
    xr = project(P2, Ys) + noise * rng.standard_normal((n, 2))
    outlier = np.zeros(n, bool)
    if kind != "all_behind":
        cand = np.flatnonzero(~behind)
        k = int(outlier_share * len(cand)) if n > 6 else 0          # n = 6 stays clean: min_inliers = 6 must be reachable
        outlier[rng.permutation(cand)[:k]] = True
    m = int(outlier.sum())
    ang = rng.uniform(0, 2 * np.pi, m)
    rad = rng.uniform(15.0, 80.0, m)                             # gross: 15 .. 80 px, in both views
    off = np.stack([rad * np.cos(ang), rad * np.sin(ang)], 1)
    xl[outlier] += off
    xr[outlier] -= off[:, ::-1]
    R0, t0 = start_pose()
    return dict(rig=rig, n=n, kind=kind, X=X, xl=xl.astype(np.float32), xr=xr.astype(np.float32), P1=P1, P2=P2,
                R0=R0, t0=t0, rvec0=RR.so3_log(R0), R_true=R, t_true=t, behind=behind, outlier=outlier)


# The settings the fixtures are run with: the defaults, but 20 iterations per round -- from 10 cm off, the Huber rounds (IRLS
# converges linearly) rarely get down to |xi| < 1e-10 within 10.
ROUNDS, ITERS = 4, 20

# fixture_ok (tests/test_refine_ref.py) asks that every round of the reference's run ends through the |xi| < 1e-10 exit, i.e.
# that the last accepted step of each round is that short.  Whether such a step still DEcreases the cost is decided by the
# rounding of a sum, so it holds for about one seed in seven; SEED_OFFSET lists, per case, the first offset from SEED0 for
# which it does (found by find_seed_offsets() below; "pick another seed, do not loosen the bar").
SEED_OFFSET = {('R0', 6, 'outliers', 2): 4,
 ('R0', 6, 'outliers', 4): 5,
 ('R0', 6, 'some_behind', 2): 1,
 ('R0', 6, 'some_behind', 4): 20,
 ('R0', 63, 'outliers', 4): 1,
 ('R0', 63, 'some_behind', 2): 10,
 ('R0', 64, 'outliers', 2): 1,
 ('R0', 64, 'outliers', 4): 3,
 ('R0', 64, 'some_behind', 2): 2,
 ('R0', 64, 'some_behind', 4): 4,
 ('R0', 65, 'some_behind', 2): 11,
 ('R0', 65, 'some_behind', 4): 10,
 ('R0', 255, 'outliers', 4): 1,
 ('R0', 255, 'some_behind', 2): 1,
 ('R0', 256, 'outliers', 2): 8,
 ('R0', 256, 'outliers', 4): 2,
 ('R0', 256, 'some_behind', 2): 2,
 ('R0', 256, 'some_behind', 4): 3,
 ('R0', 257, 'outliers', 2): 11,
 ('R0', 257, 'outliers', 4): 1,
 ('R0', 257, 'some_behind', 2): 9,
 ('R0', 257, 'some_behind', 4): 1,
 ('R0', 2500, 'outliers', 2): 1,
 ('R0', 2500, 'outliers', 4): 5,
 ('R0', 2500, 'some_behind', 2): 1,
 ('R0', 2500, 'some_behind', 4): 1,
 ('R3', 6, 'outliers', 2): 9,
 ('R3', 6, 'outliers', 4): 16,
 ('R3', 6, 'some_behind', 2): 2,
 ('R3', 6, 'some_behind', 4): 9,
 ('R3', 63, 'outliers', 2): 1,
 ('R3', 63, 'some_behind', 4): 1,
 ('R3', 64, 'outliers', 2): 2,
 ('R3', 64, 'outliers', 4): 3,
 ('R3', 64, 'some_behind', 2): 25,
 ('R3', 64, 'some_behind', 4): 1,
 ('R3', 65, 'outliers', 2): 4,
 ('R3', 65, 'outliers', 4): 1,
 ('R3', 255, 'outliers', 2): 4,
 ('R3', 255, 'some_behind', 2): 1,
 ('R3', 255, 'some_behind', 4): 1,
 ('R3', 256, 'some_behind', 2): 2,
 ('R3', 257, 'outliers', 2): 1,
 ('R3', 257, 'some_behind', 2): 2,
 ('R3', 257, 'some_behind', 4): 5,
 ('R3', 2500, 'some_behind', 2): 2}


def case_seed(rig, n, kind, d):
    return SEED0 + SEED_OFFSET.get((rig, n, kind, d), 0)


_CACHE = {}


def ref_run(rig, n, kind, d, seed=None):
    """The reference's run of a case, computed once per session and shared (start pose as the stage call forms it: Rodrigues
    of rvec0)."""
    key = (rig, n, kind, d, seed)
    if key not in _CACHE:
        c = make_case(rig, n, kind, case_seed(rig, n, kind, d) if seed is None else seed)
        run = RR.refine(c["X"], c["xl"], c["xr"] if d == 4 else None, c["P1"], c["P2"], RR.rodrigues(c["rvec0"]), c["t0"],
                        rounds=ROUNDS, iters=ITERS)
        _CACHE[key] = (c, run)
    return _CACHE[key]


def find_seed_offsets(ok, limit=400):
    """Maintenance helper: the SEED_OFFSET table for the predicate `ok` (fixture_ok)."""
    table = {}
    for case in stage_cases():
        if case[2] == "all_behind":
            continue
        for off in range(limit):
            _, run = ref_run(*case, seed=SEED0 + off)
            if ok(run):
                if off:
                    table[case] = off
                break
        else:
            raise RuntimeError(f"no seed for {case}")
    return table


def self_spread(X, xl, xr, P1, P2, R0, t0, run, starts=(1e-15, 1e-13, 1e-11, 1e-9), per=2, seed=1, **kw):
    """How far the reference's own outcomes lie apart on a fixture: it is started `per` times at each distance of `starts` from
    t0 (same settings **kw); the largest |t| / |rvec| difference to `run`, inf where the flags or the status differ.  Where
    the accept test of R6 meets a step whose cost decrease is at the rounding of the terms (u - x cancels at ~1e2 px: a step of
    ~1e-9 at 416x128) the outcomes part by up to ~1e-9; a comparison at 1e-9 says something only on fixtures where they do not."""
    rng, spread = np.random.default_rng(seed), 0.0
    for eps in starts:
        for _ in range(per):
            r = RR.refine(X, xl, xr, P1, P2, R0, np.asarray(t0, np.float64) + eps * rng.standard_normal(3), **kw)
            if not (np.array_equal(r["active"], run["active"]) and r["status"] == run["status"]):
                return np.inf
            spread = max(spread, np.abs(r["t"] - run["t"]).max(), np.abs(r["rvec"] - run["rvec"]).max())
    return spread


# Stage-call cases at the DEFAULT settings (4 rounds x 10 iterations), where fixture_ok cannot hold (the Huber rounds do not get to
# |xi| < 1e-10 within 10 iterations from 10 cm off): what is asked of them instead is that the reference reproduces itself to a
# tenth of the comparison bar (self_spread <= 1e-10) and that no flag hangs on the last bits.  Seed offsets as above.
DEFAULT_CASES = [(rig, n, "outliers", d) for rig in ("R0", "R3") for d in (2, 4) for n in (65, 2500)]
DEFAULT_SEED_OFFSET = {('R0', 65, 'outliers', 2): 2, ('R3', 65, 'outliers', 2): 3, ('R3', 65, 'outliers', 4): 7}


def default_run(rig, n, kind, d, seed=None):
    key = ("default", rig, n, kind, d, seed)
    if key not in _CACHE:
        c = make_case(rig, n, kind, SEED0 + 1000 + DEFAULT_SEED_OFFSET.get((rig, n, kind, d), 0) if seed is None else seed)
        a = (c["X"], c["xl"], c["xr"] if d == 4 else None, c["P1"], c["P2"], RR.rodrigues(c["rvec0"]), c["t0"])
        run = RR.refine(*a)
        _CACHE[key] = (c, run, self_spread(*a, run))
    return _CACHE[key]


def stage_cases():
    return [(rig, n, kind, d) for rig in ("R0", "R3") for d in (2, 4) for kind in KINDS for n in STAGE_N]
