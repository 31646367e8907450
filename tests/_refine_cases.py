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


# ==== the fixtures of tests/test_gpu_refine_edges.py (tests/test_refine_ref.py proves on the CPU that each reaches its path) ===
EDGE_N = (65, 257)                               # one point past a wave, one past the workgroup stride
EDGE_KINDS = ("outliers", "some_behind")
SIGMAS = (0.5, 0.75, 2.0)
# The pixel noise of the sigma fixtures.  This mode holds the points at their true places, so at the 0.3 px of the other
# fixtures c_i = |noise|^2 / sigma^2 stays far below tau for every clean point even at sigma = 0.5 (mean 1.4 against 9.488) and
# the flags would not know what sigma is; at 0.6 px the cut at sigma = 0.5 takes a share of them (mean 5.8).
SIGMA_NOISE = 0.6


def absdiff(a, b):
    """max |a - b|; an entry that is the same non-finite number on both sides counts as equal, any other non-finite difference
    as inf."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.size == 0:
        return 0.0
    with np.errstate(invalid="ignore"):
        d = np.abs(a - b)
    d = np.where(~np.isfinite(a) & ((a == b) | (np.isnan(a) & np.isnan(b))), 0.0, d)
    return float(np.where(np.isnan(d), np.inf, d).max())


def run_ref(c, d, t0=None, **kw):
    kw = dict(dict(rounds=ROUNDS, iters=ITERS), **kw)
    return RR.refine(c["X"], c["xl"], c["xr"] if d == 4 else None, c["P1"], c["P2"], RR.rodrigues(c["rvec0"]),
                     c["t0"] if t0 is None else t0, **kw)


def edge_spread(c, d, run, starts=(1e-15, 1e-13, 1e-11, 1e-9), per=2, seed=1, **kw):
    """self_spread on the refinement's own estimate (t_ref, rvec_ref): where the PnP pose is kept, what stands is the start
    itself, which says nothing.  The fixtures whose single round is cut off by the iteration cap are not converged (a start
    1e-9 away ends further away than that): they are started 1e-15 and 1e-14 apart, as _ba_cases.far_case is."""
    kw = dict(dict(rounds=ROUNDS, iters=ITERS), **kw)
    rng, spread = np.random.default_rng(seed), 0.0
    for eps in starts:
        for _ in range(per):
            r = run_ref(c, d, t0=c["t0"] + eps * rng.standard_normal(3), **kw)
            if not (np.array_equal(r["active"], run["active"]) and r["status"] == run["status"]):
                return np.inf
            spread = max(spread, absdiff(r["t_ref"], run["t_ref"]), absdiff(r["rvec_ref"], run["rvec_ref"]))
    return spread


def edge_ok(run, spread, tight=1e-9, exits=("xi",), accept=False):
    """What a GPU test may compare on: the reference reproduces itself to a tenth of the bar from eight starts 1e-15 .. 1e-9
    apart; no c_i within 1e-6 tau of the cut at a re-classification; every round ended through one of `exits` ("xi": the
    mode's fixture_ok -- a round that ends that way has converged, its last accepted step is a tie by construction and the
    spread is what vouches for it); where a trial was rejected for a point that stopped being projectable, that point's depth
    1e-6 m or more from the cut; with `accept` (the fixtures whose rounds are cut off by the iteration cap), no accept
    decision within 1e-6 of a tie."""
    return (spread <= 0.1 * tight and all(e["exit"] in exits and e["margin"] >= 1e-6 for e in run["log"])
            and all(s[1] >= 1e-6 for e in run["log"] for s in e["steps"] if s[0] == "unprojectable")
            and (not accept or all(e["accept_margin"] >= 1e-6 for e in run["log"])))


def rig_cases():
    """Section A: the rigs with fy != fx (R1) and K2 != K1 (R2)."""
    return [(rig, n, kind, d) for rig in ("R1", "R2") for d in (2, 4) for kind in EDGE_KINDS for n in EDGE_N]


def sigma_cases():
    """Section B: sigma as data, one two-view and one one-view fixture per value."""
    return [(rig, n, kind, d, s) for s in SIGMAS for rig, n, kind, d in (("R0", 65, "some_behind", 4), ("R3", 257, "some_behind", 2))]


# per edge case, the first offset from SEED0 for which edge_ok holds (and, for sigma = 0.5, the final flags differ from the
# sigma = 1 run of the same data); find_edge_offsets() below
EDGE_SEED_OFFSET = {
    ('R1', 65, 'outliers', 2): 7,
    ('R1', 65, 'outliers', 4): 6,
    ('R1', 65, 'some_behind', 2): 19,
    ('R1', 65, 'some_behind', 4): 8,
    ('R1', 257, 'outliers', 2): 11,
    ('R1', 257, 'outliers', 4): 1,
    ('R1', 257, 'some_behind', 2): 3,
    ('R2', 65, 'outliers', 2): 9,
    ('R2', 65, 'some_behind', 4): 3,
    ('R2', 257, 'some_behind', 2): 7,
    ('R2', 257, 'some_behind', 4): 3,
    ('R0', 65, 'some_behind', 4, 0.5): 2,
    ('R0', 65, 'some_behind', 4, 0.75): 2,
    ('R0', 65, 'some_behind', 4, 2.0): 5,
    ('R3', 257, 'some_behind', 2, 0.5): 3,
    ('R3', 257, 'some_behind', 2, 0.75): 10,
    ('R3', 257, 'some_behind', 2, 2.0): 9,
}


def edge_run(rig, n, kind, d, sigma=1.0, seed=None):
    """(case, reference run, the reference's own spread) of a rig or sigma case, computed once per session and shared."""
    key = ("edge", rig, n, kind, d, sigma, seed)
    if key not in _CACHE:
        off = EDGE_SEED_OFFSET.get((rig, n, kind, d) if sigma == 1.0 else (rig, n, kind, d, sigma), 0)
        c = make_case(rig, n, kind, SEED0 + off if seed is None else seed, noise=0.3 if sigma == 1.0 else SIGMA_NOISE)
        run = run_ref(c, d, sigma=sigma)
        ok = all(e["exit"] == "xi" and e["margin"] >= 1e-6 for e in run["log"])          # (the spread costs eight more runs)
        _CACHE[key] = (c, run, edge_spread(c, d, run, sigma=sigma) if ok or seed is None else np.inf)
    return _CACHE[key]


def wrong_intrinsics(c):
    """The case with the mistake its rig exists to catch: R1 -- fy read where fx stands; R2 -- the left camera's intrinsics
    used for the right one (the left 3 x 3 of P2 becomes K1 R_rl; the fourth column stands)."""
    w = dict(c)
    P1, P2 = c["P1"].copy(), c["P2"].copy()
    if c["rig"] == "R1":
        P1[1, 1] = P1[0, 0]
    else:
        P2[:, :3] = P1[:, :3] @ np.asarray(_rigs.RIGS[c["rig"]].get("R_rl", np.eye(3)), np.float64)
    w.update(P1=P1, P2=P2)
    return w


def find_edge_offsets(limit=120):
    """Maintenance helper: the EDGE_SEED_OFFSET table."""
    table = {}
    for case in rig_cases() + sigma_cases():
        sigma = case[4] if len(case) == 5 else 1.0
        for off in range(limit):
            c, run, spread = edge_run(*case[:4], sigma=sigma, seed=SEED0 + off)
            ok = edge_ok(run, spread)
            if ok and sigma == 0.5:
                ok = not np.array_equal(run["active"], run_ref(c, case[3])["active"])
            if ok:
                if off:
                    table[case] = off
                break
        else:
            raise RuntimeError(f"no seed for {case}")
    return table


# ---- the lambda exit: the scene with exact pixels (_ba_cases.exact_case) started AT the true pose.  Every residual is exactly
# 0, g = 0, the trial cost 0 is not below the cost 0: fifteen steps are rejected (lambda 1e-4 -> 1e11), the round leaves through
# lam > 1e10.
def lambda_case():
    import _ba_cases
    c = _ba_cases.lambda_case()
    c["X"] = c["X0"]
    return c


LAMBDA_KW = (dict(rounds=1, iters=20), dict(rounds=2, iters=16))          # 15 and 30 iterations

# ---- a trial rejected because an active point stops being projectable.  Here only the pose moves, and a pose step that
# sends a point of a consistent scene behind the camera raises the cost over the others (40 seeds of _ba_cases.near_case at
# seven starts: never otherwise), so the cost would reject it anyway.  The fixture therefore holds points the TRUE pose has
# behind the camera.
NEAR_KW = dict(rounds=1, iters=6)
NEAR_SEED = {2: 0, 4: 3}
NEAR_STARTS = dict(starts=(1e-15, 1e-14), per=2)


def near_case(d, seed=None, n=300, k=3, off=0.5, noise=0.3):
    """make_case("R0", n, "outliers") with k clean points, none in wave 0 of its stride, moved to 0.1 .. 0.3 m BEHIND the t2
    camera at the true pose (their pixels: any finite ones, as for the points of `some_behind`), and the start `off` m off along
    +z, where they lie 0.2 .. 0.4 m in front of it: projectable, so active.  A step towards the true pose lowers the cost
    over the other points and carries these through the camera plane."""
    seed = NEAR_SEED[d] if seed is None else seed
    c = make_case("R0", n, "outliers", SEED0 + 3000 + seed, noise=noise)
    rng = np.random.default_rng([SEED0, seed, 78])
    R, t = c["R_true"], c["t_true"]
    cand = np.flatnonzero(~c["outlier"] & (np.arange(n) % 256 >= 64))
    idx = rng.permutation(cand)[:k]
    Y = c["X"][idx].astype(np.float64) @ R.T + t
    z = -rng.uniform(0.1, 0.3, k)
    Y = np.stack([Y[:, 0] / Y[:, 2] * 0.2, Y[:, 1] / Y[:, 2] * 0.2, z], 1)
    c["X"][idx] = ((Y - t) @ R).astype(np.float32)
    Y = c["X"][idx].astype(np.float64) @ R.T + t
    K1 = np.zeros((3, 4))
    K1[:, :3] = c["P1"][:, :3]
    c["xl"][idx] = (project(K1, Y * [1, 1, -1]) + noise * rng.standard_normal((k, 2))).astype(np.float32)
    c["xr"][idx] = (project(c["P2"], Y * [1, 1, -1]) + noise * rng.standard_normal((k, 2))).astype(np.float32)
    c.update(t0=t + off * np.array([0.0, 0.0, 1.0]), through=idx)
    return c


def unprojectable_steps(run):
    return [(r, k, s) for r, e in enumerate(run["log"]) for k, s in enumerate(e["steps"]) if s[0] == "unprojectable"]


def near_ok(run, spread, stride=256, wave=64):
    """A rejection of this kind in which every bad point lies outside wave 0 of its stride, the trial cost over the other points
    below the standing cost by 1e-6 of it or more (only the bad count decides), and edge_ok with the accept margins on the rest."""
    good = [s for _, _, s in unprojectable_steps(run)
            if len(s[2]) and (s[2] % stride >= wave).all() and s[3] < s[4] and (s[4][0] - s[3][0]) >= 1e-6 * s[4][0]]
    return bool(good) and edge_ok(run, spread, exits=("iters", "xi"), accept=True)


# ---- non-finite input: one point of a fixture_ok fixture spoiled
NONFINITE = ("nan_X", "inf_Z", "nan_x2", "inf_x2")
# the spoiled point: the k-th of the fixture's clean points; 0 unless edge_ok asks otherwise
NONFINITE_PICK = {("R0", 2, "nan_X"): 3, ("R0", 2, "inf_Z"): 3, ("R0", 2, "nan_x2"): 3, ("R0", 2, "inf_x2"): 3,
                  ("R3", 4, "nan_X"): 3, ("R3", 4, "inf_Z"): 3}


def nonfinite_case(rig, d, variant, pick=None):
    c, _ = ref_run(rig, 65, "outliers", d)
    c = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in c.items()}
    k = NONFINITE_PICK.get((rig, d, variant), 0) if pick is None else pick
    i = int(np.flatnonzero(~c["outlier"] & ~c["behind"])[k])
    if variant == "nan_X":
        c["X"][i, 1] = np.nan
    elif variant == "inf_Z":
        c["X"][i, 2] = np.inf
    elif variant == "nan_x2":
        c["xl"][i, 0] = np.nan
    elif variant == "inf_x2":
        c["xl"][i, 1] = np.inf
    else:
        raise KeyError(variant)
    c["spoiled"] = i
    return c


def nonfinite_run(rig, d, variant, pick=None):
    key = ("nonfinite", rig, d, variant, pick)
    if key not in _CACHE:
        import warnings
        c = nonfinite_case(rig, d, variant, pick)
        with np.errstate(all="ignore"), warnings.catch_warnings():
            warnings.simplefilter("ignore")
            run = run_ref(c, d)
            _CACHE[key] = (c, run, edge_spread(c, d, run))
    return _CACHE[key]
