"""Synthetic fixtures of the bundle-adjustment tests (CPU twin tests and GPU stage-call tests share them).

A case is _refine_cases.make_case (float32 t2 observations in both cameras under a known motion, 0.3 px noise, gross outliers,
optionally points behind the camera) plus what the bundle adjustment reads beside them: float32 t1 observations, the TRUE
points projected into both views with 0.3 px noise, and X0, the oracle's triangulation of those t1 observations -- the noisy
float32 start that the fused path hands the stage.  A point "behind the camera" has no triangulation worth the name: it keeps
make_case's point, so that the kinds some_behind / all_behind mean here what they mean there."""
import numpy as np

import conftest
import _ba_ref as BA
import _refine_cases as RC
import _refine_ref as RR
import _rigs

STAGE_N, KINDS, SEED0 = RC.STAGE_N, RC.KINDS, RC.SEED0
# The settings the fixtures are run with: 4 rounds of 2 iterations.  From 10 cm off the first two steps of a round change the
# cost by 1e-2 .. 1e-6 of itself; from the third on the change is ~1e-15 of it, i.e. whether the step is accepted is decided
# by the rounding of the cost's terms, and with it where a weakly determined point (depth at 40 m: d^2 cost / dz^2 ~ 0.1) ends,
# to ~1e-8.  A comparison at 1e-9 says something only where every decision is far from a tie, so the cap keeps the rounds
# inside that regime; the eight steps still end within the noise of the data (4 mm of the true translation).
# The six-point cases have no outliers: their later rounds have nothing to re-classify and would start converged, every
# decision a tie; they run the two Huber rounds only.
ROUNDS, ITERS = 4, 2


def settings(n):
    return dict(rounds=2 if n <= 6 else ROUNDS, iters=ITERS)

def make_case(rig, n, kind, seed=SEED0, noise=0.3):
    c = RC.make_case(rig, n, kind, seed, noise=noise)
    rng = np.random.default_rng([seed, n, KINDS.index(kind), sorted(_rigs.RIGS).index(rig), 1])
    P1, P2 = c["P1"], c["P2"]
    K1 = np.zeros((3, 4))
    K1[:, :3] = [[P1[0, 0], 0, P1[0, 2]], [0, P1[1, 1], P1[1, 2]], [0, 0, 1]]
    X = c["X"].astype(np.float64)
    Xs = np.where(c["behind"][:, None], X * [1, 1, -1], X)          # any finite pixel for the points nobody sees
    x1l = (RC.project(K1, Xs) + noise * rng.standard_normal((n, 2))).astype(np.float32)
    x1r = (RC.project(P2, Xs) + noise * rng.standard_normal((n, 2))).astype(np.float32)
    X0 = conftest.entry.load_oracle().triangulate(P1, P2, x1l, x1r) if n else np.zeros((0, 3), np.float32)
    X0[c["behind"]] = c["X"][c["behind"]]
    c.update(x1l=x1l, x1r=x1r, X0=np.ascontiguousarray(X0, np.float32))
    return c


def run_twin(c, d, t0=None, **kw):
    kw = dict(settings(len(c["X0"])), **kw)
    return BA.refine_ba(c["X0"], c["x1l"], c["x1r"], c["xl"], c["xr"] if d == 8 else None, c["P1"], c["P2"],
                        RR.rodrigues(c["rvec0"]), c["t0"] if t0 is None else t0, **kw)


def self_spread(c, d, run, starts=(1e-15,), per=1, seed=1, **kw):
    """How far the twin's own outcomes lie apart on a fixture: started `per` times at each distance of `starts` from t0, the
    largest |t|, |rvec| or |X| difference to `run`; inf where the flags or the status differ."""
    rng, spread = np.random.default_rng(seed), 0.0
    for eps in starts:
        for _ in range(per):
            r = run_twin(c, d, t0=c["t0"] + eps * rng.standard_normal(3), **kw)
            if not (np.array_equal(r["active"], run["active"]) and r["status"] == run["status"]):
                return np.inf
            # (the adjustment's own estimate: when the PnP pose is kept, what stands is the start itself)
            spread = max(spread, np.abs(r["t_ref"] - run["t_ref"]).max(), np.abs(r["rvec_ref"] - run["rvec_ref"]).max(),
                         np.abs(r["X_ref"] - run["X_ref"]).max() if len(r["X_ref"]) else 0.0)
    return spread


def fixture_ok(run, spread, tight):
    """What a GPU test may compare on: started 1e-15 apart the twin reproduces itself to a tenth of the bar, no c_i lies within
    1e-6 tau of the cut at a re-classification, and at no accept decision the trial cost lies within 1e-6 of the cost it is
    compared with, relative to that cost (a difference that small is decided by the rounding of the terms)."""
    return spread <= 0.1 * tight and all(e["margin"] >= 1e-6 and e["accept_margin"] >= 1e-6 for e in run["log"])


# per case, the first offset from SEED0 for which fixture_ok holds (find_seed_offsets below; "pick another seed, do not loosen
# the bar")
SEED_OFFSET = {
    ('R0', 63, 'some_behind', 6): 3,
    ('R0', 64, 'some_behind', 6): 3,
    ('R0', 64, 'some_behind', 8): 5,
    ('R0', 255, 'outliers', 6): 2,
    ('R0', 255, 'outliers', 8): 2,
    ('R0', 257, 'outliers', 6): 1,
    ('R0', 257, 'outliers', 8): 1,
    ('R3', 6, 'outliers', 6): 1,
    ('R3', 63, 'outliers', 6): 1,
    ('R3', 63, 'outliers', 8): 1,
    ('R3', 63, 'some_behind', 8): 7,
    ('R3', 64, 'outliers', 6): 2,
    ('R3', 64, 'outliers', 8): 5,
    ('R3', 64, 'some_behind', 6): 1,
    ('R3', 64, 'some_behind', 8): 3,
    ('R3', 65, 'outliers', 6): 3,
    ('R3', 65, 'outliers', 8): 2,
    ('R3', 256, 'some_behind', 8): 2,
    ('R3', 257, 'outliers', 8): 1,
    ('R3', 257, 'some_behind', 8): 3,
}


def stage_cases():
    return [(rig, n, kind, d) for rig in ("R0", "R3") for d in (6, 8) for kind in KINDS for n in STAGE_N]


_CACHE = {}


def ref_run(rig, n, kind, d, seed=None):
    """(case, twin run), computed once per session and shared."""
    key = (rig, n, kind, d, seed)
    if key not in _CACHE:
        c = make_case(rig, n, kind, SEED0 + SEED_OFFSET.get((rig, n, kind, d), 0) if seed is None else seed)
        _CACHE[key] = (c, run_twin(c, d))
    return _CACHE[key]


def ref_spread(rig, n, kind, d, seed=None):
    c, run = ref_run(rig, n, kind, d, seed)
    return 0.0 if kind == "all_behind" else self_spread(c, d, run)


def find_seed_offsets(tight=1e-9, limit=200):
    """Maintenance helper: the SEED_OFFSET table."""
    table = {}
    for case in stage_cases():
        if case[2] == "all_behind":
            continue
        for off in range(limit):
            _, run = ref_run(*case, seed=SEED0 + off)
            if fixture_ok(run, ref_spread(*case, seed=SEED0 + off), tight):
                if off:
                    table[case] = off
                break
        else:
            raise RuntimeError(f"no seed for {case}")
    return table


# ---- cases that take the LM branches the 4 x 2 fixtures never reach, each decisively ---------------------------------------
def exact_case(n=70, seed=1, off=0.05):
    """A scene whose pixels are exact: f = 512, dyadic coordinates, depths 2 / 4 / 8 m, a motion of 0.25 m along x, identity
    rotation -- every projection is a float32 number and every residual is exactly 0 in double at the true estimate.  With
    nothing for the terms of the cost to round, the cost falls by its own size with every step down to 1e-14 m (quadratic
    convergence of a zero-residual problem), so a round started 5 cm and 0.1 degree off ends through the short-step exit
    (|xi| < 1e-10, max |dX| < 1e-9) after four accepted steps, none of them near a tie."""
    rng = np.random.default_rng(seed)
    f, cx, cy, b = 512.0, 320.0, 96.0, 0.5
    P1 = np.array([[f, 0, cx, 0], [0, f, cy, 0], [0, 0, 1, 0.0]])
    P2 = P1.copy()
    P2[0, 3] = -f * b
    Z = rng.choice([2.0, 4.0, 8.0], n)
    X = np.stack([rng.integers(-64, 65, n) / 64.0 * Z / 4, rng.integers(-32, 33, n) / 64.0 * Z / 4, Z], 1)
    t = np.array([0.25, 0.0, 0.0])
    obs = [RC.project(P, Y) for Y in (X, X + t) for P in (P1, P2)]
    assert all(np.array_equal(o, o.astype(np.float32).astype(np.float64)) for o in obs)
    rvec0 = np.deg2rad(0.1) * np.array([0.6, -0.48, 0.64])
    return dict(P1=P1, P2=P2, X0=X.astype(np.float32), x1l=obs[0].astype(np.float32), x1r=obs[1].astype(np.float32),
                xl=obs[2].astype(np.float32), xr=obs[3].astype(np.float32), rvec0=rvec0, t0=t + off * np.array([0.48, 0.6, -0.64]),
                R_true=np.eye(3), t_true=t)


EXACT_KW = dict(rounds=1, iters=12)


def far_case(d):
    """A start 1 m and 3 degrees off the true pose: at lambda = 1e-4 a Gauss-Newton step from there overshoots, the cost rises
    by a tenth of itself or more and the step is rejected; the retry at 10 lambda from the untouched points is accepted.
    One round of four iterations; d = 6: the FIRST step is the rejected one, d = 8: the second."""
    from scipy.spatial.transform import Rotation
    c = make_case("R0", 65, "outliers", SEED0 + (1 if d == 6 else 0))
    R0 = Rotation.from_rotvec(np.deg2rad(3.0) * np.array([0.6, -0.48, 0.64])).as_matrix() @ c["R_true"]
    c.update(rvec0=RR.so3_log(R0), t0=c["t_true"] + 1.0 * np.array([0.48, 0.6, -0.64]))
    return c


FAR_KW = dict(rounds=1, iters=4)

# The default settings (4 rounds x 10 iterations) run into the regime where rounding decides the accept test, so what can be
# asked there is what the twin asks of itself.  Measured with the twin alone, eight starts 1e-15 .. 1e-9 apart, three seeds per
# case: flags and status always equal; pose up to 1.8e-10, points up to 1.5e-7 apart (R0 257 outliers d = 8: 7.8e-11 / 1.0e-7;
# R3 65 some_behind d = 6: 1.8e-10 / 1.5e-7).  The bars are ten times the largest figure; info moves with the points at first
# order (1 / depth per metre, depths >= 4 m), so the points' bar bounds its relative change.
DEFAULT_CASES = [("R0", 257, "outliers", 8), ("R3", 65, "some_behind", 6)]
DEFAULT_POSE_BAR, DEFAULT_POINT_BAR, DEFAULT_INFO_BAR = 2e-9, 2e-6, 2e-6


def default_run(rig, n, kind, d):
    key = ("default", rig, n, kind, d)
    if key not in _CACHE:
        c = make_case(rig, n, kind, SEED0 + 2000)
        _CACHE[key] = (c, run_twin(c, d, rounds=4, iters=10))
    return _CACHE[key]


# ==== the fixtures of tests/test_gpu_refine_edges.py (tests/test_ba_ref.py proves on the CPU that each reaches its path) =======
# Every one is run at settings(n) -- 4 x 2 -- unless its own settings are named, and must meet fixture_ok.
EDGE_N = (65, 257)                               # one point past a wave, one past the workgroup stride
EDGE_KINDS = ("outliers", "some_behind")
SIGMAS = (0.5, 0.75, 2.0)


def absdiff(a, b):
    """max |a - b| where an entry that is the same non-finite number on both sides counts as equal, any other non-finite
    difference as inf (the fixtures with a spoiled point carry that point's NaN / inf through)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.size == 0:
        return 0.0
    with np.errstate(invalid="ignore"):
        d = np.abs(a - b)
    same = ~np.isfinite(a) & ((a == b) | (np.isnan(a) & np.isnan(b)))
    d = np.where(same, 0.0, d)
    return float(np.where(np.isnan(d), np.inf, d).max())


def edge_spread(c, d, run, **kw):
    """self_spread, with the non-finite entries of a spoiled point compared as what they are."""
    r = run_twin(c, d, t0=c["t0"] + 1e-15 * np.random.default_rng(1).standard_normal(3), **kw)
    if not (np.array_equal(r["active"], run["active"]) and r["status"] == run["status"]):
        return np.inf
    return max(absdiff(r["t_ref"], run["t_ref"]), absdiff(r["rvec_ref"], run["rvec_ref"]), absdiff(r["X_ref"], run["X_ref"]))


def edge_ok(run, spread, tight):
    """fixture_ok, and where a trial was rejected for a point that stopped being projectable (the twin's log names it), that
    point's depth 1e-6 m or more from the cut: that decision does not hang on a last bit either."""
    return fixture_ok(run, spread, tight) and all(s[1] >= 1e-6 for e in run["log"] for s in e["steps"] if s[0] == "unprojectable")


def rig_cases():
    """Section A: the rigs with fy != fx (R1) and K2 != K1 (R2)."""
    return [(rig, n, kind, d) for rig in ("R1", "R2") for d in (6, 8) for kind in EDGE_KINDS for n in EDGE_N]


def sigma_cases():
    """Section B: sigma as data, one four-view and one three-view fixture per value."""
    return [(rig, n, kind, d, s) for s in SIGMAS for rig, n, kind, d in (("R0", 65, "some_behind", 8), ("R3", 257, "some_behind", 6))]


# per edge case, the first offset from SEED0 for which fixture_ok holds (and, for sigma = 0.5, the final flags differ from the
# sigma = 1 run of the same data); find_edge_offsets() below
EDGE_SEED_OFFSET = {
    ('R1', 65, 'outliers', 6): 1,
    ('R1', 65, 'outliers', 8): 1,
    ('R1', 257, 'some_behind', 6): 1,
    ('R2', 65, 'outliers', 6): 2,
    ('R2', 65, 'outliers', 8): 3,
    ('R2', 65, 'some_behind', 6): 2,
    ('R2', 65, 'some_behind', 8): 6,
    ('R2', 257, 'outliers', 8): 1,
    ('R0', 65, 'some_behind', 8, 2.0): 1,
}


def edge_run(rig, n, kind, d, sigma=1.0, seed=None):
    """(case, twin run, twin's own spread) of a rig or sigma case, computed once per session and shared."""
    key = ("edge", rig, n, kind, d, sigma, seed)
    if key not in _CACHE:
        off = EDGE_SEED_OFFSET.get((rig, n, kind, d) if sigma == 1.0 else (rig, n, kind, d, sigma), 0)
        c = make_case(rig, n, kind, SEED0 + off if seed is None else seed)
        run = run_twin(c, d, sigma=sigma)
        _CACHE[key] = (c, run, self_spread(c, d, run, sigma=sigma))
    return _CACHE[key]


def wrong_intrinsics(c):
    """The case with the mistake its rig exists to catch: R1 -- fy read where fx stands; R2 -- the left camera's intrinsics
    used for the right one (the left 3 x 3 of P2 becomes K1 R_rl; the fourth column stands)."""
    w = dict(c)
    P1, P2 = c["P1"].copy(), c["P2"].copy()
    if c["rig"] == "R1":
        P1[1, 1] = P1[0, 0]
    else:
        r = _rigs.RIGS[c["rig"]]
        P2[:, :3] = P1[:, :3] @ np.asarray(r.get("R_rl", np.eye(3)), np.float64)
    w.update(P1=P1, P2=P2)
    return w


def find_edge_offsets(tight=1e-9, limit=60):
    """Maintenance helper: the EDGE_SEED_OFFSET table."""
    table = {}
    for case in rig_cases() + sigma_cases():
        sigma = case[4] if len(case) == 5 else 1.0
        for off in range(limit):
            c, run, spread = edge_run(*case[:4], sigma=sigma, seed=SEED0 + off)
            ok = edge_ok(run, spread, tight)
            if ok and sigma == 0.5:
                ok = not np.array_equal(run["active"], run_twin(c, case[3])["active"])
            if ok:
                if off:
                    table[case] = off
                break
        else:
            raise RuntimeError(f"no seed for {case}")
    return table


# ---- the lambda exit: the exact scene started AT the true pose.  Every residual is exactly 0, the trial cost 0 is not below
# the cost 0, fifteen steps are rejected (lambda 1e-4 -> 1e11) and the round leaves through lam > 1e10; nothing is rounded,
# so the tie is exact on both sides.
def lambda_case():
    c = exact_case()
    c.update(rvec0=np.zeros(3), t0=c["t_true"].copy())
    return c


LAMBDA_KW = (dict(rounds=1, iters=20), dict(rounds=2, iters=16))          # 15 and 30 iterations


# ---- a trial rejected because an active point stops being projectable.  15 % of the points lie 0.3 .. 0.6 m in front of the
# t2 camera; from 0.5 m off along -z a step moves the pose (and the points) far enough for one of them to end behind a camera
# while the cost over the others falls: the bad count alone rejects the step.
NEAR_KW = dict(rounds=1, iters=6)
NEAR_SEED = {6: 1, 8: 0}


def near_case(d, seed=None, n=300, share=0.15, off=0.5, noise=0.3, rig="R0", outlier_share=0.3):
    seed = NEAR_SEED[d] if seed is None else seed
    P1, P2 = _rigs.matrices(rig)
    rng = np.random.default_rng([SEED0, seed, 77])
    R, t = RC.true_pose()
    K1 = np.zeros((3, 4))
    K1[:, :3] = [[P1[0, 0], 0, P1[0, 2]], [0, P1[1, 1], P1[1, 2]], [0, 0, 1]]
    u, v, z = rng.uniform(40, _rigs.W - 40, n), rng.uniform(20, _rigs.H - 20, n), rng.uniform(4.0, 40.0, n)
    near = rng.permutation(n)[:int(share * n)]
    z[near] = rng.uniform(0.3, 0.6, len(near))
    Y = np.stack([(u - K1[0, 2]) / K1[0, 0] * z, (v - K1[1, 2]) / K1[1, 1] * z, z], 1)
    X = ((Y - t) @ R).astype(np.float32).astype(np.float64)
    Y = X @ R.T + t
    obs = [(RC.project(P, Z) + noise * rng.standard_normal((n, 2))).astype(np.float32) for Z in (X, Y) for P in (K1, P2)]
    outlier = np.zeros(n, bool)
    outlier[rng.permutation(n)[:int(outlier_share * n)]] = True
    ang, rad = rng.uniform(0, 2 * np.pi, outlier.sum()), rng.uniform(15.0, 80.0, outlier.sum())      # gross, as make_case's
    o2 = np.stack([rad * np.cos(ang), rad * np.sin(ang)], 1).astype(np.float32)
    obs[2][outlier] += o2
    obs[3][outlier] -= o2[:, ::-1]
    X0 = np.ascontiguousarray(conftest.entry.load_oracle().triangulate(P1, P2, obs[0], obs[1]), np.float32)
    R0, _ = RC.start_pose()
    return dict(rig=rig, P1=P1, P2=P2, X=X.astype(np.float32), X0=X0, x1l=obs[0], x1r=obs[1], xl=obs[2], xr=obs[3], rvec0=RR.so3_log(R0),
                t0=t + off * np.array([0.0, 0.0, -1.0]), R_true=R, t_true=t, near=near, outlier=outlier)


def unprojectable_steps(run):
    """The twin's rejections for a point that stops being projectable: (round, step index, entry)."""
    return [(r, k, s) for r, e in enumerate(run["log"]) for k, s in enumerate(e["steps"]) if s[0] == "unprojectable"]


def near_ok(run, spread, tight, stride=256, wave=64):
    """What section C asks of such a fixture: a rejection of this kind in which every bad point lies outside wave 0 of its
    stride (wave 0's bad count is zero: a sum over wave 0 alone would accept), the trial cost over the other points BELOW the
    standing cost (only the bad count decides), every bad depth 1e-6 m or more from the cut, and fixture_ok on the rest."""
    good = [s for _, _, s in unprojectable_steps(run)
            if len(s[2]) and (s[2] % stride >= wave).all() and s[3] < s[4] and (s[4][0] - s[3][0]) >= 1e-6 * s[4][0]]
    return bool(good) and edge_ok(run, spread, tight)


# ---- non-finite input: one point of a fixture_ok fixture spoiled
NONFINITE = ("nan_X", "inf_Z", "nan_x2", "nan_x1", "inf_x2")
NONFINITE_BASE = [("R0", 65, "outliers"), ("R3", 65, "outliers")]
# the spoiled point: the k-th of the fixture's clean points (neither outlier nor behind); 0 unless the margins ask otherwise
NONFINITE_PICK = {}


def nonfinite_case(rig, d, variant, pick=None):
    c, _ = ref_run(rig, 65, "outliers", d)
    c = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in c.items()}
    k = NONFINITE_PICK.get((rig, d, variant), 0) if pick is None else pick
    i = int(np.flatnonzero(~c["outlier"] & ~c["behind"])[k])
    if variant == "nan_X":
        c["X0"][i, 1] = np.nan
    elif variant == "inf_Z":
        c["X0"][i, 2] = np.inf
    elif variant == "nan_x2":
        c["xl"][i, 0] = np.nan
    elif variant == "nan_x1":
        c["x1r"][i, 1] = np.nan
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
            run = run_twin(c, d)
            _CACHE[key] = (c, run, edge_spread(c, d, run))
    return _CACHE[key]
