"""The references of the carry / keyframe / window chain against the renderer's ground truth (CPU): exact correspondences from
tests/_exact_chain.py through oracle.triangulate -> oracle.pnp_ransac -> _pose_ref -> _keyframe_ref.Chain -> _window_ref.update
-> _window_ref.solve.  Every pose the chain makes must be the truth pose to float32 rounding of the pixels; a transposed pose,
a swapped pose_a / pose_b or a keyframe index off by one is three to five orders of magnitude above the bar.
tests/test_gpu_exact_chain.py runs the same steps through the HIP stage calls, against the same truth and the same bar."""
import numpy as np
import pytest

import _exact_chain as EC
import _keyframe_ref as KR
import _window_ref as WR

# `python tools/chain_truth.py` prints this constant (and writes it to profiles/chain_truth.json, "exact_chain"): the largest
# absolute element difference between any pose of the twin chain -- chained, keyframe, window slot before and after the solve --
# and the truth, over both rigs, max_gap 0 and 4, W = 3 and 8 (measured 6.425e-06, rounded up to one digit).
WORST = 7e-06
# 10 x the reference's own worst, capped: the smallest convention error of this scene is ~5e-3 in a rotation element (the yaw
# between two frames, transposed) and ~0.5 m in translation (the baseline, a frame's step); the pixels' float32 rounding
# gives ~1e-5.  Were 10 x WORST above the cap, the chain would have a defect to look for, not the cap a reason to move.
BAR = min(10 * WORST, 1e-4)
X_REL = 1e-4                       # a world point against the generator's: 60 m deep at most, ~1.4e-5 from the pixels' rounding

RIGS = ("default", "R3X")
_CASE, _RUN = {}, {}


@pytest.fixture(scope="module")
def seq(synth):
    return EC.sequence(synth)


def case(seq, rig):
    if rig not in _CASE:
        P1, P2 = EC.rig_matrices(seq, rig)
        _CASE[rig] = EC.make(seq, P1=P1, P2=P2)
    return _CASE[rig]


def run(oracle, seq, rig, W, max_gap):
    if (rig, W, max_gap) not in _RUN:
        _RUN[rig, W, max_gap] = EC.twin_run(oracle, case(seq, rig), W, max_gap)
    return _RUN[rig, W, max_gap]


# ---- the generator ---------------------------------------------------------------------------------------------------------------
def _ray_miss(P, T_cw, X, xy):
    """Pixels between an observation and its world point, by back-projection (not EC.project's forward form): the distance of
    the camera-frame point from the ray C + s M^-1 [x y 1], as an angle times the focal length."""
    M, p4 = P[:, :3], P[:, 3]
    C = -np.linalg.solve(M, p4)
    d = np.linalg.solve(M, np.c_[xy.astype(np.float64), np.ones(len(xy))].T).T
    v = X @ T_cw[:3, :3].T + T_cw[:3, 3] - C
    return np.linalg.norm(np.cross(v, d), axis=1) / (np.linalg.norm(v, axis=1) * np.linalg.norm(d, axis=1)) * abs(M[0, 0])


@pytest.mark.parametrize("rig", RIGS)
def test_generator_is_consistent(seq, rig):
    c = case(seq, rig)
    assert len(c["pairs"]) == EC.N_FRAMES - 1 and np.abs(c["poses"][0] - np.eye(4)).max() < 1e-15
    assert (np.diff(c["ids"]) > 0).all() and c["ids"].min() > 1 << 33
    seen = {}
    for pr in c["pairs"]:
        assert pr["ids"].dtype == np.int64 and (np.diff(pr["ids"]) > 0).all() and len(pr["ids"]) >= 200
        assert (c["ids"][pr["idx"]] == pr["ids"]).all() and (c["born"][pr["idx"]] <= pr["a"]).all()
        for name, t, P in (("t1_left", pr["a"], c["P1"]), ("t1_right", pr["a"], c["P2"]), ("t2_left", pr["b"], c["P1"]), ("t2_right", pr["b"], c["P2"])):
            o = pr[name]
            assert o.dtype == np.float32 and o.shape == (len(pr["ids"]), 2)
            assert (o[:, 0] >= 0).all() and (o[:, 0] <= EC.W - 1).all() and (o[:, 1] >= 0).all() and (o[:, 1] <= EC.H - 1).all()
            miss = _ray_miss(c["P1"] if "left" in name else c["P2"], np.linalg.inv(c["poses"][t]), c["X"][pr["idx"]], o)
            assert miss.max() <= 4e-5, (name, miss.max())           # float32 rounding of a pixel below 512: 1.5e-5 a coordinate
            for i, xy in zip(pr["ids"], o):                          # an id is one point: its pixel in a frame is the same in every pair
                assert seen.setdefault((int(i), t, name[3:]), xy.tobytes()) == xy.tobytes()
    rel = [np.linalg.inv(c["poses"][t]) @ c["poses"][t - 1] for t in range(1, EC.N_FRAMES)]
    assert max(np.abs(r - seq.relative_gt(t + 1).numpy()).max() for t, r in enumerate(rel)) < 1e-12
    assert all(0.75 < np.linalg.norm(r[:3, 3]) < 1.25 for r in rel)


def test_default_size_passes_the_workgroup_widths(oracle, seq):
    """keyframe_join_kernel and window_update_kernel run 1024 lanes: a pair with more tracks, a table with more rows, a table
    of more rows than tracks and a join against a longer and a shorter table."""
    for rig in RIGS:
        assert max(len(pr["ids"]) for pr in case(seq, rig)["pairs"]) > 1024
        assert max(e["mid"]["m"] for e in run(oracle, seq, rig, 3, 4).steps) > 1024
    r = run(oracle, seq, "default", 3, 4)
    assert any(len(e["kf_table"][0]) > len(e["pair"]["ids"]) for e in r.steps if e["kf_table"])
    assert any(len(e["kf_table"][0]) < len(e["pair"]["ids"]) for e in r.steps if e["kf_table"])


# ---- the twins against the truth ----------------------------------------------------------------------------------------------------
def check_run(r, c, W, max_gap, bar=BAR, x_rel=X_REL):
    """What both this file and the GPU file hold a Run to."""
    for k, e in enumerate(r.steps):
        pr, kf = e["pair"], e["kf"]
        assert int(e["pnp"]["ok"]) == 1 and e["pnp"]["n_inliers"] >= 0.99 * len(pr["ids"])
        for what, d in e["dev"].items():
            assert d <= bar, (k, what, d)
        # the keyframe: the status, the index it reports and the frame its pose and its table belong to
        assert kf["status"] == (KR.APPLIED if k else KR.NONE), (k, kf["status"])
        if k:
            f = kf["kf_index"]
            assert kf["gap"] == pr["b"] - f and (kf["gap"] <= max_gap if max_gap else f == 0)
            assert EC.dev(kf["pose_K"], c["poses"][f]) <= bar
            ids, X = e["kf_table"]
            rows = np.searchsorted(c["ids"], ids)
            T = np.linalg.inv(c["poses"][f])
            want = c["X"][rows] @ T[:3, :3].T + T[:3, 3]
            assert (np.linalg.norm(X - want, axis=1) <= x_rel * np.linalg.norm(want, axis=1)).all(), k
            assert kf["n_join"] == len(np.intersect1d(ids, pr["ids"])) >= EC.MIN_TRACKS
        assert kf["switched"] == (1 if k == 0 or (max_gap and kf["gap"] >= max_gap) else 0)
        # the window: the slots' frames, the rows' ids, the world points of the rows this step made
        mid = e["mid"]
        assert mid["n"] == min(k + 2, W) == len(e["frames"]) and e["frames"] == list(range(pr["b"] - mid["n"] + 1, pr["b"] + 1))
        m = mid["m"]
        assert e["res"]["status"] == WR.APPLIED and e["res"]["n_frames"] == mid["n"] and e["res"]["n_landmarks"] == m
        assert e["res"]["cost_last"] <= e["res"]["cost_first"]
        WR.check_invariants({q: (np.asarray(mid[q])[:m] if q in ("ids", "seen", "active") else mid[q]) for q in ("n", "m", "ids", "seen", "active", "poses")})
        assert set(pr["ids"].tolist()) <= set(np.asarray(mid["ids"])[:m].tolist())
        want = c["X"][np.searchsorted(c["ids"], np.asarray(mid["ids"])[:m])]
        err = np.linalg.norm(np.asarray(mid["X"])[:m] - want, axis=1) / np.linalg.norm(want, axis=1)
        assert (e["new_rows"].sum() >= 100) == (pr["a"] % EC.EVERY == 0) and (err[e["new_rows"]] <= x_rel).all(), (k, err[e["new_rows"]].max(initial=0))
    if max_gap == 0:
        assert r.steps[-1]["kf"]["gap"] == EC.N_FRAMES - 1
    else:
        assert sum(e["kf"]["switched"] for e in r.steps) >= 3


@pytest.mark.parametrize("W", [3, 8])
@pytest.mark.parametrize("max_gap", [0, 4])
@pytest.mark.parametrize("rig", RIGS)
def test_twin_chain_is_the_truth(oracle, seq, rig, max_gap, W):
    r = run(oracle, seq, rig, W, max_gap)
    print(rig, "max_gap", max_gap, "W", W, {k: "%.2e" % v for k, v in r.worst().items()})
    check_run(r, case(seq, rig), W, max_gap)
    assert max(r.worst().values()) <= WORST                          # the committed constant is this chain's own worst


def truth_table(c, W, upto):
    """The window table over the pairs up to `upto` with the truth poses handed in and the generator's world points."""
    tab = WR.empty()
    for pr in c["pairs"][:upto]:
        tri = np.zeros((len(pr["ids"]), 3), np.float32)              # finite; every row's X is replaced below
        tab = WR.update(tab, W, pr["t1_left"], pr["t1_right"], pr["t2_left"], pr["t2_right"], pr["ids"], tri, pr["pose_a"], pr["pose_b"])
    tab["X"] = c["X"][np.searchsorted(c["ids"], tab["ids"])].copy()
    return tab


@pytest.mark.parametrize("W", [3, 8])
@pytest.mark.parametrize("rig", RIGS)
def test_solve_keeps_a_table_that_is_the_truth(seq, rig, W):
    c = case(seq, rig)
    tab = truth_table(c, W, W + 1)                                   # a full window that has slid twice
    assert tab["n"] == W
    truth = np.stack([EC.slot_truth(c["poses"][f]) for f in range(2, W + 2)])
    assert EC.dev(tab["poses"][:W], truth) < 1e-12
    r = WR.solve(tab, c["P1"], c["P2"], **EC.BA)
    move = np.linalg.norm(r["X"] - tab["X"], axis=1) / np.linalg.norm(tab["X"], axis=1)
    print(rig, W, "status", r["status"], "cost %.3e -> %.3e" % (r["cost_first"], r["cost_last"]), "poses move %.2e" % EC.dev(r["poses"][:W], truth),
          "X moves %.2e" % move.max())
    seen = WR.slot_masks(tab["seen"], W)
    in_two = int(seen[seen.sum(1) >= 2].sum())                       # W3: a landmark needs two observations; none is an outlier here
    assert r["status"] == WR.APPLIED and r["n_active"] == in_two and r["cost_last"] <= r["cost_first"] < 1e-6 * r["n_obs"]
    assert EC.dev(r["poses"][:W], truth) <= BAR and move.max() <= X_REL
