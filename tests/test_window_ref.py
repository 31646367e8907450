"""CPU test of the numpy twin of the sliding window's landmark table (tests/_window_ref.py), the reference test_gpu_window.py
holds the HIP kernel to: the rules T2-T7 of include/svo_abi.h on hand-made tables, and the invariants on every GPU fixture."""
import numpy as np
import pytest

import os
import re

import conftest
import _window_cases as WC
import _window_ref as WR


@pytest.fixture(autouse=True)
def _twin_restates_the_header():
    """The twin is the restatement of rules the header states: every test here is about a library that declares them."""
    hdr = open(os.path.join(conftest.ROOT, "include", "svo_abi.h")).read()
    assert re.search(r"#define\s+SVO_WINDOW_MAX_FRAMES\s+%d\b" % WR.MAX_FRAMES, hdr) and "tau = %.3f" % WR.TAU in hdr
    assert "svo_window_update" in hdr and "svo_set_window_ba" in hdr


def _pair(ids, base=0.0, tri=None):
    n = len(ids)
    k = np.arange(n, dtype=np.float32)[:, None]
    p = dict(ids=np.asarray(ids, np.int64), tri=np.tile(np.float32([1, 2, 10]), (n, 1)) if tri is None else np.asarray(tri, np.float32))
    for j, name in enumerate(("t1_left", "t1_right", "t2_left", "t2_right")):
        p[name] = (np.float32(base + 10 * j) + k + np.float32([0, 0.5])).astype(np.float32)
    return p


def _step(ids, base=0.0, pose_a=None, pose_b=None, **kw):
    return dict(pair=_pair(ids, base, **kw), pose_a=np.eye(4) if pose_a is None else pose_a, pose_b=np.eye(4) if pose_b is None else pose_b)


def test_first_pair_makes_two_slots_and_world_points():
    rng = np.random.default_rng(0)
    Pa, Pb = WC.rand_pose(rng), WC.rand_pose(rng)
    s = _step([3, 5, 9], pose_a=Pa, pose_b=Pb)
    t = WC.apply(WR.empty(), 4, s)
    WR.check_invariants(t)
    assert (t["n"], t["m"]) == (2, 3) and t["ids"].tolist() == [3, 5, 9] and (t["seen"] == 3).all() and (t["active"] == 0).all()
    for slot, P in ((0, Pa), (1, Pb)):                                   # T2 / T4: camera from world = inverse(chain pose)
        R, tt = t["poses"][slot, :9].reshape(3, 3), t["poses"][slot, 9:]
        M = np.eye(4)
        M[:3, :3], M[:3, 3] = R, tt
        assert np.abs(M @ P - np.eye(4)).max() < 1e-14
    Ra, ta = t["poses"][0, :9].reshape(3, 3), t["poses"][0, 9:]
    assert np.abs(t["X"] @ Ra.T + ta - [1, 2, 10]).max() < 1e-13        # X is the triangulated point taken to the world
    assert (t["obs_left"][:, 0] == s["pair"]["t1_left"]).all() and (t["obs_right"][:, 1] == s["pair"]["t2_right"]).all()
    assert (t["obs_left"][:, 2:] == 0).all()


def test_slot_before_keeps_what_it_has():
    """T5 "unless set": the second pair's t1 differs from the first pair's t2, and the row keeps the first pair's."""
    t1 = WC.apply(WR.empty(), 4, _step([1, 2]))
    t2 = WC.apply(t1, 4, _step([1, 2], base=100.0))
    assert (t2["obs_left"][:, 1] == t1["obs_left"][:, 1]).all() and (t2["obs_left"][:, 1] != _pair([1, 2], 100.0)["t1_left"]).all()
    assert (t2["obs_left"][:, 2] == _pair([1, 2], 100.0)["t2_left"]).all() and (t2["seen"] == 7).all() and (t2["X"] == t1["X"]).all()


def test_hole_is_filled_from_t1():
    """A track unusable for one pair has no observation in that pair's newest slot; the next pair fills it from its t1."""
    bad = _step([1, 2], base=50.0)
    bad["pair"]["t2_right"][1, 0] = np.inf
    t = WC.apply(WC.apply(WR.empty(), 4, _step([1, 2])), 4, bad)
    assert t["seen"].tolist() == [7, 3]
    t = WC.apply(t, 4, _step([1, 2], base=100.0))
    assert t["seen"].tolist() == [15, 15]
    assert (t["obs_left"][1, 2] == _pair([1, 2], 100.0)["t1_left"][1]).all() and (t["obs_left"][0, 2] == bad["pair"]["t2_left"][0]).all()


def test_late_row_enters_at_its_ids_place():
    s0, s1 = WC.late_row_case()
    t = WC.apply(WR.empty(), 4, s0)
    assert t["ids"].tolist() == [10, 30]
    t2 = WC.apply(t, 4, s1)
    WR.check_invariants(t2)
    assert t2["ids"].tolist() == [10, 20, 30, 40] and t2["seen"].tolist() == [7, 6, 7, 6]
    Ra, ta = t2["poses"][1, :9].reshape(3, 3), t2["poses"][1, 9:]      # made with slot a's pose: the first pair's frame b
    assert np.abs(Ra @ t2["X"][1] + ta - s1["pair"]["tri"][1]).max() < 1e-5
    assert (t2["X"][[0, 2]] == t["X"]).all()


def test_slide_drops_the_oldest_slot_and_unseen_rows():
    t = WC.apply(WR.empty(), 3, _step([1, 2, 3]))
    t = WC.apply(t, 3, _step([2, 3, 4], base=30.0))                       # n = 3 = W; id 1 is seen in slots 0, 1
    before = {k: v.copy() if hasattr(v, "copy") else v for k, v in t.items()}
    t = WC.apply(t, 3, _step([3, 4, 5], base=60.0))                       # slide: id 1 keeps slot 1 -> 0
    assert t["n"] == 3 and t["ids"].tolist() == [1, 2, 3, 4, 5] and t["seen"].tolist() == [1, 3, 7, 7, 6]
    assert (t["poses"][:2] == before["poses"][1:3]).all()
    assert (t["obs_right"][0, 0] == before["obs_right"][0, 1]).all() and (t["obs_right"][0, 1:] == 0).all()
    t = WC.apply(t, 3, _step([5], base=90.0))                             # slide: ids 1 (seen 1) leaves, 2 keeps one slot
    assert t["ids"].tolist() == [2, 3, 4, 5] and t["seen"].tolist() == [1, 3, 3, 7]
    WR.check_invariants(t)


def test_active_moves_with_the_slide_and_new_observations_are_clear():
    t = WC.apply(WC.apply(WR.empty(), 2, _step([1, 2])), 2, _step([1, 2]))
    t["active"][:] = [3, 2]
    t2 = WC.apply(t, 2, _step([1, 2]))
    assert t2["active"].tolist() == [1, 1] and t2["seen"].tolist() == [3, 3]


def test_capacity():
    t = WC.apply(WR.empty(), 3, _step([1, 2, 3]), cap=3)
    assert len(t["ids"]) == 3
    with pytest.raises(WR.Overflow) as e:
        WC.apply(t, 3, _step([3, 4]), cap=3)
    assert e.value.args[0] == 4


@pytest.mark.parametrize("name", sorted(WC.UPDATE_CASES))
def test_fixtures_obey_the_invariants(name):
    """Every GPU fixture: a valid table in, a valid table out, the counts the case is named for, ids ascending in the pair."""
    tab, frames, step, cap = WC.UPDATE_CASES[name]()
    WR.check_invariants(tab)
    assert (np.diff(step["pair"]["ids"]) > 0).all()
    out = WC.apply(tab, frames, step, cap)
    WR.check_invariants(out)
    assert out["n"] == min(max(tab["n"], 1) + 1, frames)
    if name.startswith("slide") or name.startswith("rows_"):
        assert tab["n"] == frames and ((tab["seen"][:tab["m"]] >> 1) == 0).any()           # rows drop out at this slide
    if name.startswith("rows_"):
        r, k = (int(v) for v in name.split("_")[1::2])
        assert tab["m"] == r and len(step["pair"]["ids"]) == k
        joined = np.isin(step["pair"]["ids"], tab["ids"]).sum()
        assert 0 < joined < k


# ---- the optimiser's twin (WR.solve) ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(WC.BA_CASES))
def test_ba_fixtures_are_far_from_ties(name):
    """What lets the GPU kernel be compared at 1e-9: no re-classification within 1e-6 tau of the cut, no accept decision within
    1e-6 of the cost of a tie, and the twin started 1e-15 away lands on itself to 1e-10."""
    tab, want = WC.ba_case(name)
    st = WC.ba_settings(name)
    assert len(want["log"]) == st["rounds"]
    for rd in want["log"]:
        assert rd["margin"] >= 1e-6 and rd["accept_margin"] >= 1e-6, rd
    moved = dict(tab, X=tab["X"] * (1 + 1e-15), poses=tab["poses"] * (1 + 1e-15))
    again = WR.solve(moved, WC.P1, WC.P2, **st)
    for k in ("status", "n_usable", "n_obs", "n_active", "iters"):
        assert again[k] == want[k], k
    assert (again["frame_active"] == want["frame_active"]).all() and (again["active"] == want["active"]).all()
    for k in ("poses", "X", "info"):
        scale = max(1.0, float(np.abs(want[k]).max(initial=0.0)))
        assert np.abs(again[k] - want[k]).max(initial=0.0) <= 1e-10 * scale, k


def test_ba_outcomes_cover_the_rules():
    st = {k: WC.ba_case(k)[1] for k in WC.BA_CASES}
    assert st["n8_2Tp1_holes"]["status"] == WR.APPLIED and st["n2_Tm1"]["status"] == WR.APPLIED
    low = st["slot_below_min_obs"]
    assert low["status"] == WR.KEPT and 0 < low["frame_active"][2] < WC.BA_SETTINGS["min_obs"]
    none = st["slot_without_observations"]
    assert none["status"] == WR.KEPT and none["frame_active"][2] == 0 and all(r["exit"] == "iters" for r in none["log"])
    assert none["iters"] == 8 and np.isinf([r["accept_margin"] for r in none["log"]]).all()      # every factorisation failed
    assert st["nan_observation"]["status"] == WR.KEPT and np.isnan(st["nan_observation"]["cost_first"])
    assert st["far_start"]["status"] == WR.APPLIED
    for k, o in st.items():
        tab = WC.ba_case(k)[0]
        if o["status"] != WR.APPLIED:                             # the table is handed back bit for bit
            assert o["poses"].tobytes() == tab["poses"].tobytes() and o["X"].tobytes() == tab["X"].tobytes()
            assert o["active"].tobytes() == tab["active"].tobytes()
        else:
            assert (o["poses"][0] == tab["poses"][0]).all()      # W1: slot 0 is the gauge
            assert (o["active"] & ~tab["seen"] == 0).all()


def test_ba_far_start_takes_a_cost_reject_then_an_accept():
    """The path a far start is there for: a step refused by the cost, lambda raised, a later step of the same round accepted."""
    steps = WC.ba_case("reject_then_accept")[1]["log"][0]["steps"]
    assert steps[:4] == ["unprojectable", "unprojectable", "rejected", "accepted"]
    assert WC.ba_case("far_start")[1]["log"][0]["steps"][0] == "accepted"            # (this one accepts at once)


def test_ba_pulls_the_poses_to_the_truth():
    tab, truth = WC.scene(**WC.BA_CASES["n8_2Tp1_holes"])
    o = WC.ba_case("n8_2Tp1_holes")[1]
    err = lambda P: max(np.abs(P[f, 9:] - truth["Rt"][f][1]).max() for f in range(1, 8))
    assert err(o["poses"]) < 0.25 * err(tab["poses"])


def test_ba_lambda_exit_without_observations():
    """With enough iterations a slot nobody observes drives lambda past 1e10: the round ends there (W6), the table is kept."""
    tab, _ = WC.scene(**WC.BA_CASES["slot_without_observations"])
    o = WR.solve(tab, WC.P1, WC.P2, rounds=2, iters=20, sigma=1.0, min_obs=10)
    assert [r["exit"] for r in o["log"]] == ["lambda", "lambda"] and o["iters"] == 2 * 15 and o["status"] == WR.KEPT


def test_ba_info_is_the_dense_schur_complement():
    """info = the pose block of the full normal equations with the landmarks eliminated, assembled densely here."""
    tab, o = WC.ba_case("n4_64_holes")
    assert o["status"] == WR.APPLIED
    n, m = tab["n"], tab["m"]
    R, t, X, act = o["ref"]["R"], o["ref"]["t"], o["ref"]["X"], o["ref"]["act"]
    P1, P2 = WC.P1, WC.P2
    views = [(np.array([[P1[0, 0], 0, P1[0, 2]], [0, P1[1, 1], P1[1, 2]], [0, 0, 1.0]]), np.zeros(3)), (P2[:, :3], P2[:, 3])]
    ev = WR.ba_evaluate(X, R, t, tab["obs_left"], tab["obs_right"], views, 1.0)
    D, use = 6 * (n - 1), np.nonzero(act.any(1))[0]
    J = []
    for i in use:
        for f in range(n):
            if not act[i, f]:
                continue
            for k in range(4):
                row = np.zeros(D + 3 * len(use))
                a = ev[3][i, f, k]
                if f:
                    row[6 * f - 6:6 * f] = np.concatenate([a, np.cross(ev[4][i, f], a)])
                row[D + 3 * int(np.searchsorted(use, i)):][:3] = a @ R[f]
                J.append(row)
    J = np.array(J)
    N = J.T @ J
    S = N[:D, :D] - N[:D, D:] @ np.linalg.solve(N[D:, D:], N[D:, :D])
    assert np.abs(S - o["info"][:D, :D]).max() <= 1e-9 * np.abs(S).max()
    assert (o["info"][D:] == 0).all() and (o["info"][:, D:] == 0).all()


def _clean_two_frames():
    tab, _ = WC.scene(seed=21, n=2, m=120, noise=0.05)
    tab["poses"][0] = [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]                # slot 0 at the origin: the two-frame BA's frame 1
    return tab


def test_two_frames_all_active_is_the_two_frame_ba_step():
    """n = 2 with every observation active and plain weights: the reduced system and the step are tests/_ba_ref.py's, whose
    t1 views are this window's slot 0 and whose pose is slot 1's."""
    import _ba_ref as BR
    tab = _clean_two_frames()
    m = tab["m"]
    assert (tab["seen"] == 3).all()
    R, t = tab["poses"][:2, :9].reshape(2, 3, 3), tab["poses"][:2, 9:]
    views = BR.views_of(WC.P1, WC.P2)
    X = tab["X"].copy()
    obs = [tab[k][:, f].astype(np.float64) for f in (0, 1) for k in ("obs_left", "obs_right")]
    r, c, proj, Jx, Jp = BR.evaluate(X, obs, views, R[1], t[1])
    act = np.ones(m, bool)
    assert proj.all()
    cost2, H2, g2, dU2, pts2 = BR.build(r, c, Jx, Jp, act, BR.TAU8, False, 1.0, 1e-4)
    ev = WR.ba_evaluate(X, R, t, tab["obs_left"], tab["obs_right"], views, 1.0)
    costw, Hw, gw, dUw, ptsw = WR.ba_build(ev, R, np.ones((m, 2), bool), False, 1.0, 1e-4)
    close = lambda a, b: np.abs(a - b).max() <= 1e-12 * max(1.0, np.abs(b).max())
    assert abs(costw[0] - cost2[0]) <= 1e-12 * cost2[0] and close(Hw, H2) and close(gw, g2) and close(dUw, dU2)
    ok2, xi2 = BR.RR.chol_solve6(H2 + 1e-4 * np.diag(dU2), -g2)
    okw, xiw = WR.chol_solve(Hw + 1e-4 * np.diag(dUw), -gw)
    assert ok2 and okw and close(xiw, xi2)
    assert close(WR.ba_back_substitute(ptsw, xiw), BR.back_substitute(pts2, xi2))


def test_solve_converges_to_scipy_least_squares():
    """Clean data, nothing cut: the twin's optimum is that of scipy's Levenberg-Marquardt on the same plain-weight residuals with
    the analytic Jacobian (J_p, J_x as the twin builds them)."""
    from scipy.optimize import least_squares
    tab, _ = WC.scene(seed=22, n=4, m=80, noise=0.05, holes=True)
    n, m = tab["n"], tab["m"]
    o = WR.solve(tab, WC.P1, WC.P2, rounds=4, iters=10, sigma=1.0, min_obs=5)
    assert o["status"] == WR.APPLIED and o["n_active"] == o["n_obs"]      # every observation stayed active
    views = [(np.array([[300.0, 0, 208.0], [0, 300.0, 64.0], [0, 0, 1.0]]), np.zeros(3)), (WC.P2[:, :3], WC.P2[:, 3])]
    seen = WR.slot_masks(tab["seen"], n)
    R0, t0 = tab["poses"][:n, :9].reshape(n, 3, 3), tab["poses"][:n, 9:]

    def unpack(p):
        R, t = R0.copy(), t0.copy()
        for f in range(1, n):
            E, Vr = WR.RR.se3_exp(p[6 * f - 6:6 * f])
            R[f], t[f] = E @ R0[f], E @ t0[f] + Vr
        return R, t, p[6 * (n - 1):].reshape(m, 3)

    def fun(p):
        R, t, X = unpack(p)
        return WR.ba_evaluate(X, R, t, tab["obs_left"], tab["obs_right"], views, 1.0)[1][seen].ravel()

    def jac(p):
        """The twin's own J_p and J_x at p (the pose columns are exact at p = 0 only: d exp(xi) exp(p) / d xi is taken at
        xi = 0 on the left, so the poses are re-based at every call through `base`)."""
        R, t, X = unpack(p)
        ev = WR.ba_evaluate(X, R, t, tab["obs_left"], tab["obs_right"], views, 1.0)
        rows = []
        for i, f in zip(*np.nonzero(seen)):
            for k in range(4):
                row = np.zeros(len(p))
                a = ev[3][i, f, k]
                if f:
                    row[6 * f - 6:6 * f] = np.concatenate([a, np.cross(ev[4][i, f], a)])
                row[6 * (n - 1) + 3 * i:][:3] = a @ R[f]
                rows.append(row)
        return np.array(rows)

    p0 = np.concatenate([np.zeros(6 * (n - 1)), tab["X"].ravel()])
    for _ in range(6):                                                   # re-base: poses absorbed into R0, t0, xi back to 0
        sol = least_squares(fun, p0, jac=jac, method="lm", xtol=1e-15, ftol=1e-15, gtol=1e-15, max_nfev=2)
        R0, t0, X = unpack(sol.x)
        p0 = np.concatenate([np.zeros(6 * (n - 1)), X.ravel()])
    R, t, X = unpack(sol.x)
    assert abs(2 * sol.cost - o["cost_last"]) <= 1e-9 * o["cost_last"]
    assert np.abs(R.reshape(n, 9) - o["poses"][:n, :9]).max() < 1e-8 and np.abs(t - o["poses"][:n, 9:]).max() < 1e-7
    assert np.abs(X - o["X"]).max() < 1e-5
