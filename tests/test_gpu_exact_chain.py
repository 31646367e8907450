"""The carry / keyframe / window chain through the HIP stage calls against the renderer's ground truth (-m gpu): the exact
correspondences of tests/_exact_chain.py through svo_triangulate -> svo_pnp_ransac -> svo_chain_relative -> svo_keyframe_join ->
svo_pnp_ransac on the joined lists -> svo_window_update -> svo_window_ba, HOST and DEVICE.  Nothing here is compared with a numpy
twin of a kernel: every pose, every window slot and every new world point is held to the truth, at the bar tests/test_exact_chain.py
derives from the references' own deviation.  Only the keyframe switch rule (K6) and the composition of the keyframe pose (K5) run
in the test, through _keyframe_ref.Chain, whose join is replaced by the stage call's lists.  The fused keyframe_update_kernel
cannot be fed exact tracks; the last test checks its read-backs against each other on rendered frames."""
import sys

import numpy as np
import pytest

import _exact_chain as EC
import _keyframe_ref as KR
from test_exact_chain import case, check_run, seq               # noqa: F401  (seq: the fixture)
from test_gpu_keyframe import MAX_GAP, MIN_TRACKS, seq12        # noqa: F401  (seq12: the fixture; no second render)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tc():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def stage_ctx(pkg):
    c = pkg.Context(64, 64, device=0)              # the stage entries are independent of the context's frame size
    yield c
    c.close()


def _inverse(R, t):
    """[R t]^-1 as a 4 x 4, in plain numpy."""
    R, t = np.asarray(R, np.float64).reshape(3, 3), np.asarray(t, np.float64).reshape(3)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R.T, -(R.T @ t)
    return T


def _check_join(e):
    """The stage call's lists: every common id, in track order, X the table's row bit for bit, xy the track's t2_left."""
    j, pr = e["joined"], e["pair"]
    ids, X = e["kf_table"]
    common = np.intersect1d(ids, pr["ids"])
    assert len(j["trk"]) == len(common) == e["kf"]["n_join"] and (np.diff(j["trk"]) > 0).all()
    assert (pr["ids"][j["trk"]] == common).all() and (ids[j["row"]] == common).all()
    assert j["X"].tobytes() == X[j["row"]].tobytes() and j["xy"].tobytes() == pr["t2_left"][j["trk"]].tobytes()


def gpu_run(ctx, c, W, max_gap, tc=None):
    """EC.Run over the stage calls; tc: torch, for operands in DEVICE memory (results come back to the host for the checks)."""
    K = EC.K_of(c["P1"])
    up = (lambda a: a) if tc is None else (lambda a: tc.from_numpy(np.ascontiguousarray(a)).cuda())
    down = (lambda a: a) if tc is None else (lambda a: a.cpu().numpy())
    last = {}

    def triangulate(P1, P2, x1, x2):
        return down(ctx.triangulate(P1, P2, up(x1), up(x2)))

    def pnp(X, xy, K):
        return ctx.pnp_ransac(up(np.asarray(X, np.float32)), up(np.asarray(xy, np.float32)), K)

    def compose(pose_a, R, t):
        T, ok = up(_inverse(R, t).reshape(1, 16)), up(np.ones(1, np.int32))
        return down(ctx.chain_relative(T, ok, pose0=pose_a)).reshape(4, 4)

    def join(tab_ids, tab_X, trk_ids, trk_xy):
        j = ctx.keyframe_join(up(tab_ids), up(tab_X), up(trk_ids), up(trk_xy))
        if tc is not None:
            n = int(j["n_out"].cpu()[0])
            j = {k: j[k].cpu().numpy()[:n] for k in ("X", "xy", "trk", "row")}
        last["j"] = j
        return j

    def kf_solve(X, xy):                                             # the twin's own join is not used: the lists are the stage call's
        return pnp(last["j"]["X"], last["j"]["xy"], K)

    def update(tab, W, pr, tri, pose_a, pose_b):
        lists = [up(pr[k]) for k in ("t1_left", "t1_right", "t2_left", "t2_right", "ids")] + [up(tri)]
        if tc is None:
            return ctx.window_update(tab, W, *lists, pose_a, pose_b)
        m_in = 0 if tab is None else tab["m"]
        t = None if tab is None else {k: v[:max(m_in, 1)] if k not in ("poses", "counts") else v for k, v in tab["dev"].items()}
        out = ctx.window_update(t, W, *lists, up(pose_a), up(pose_b), cap=m_in + len(pr["ids"]))
        return _host_view(out)

    def _host_view(d):
        h = {k: v.cpu().numpy() for k, v in d.items()}
        n, m = int(h["counts"][0]), int(h["counts"][1])
        assert h["counts"][2] == m and h["counts"][3] == 0
        res = {k: (v if k == "poses" else v[:m].copy()) for k, v in h.items() if k != "counts"}
        res["seen"], res["active"] = res["seen"].view(np.uint32), res["active"].view(np.uint32)
        res.update(n=n, m=m, dev=d)
        return res

    def solve(tab):
        if tc is None:
            return ctx.window_solve(tab, c["P1"], c["P2"], rounds=EC.BA["rounds"], iters=EC.BA["iters"], sigma_px=EC.BA["sigma"], min_obs=EC.BA["min_obs"])
        raw, d = ctx.window_solve(tab["dev"], c["P1"], c["P2"], rounds=EC.BA["rounds"], iters=EC.BA["iters"], sigma_px=EC.BA["sigma"],
                                  min_obs=EC.BA["min_obs"])          # in place: `tab`, the host copy made before, stays the table before
        ctx.sync()
        return sys.modules[type(ctx).__module__].WindowResult.from_buffer_copy(raw.cpu().numpy().tobytes()).as_dict(), _host_view(d)

    prm_inlier_rate, prm_max_move2 = 0.01, 100.0                     # svo_config's defaults, the values the fused chain's gates use
    kf = KR.Chain(EC.MIN_TRACKS, max_gap, prm_inlier_rate, prm_max_move2, kf_solve)
    return EC.Run(c, W, triangulate, pnp, compose, kf, update, solve, join=join)


def _check(r, c, W, max_gap):
    print("max_gap", max_gap, "W", W, {k: "%.2e" % v for k, v in r.worst().items()})
    check_run(r, c, W, max_gap)                                      # poses, slots, new world points, the keyframe's table: all against the truth
    for e in r.steps[1:]:
        _check_join(e)
    assert max(len(e["joined"]["trk"]) for e in r.steps[1:]) >= 100
    assert max(len(e["pair"]["ids"]) for e in r.steps) > 1024 and max(e["mid"]["m"] for e in r.steps) > 1024


@pytest.mark.parametrize("W", [3, 8])
@pytest.mark.parametrize("max_gap", [0, 4])
@pytest.mark.parametrize("rig", ["default", "R3X"])
def test_stage_chain_is_the_truth_host(stage_ctx, seq, rig, max_gap, W):
    c = case(seq, rig)
    _check(gpu_run(stage_ctx, c, W, max_gap), c, W, max_gap)


def test_stage_chain_is_the_truth_device(stage_ctx, tc, seq):
    c = case(seq, "default")
    _check(gpu_run(stage_ctx, c, 3, 4, tc), c, 3, 4)


# ---- the fused keyframe step's read-backs against each other ---------------------------------------------------------------------------
def _rodrigues(r):
    th = float(np.linalg.norm(r))
    if th == 0.0:
        return np.eye(3)
    k = np.asarray(r, np.float64) / th
    Kx = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.eye(3) + np.sin(th) * Kx + (1.0 - np.cos(th)) * (Kx @ Kx)


def test_fused_keyframe_read_backs_are_consistent(pkg, seq12):
    """keyframe_update_kernel, K5 and K6: on every APPLIED step the reported pose times [R(rvec) | tvec] is pose_K, and pose_K is
    the chain pose that get_pose() returned after frame kf_index, bit for bit."""
    sq, frames = seq12
    P1, P2 = sq.proj()
    c = pkg.Context(416, 128, device=0, P1=P1, P2=P2, max_batch=2)
    c.set_track_carry(True)
    c.set_keyframe(True, MIN_TRACKS, MAX_GAP)
    after, applied, gaps = [], 0, set()
    try:
        for t, fr in enumerate(frames):
            rc, g = c.add_frame(*fr)
            assert rc == 0
            after.append(c.get_pose().copy())
            if t == 0:
                continue
            r = c.keyframe_result()
            if r["kf_index"] >= 0:
                assert r["gap"] == t - r["kf_index"] and r["pose_K"].tobytes() == after[r["kf_index"]].tobytes(), t
            if r["status"] != pkg.KF_APPLIED:
                continue
            M = np.eye(4)
            M[:3, :3], M[:3, 3] = _rodrigues(r["rvec"]), r["tvec"]
            got = g["pose"].reshape(4, 4) @ M
            assert np.abs(got - r["pose_K"]).max() <= 1e-9 * max(1.0, np.abs(r["pose_K"]).max()), (t, np.abs(got - r["pose_K"]).max())
            applied += 1
            gaps.add(r["gap"])
    finally:
        c.close()
    assert applied >= 4 and max(gaps) >= 3
