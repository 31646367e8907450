"""numpy twin of keyframe mode (svo_set_keyframe / svo_keyframe_join, csrc/keyframe.hip): rules K1-K8 of include/svo_abi.h.
join(): the merge of a keyframe's table with a pair's tracks (K2).  Chain: a chain's keyframe state from step to step (K1,
K3-K7); the solve is a callable handed in (oracle.pnp_ransac on the GPU side's settings, or a hand-built record in the CPU
tests).  The HIP kernels must equal it bit for bit in every integer, list and table."""
import numpy as np

from _pose_ref import euler, gates, inv_rt, inv_t4, mul4  # noqa: F401  (re-exported: the chain's algebra lives in _pose_ref)

NONE, SHORT, PAIR_FAILED, REJECTED, APPLIED = 0, 1, 2, 3, 4


def join(tab_ids, tab_X, trk_ids, trk_xy):
    """K2: for every track i in ascending order whose id has a row j: (X[j], xy[i], i, j).  Both id lists strictly ascending;
    ids compare as 64-bit integers."""
    tab_ids = np.asarray(tab_ids, np.int64).reshape(-1)
    trk_ids = np.asarray(trk_ids, np.int64).reshape(-1)
    tab_X = np.asarray(tab_X, np.float32).reshape(-1, 3)
    trk_xy = np.asarray(trk_xy, np.float32).reshape(-1, 2)
    assert len(tab_X) == len(tab_ids) and len(trk_xy) == len(trk_ids)
    if len(tab_ids) == 0 or len(trk_ids) == 0:
        i = j = np.zeros(0, np.int64)
    else:
        pos = np.searchsorted(tab_ids, trk_ids)                     # the first row with id >= the track's
        hit = (pos < len(tab_ids)) & (tab_ids[np.minimum(pos, len(tab_ids) - 1)] == trk_ids)
        i, j = np.flatnonzero(hit), pos[hit]
    return dict(ids=trk_ids[i].copy(), X=tab_X[j].copy(), xy=trk_xy[i].copy(), trk=i.astype(np.int32), row=j.astype(np.int32))


def implied_motion(R, t, inv_K, pose_a):
    """K4: F = ([R t; 0 0 0 1] inv_K) pose_a, the motion a -> b the keyframe pose implies"""
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = np.asarray(R, np.float64).reshape(3, 3), np.asarray(t, np.float64).reshape(3)
    return mul4(mul4(M, inv_K), pose_a)


class Chain:
    """The keyframe state of one online chain.  solve(X, xy) -> dict(ok, R, rvec, tvec, n_inliers, ransac_iters, lm_iters, mask)."""

    def __init__(self, min_tracks=60, max_gap=0, inlier_rate=0.01, max_move2=100.0, solve=None):
        assert min_tracks >= 4 and max_gap >= 0 and max_gap != 1
        self.min_tracks, self.max_gap, self.inlier_rate, self.max_move2, self.solve = int(min_tracks), int(max_gap), inlier_rate, max_move2, solve
        self.clear()

    def clear(self):
        """K1"""
        self.valid, self.kf_index, self.pose_K, self.inv_K = False, -1, np.zeros((4, 4)), np.zeros((4, 4))
        self.ids, self.X = np.zeros(0, np.int64), np.zeros((0, 3), np.float32)

    def step(self, index_b, ok, pose_pair, pose_a, trk_ids, t2_left, tri):
        """One pair a -> b: index_b = b's frame counter, ok / pose_pair = the record's ok and pose as the gates left them,
        pose_a the chain pose before the step, the pair's track ids (ascending), t2_left and float32 triangulation.
        Returns the result dict; out["pose"] is the pose the record reports afterwards."""
        pose_pair, pose_a = np.asarray(pose_pair, np.float64).reshape(4, 4), np.asarray(pose_a, np.float64).reshape(4, 4)
        trk_ids, tri = np.asarray(trk_ids, np.int64).reshape(-1), np.asarray(tri, np.float32).reshape(-1, 3)
        valid = self.valid
        j = join(self.ids, self.X, trk_ids, t2_left) if valid else join([], np.zeros((0, 3)), [], np.zeros((0, 2)))
        n_join = len(j["trk"])
        out = dict(switched=0, kf_index=self.kf_index if valid else -1, gap=index_b - self.kf_index if valid else 0,
                   n_rows=len(self.ids) if valid else 0, n_join=n_join, n_inliers=0, ransac_iters=0, lm_iters=0, rvec=np.zeros(3),
                   tvec=np.zeros(3), pose_K=self.pose_K.copy() if valid else np.zeros((4, 4)), pose_pair=pose_pair.copy(),
                   pose=pose_pair.copy(), join=j, mask=np.zeros(n_join, np.uint8))
        solved = valid and n_join >= self.min_tracks
        s = None
        if solved:                                                   # K3 (and K7: also when the pair failed)
            s = self.solve(j["X"], j["xy"])
            out.update(n_inliers=int(s["n_inliers"]), ransac_iters=int(s["ransac_iters"]), lm_iters=int(s["lm_iters"]),
                       rvec=np.asarray(s["rvec"], np.float64).copy(), tvec=np.asarray(s["tvec"], np.float64).copy(),
                       mask=np.asarray(s["mask"], np.uint8).copy())
        if not valid:
            status = NONE
        elif not solved:
            status = SHORT
        elif not ok:
            status = PAIR_FAILED
        else:                                                        # K4
            status = REJECTED
            if s["ok"] and not (float(s["n_inliers"]) / float(n_join) < self.inlier_rate):
                if gates(implied_motion(s["R"], s["tvec"], self.inv_K, pose_a), self.max_move2):
                    status = APPLIED
                    out["pose"] = mul4(self.pose_K, inv_rt(s["R"], s["tvec"]))           # K5
        out["status"] = status
        if ok and (not valid or status != APPLIED or (self.max_gap > 0 and out["gap"] >= self.max_gap)):        # K6
            out["switched"] = 1
            fin = np.isfinite(tri).all(1)
            self.valid, self.kf_index, self.pose_K, self.inv_K = True, index_b - 1, pose_a.copy(), inv_t4(pose_a)
            self.ids, self.X = trk_ids[fin].copy(), tri[fin].copy()
        return out
