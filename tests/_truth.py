"""Ground truth of synth.StereoSequence for tracks on rendered frames: the surface point under a pixel, its projection into any
other view, and the distance between a tracked observation and where its surface point truly went.  chain_stats() turns a carry /
keyframe chain's read-backs into the figures tests/test_gpu_chain_truth.py bounds and tools/chain_truth.py measures; both hand it
the same lists, the test from the HIP context, the tool from the oracle twin chain."""
import numpy as np
import torch


def _uv1(xy):
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    return np.c_[xy, np.ones(len(xy))]


def world_point(seq, t, cam, xy):
    """(n, 3) float64 world points of the surfaces seen through pixels xy (n, 2) of camera `cam` (0 left, 1 right) at frame t."""
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    Z = seq.depth(t, cam, torch.from_numpy(xy[:, 0].copy()), torch.from_numpy(xy[:, 1].copy())).numpy()
    o, M = (a.numpy() for a in seq.camera(t, cam))
    return o + Z[:, None] * (_uv1(xy) @ M.T)                        # M [u v 1] has camera-frame depth 1


def project(seq, t, cam, Xw):
    """(pixels (n, 2), depth (n,)) of world points in camera `cam` at frame t, float64."""
    o, M = (a.numpy() for a in seq.camera(t, cam))
    p = np.linalg.solve(M, (np.asarray(Xw, np.float64).reshape(-1, 3) - o).T).T
    return p[:, :2] / p[:, 2:3], p[:, 2]


def transfer_error(seq, t_from, xy_from, t_to, xy_to, cam_from=0, cam_to=0):
    """Pixels between the observations xy_to in (t_to, cam_to) and the true projections of the surface points under xy_from in
    (t_from, cam_from)."""
    want, _ = project(seq, t_to, cam_to, world_point(seq, t_from, cam_from, xy_from))
    return np.linalg.norm(np.asarray(xy_to, np.float64).reshape(-1, 2) - want, axis=1)


def table_disparity_error(seq, kf, X):
    """fx b / Z_table - fx b / Z_truth per row of a keyframe table (X: (n, 3) in the left camera frame of frame kf), Z_truth
    sampled with seq.depth at the pixel the row projects to in the keyframe.  Rectified rigs only."""
    X = np.asarray(X, np.float64).reshape(-1, 3)
    u, v = seq.fx * X[:, 0] / X[:, 2] + seq.cx, seq.fy * X[:, 1] / X[:, 2] + seq.cy
    Z = seq.depth(kf, 0, torch.from_numpy(u), torch.from_numpy(v)).numpy()
    return seq.fx * seq.baseline * (1.0 / X[:, 2] - 1.0 / Z)


def chain_stats(seq, steps):
    """steps[k] for the pair k -> k + 1: dict(tracks = (t1_left, t1_right, t2_right, t2_left, inlier) in last_tracks()' order,
    ids, and `table` = (kf_index, X) where the step took a new keyframe, else None).  Returns
      pair:    median / p99 / max over the PnP inliers of all pairs of |t2_left - truth(surface under t1_left)|, and their count;
      age:     {age: median} over every observation of |t2_left - truth(surface under the id's FIRST t1_left)|, age = frames since;
      beyond10: share of the inlier observations of that list more than 10 px off, and their count;
      table:   median |e| and |mean e| of the disparity error e over every keyframe table, and the rows."""
    first, pair, by_age, carried_inl, tab = {}, [], {}, [], []
    for k, s in enumerate(steps):
        t1l, t2l, inl = s["tracks"][0], s["tracks"][3], np.asarray(s["tracks"][4]) != 0
        ids = np.asarray(s["ids"], np.int64)
        assert len(ids) == len(t1l)
        pair.append(transfer_error(seq, k, t1l[inl], k + 1, t2l[inl]))
        for i, xy in zip(ids, t1l):
            first.setdefault(int(i), (k, xy))
        born = np.array([first[int(i)][0] for i in ids])
        xy0 = np.array([first[int(i)][1] for i in ids], np.float64).reshape(-1, 2)
        err = np.zeros(len(ids))
        for t0 in np.unique(born):
            q = born == t0
            err[q] = transfer_error(seq, int(t0), xy0[q], k + 1, t2l[q])
        for age in np.unique(k + 1 - born):
            by_age.setdefault(int(age), []).append(err[k + 1 - born == age])
        carried_inl.append(err[inl])
        if s.get("table") is not None:
            tab.append(table_disparity_error(seq, *s["table"]))
    pair, carried_inl, tab = np.concatenate(pair), np.concatenate(carried_inl), np.concatenate(tab)
    return dict(pair=dict(median=float(np.median(pair)), p99=float(np.percentile(pair, 99)), max=float(pair.max()), n=len(pair)),
                age={a: float(np.median(np.concatenate(v))) for a, v in sorted(by_age.items())},
                age_n={a: int(sum(len(x) for x in v)) for a, v in sorted(by_age.items())},
                age_over3={a: float((np.concatenate(v) > 3.0).mean()) for a, v in sorted(by_age.items())},
                beyond10=dict(share=float((carried_inl > 10.0).mean()), n=len(carried_inl)),
                table=dict(median_abs=float(np.median(np.abs(tab))), abs_mean=float(abs(tab.mean())), n=len(tab)))
