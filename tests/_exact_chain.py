"""Exact correspondences over a synthetic sequence: world points ray-cast from the renderer's surfaces and projected through the
ground-truth poses into all four images of every pair, in float64, rounded to float32 once.  No image, no tracker: what a chain
of triangulation, PnP, pose composition, keyframe and window stages computes from these lists can differ from the truth by
float32 rounding only, so a wrong convention (a transposed pose, a swapped frame, a keyframe index off by one) shows at once.
tests/test_exact_chain.py holds the numpy twins to it, tests/test_gpu_exact_chain.py the HIP stage calls."""
import numpy as np
import torch

ID_OFFSET = (1 << 33) + 12345      # ids must compare as 64-bit integers
ID_STRIDE = 3
N_FRAMES, BIRTHS, EVERY, SEED = 12, 500, 2, 20251      # test_exact_chain.test_default_size_passes_the_workgroup_widths holds the sizes
W, H = 416, 128


def sequence(synth):
    """The 12 frames of the 416 x 128 rig that tests/test_gpu_keyframe.py renders (nothing is rendered here)."""
    return synth.StereoSequence(width=W, height=H, n_frames=N_FRAMES, seed=11)


def scaled(P, s):
    """A 3 x 4 projection matrix of an image scaled by s in x and y."""
    P = np.array(P, np.float64).reshape(3, 4)
    P[:2] *= s
    return P


def rig_matrices(seq, name):
    """(P1, P2), 3 x 4 float64: "default" = the sequence's own KITTI-like rig; any other name = that rig of tests/_rigs.py with its
    matrices scaled from 1241 to the sequence's width."""
    if name == "default":
        return tuple(np.asarray(p, np.float64).reshape(3, 4) for p in seq.proj())
    import _rigs
    return tuple(scaled(P, seq.w / float(_rigs.W)) for P in _rigs.matrices(name))


def project(P, T_cw, X):
    """P [T_cw X; 1] in float64: (pixels (n, 2), the homogeneous third coordinate (n,))."""
    Xc = X @ T_cw[:3, :3].T + T_cw[:3, 3]
    h = Xc @ P[:, :3].T + P[:, 3]
    return h[:, :2] / h[:, 2:3], h[:, 2]


def make(seq, n_frames=N_FRAMES, births=BIRTHS, every=EVERY, seed=SEED, P1=None, P2=None, margin=2.0, max_depth=60.0):
    """`births` world points every `every`-th frame (the last frame bears none), ray-cast through seq.camera / seq.depth at random
    pixels of the left image of the birth frame; points deeper than max_depth are drawn again (at 60 m the disparity is still
    2 px, so float32 rounding of the pixels moves a triangulated point by ~1e-5 of its distance).  The world is camera 0.
    Returns dict(P1, P2, poses (n_frames, 4, 4) world from camera, X (N, 3) float64, ids (N,), born (N,), pairs): pairs[k] is
    the pair a = k -> b = k + 1 with t1_left, t1_right, t2_left, t2_right (float32), ids (ascending int64), idx (rows of X),
    pose_a and pose_b (the truth)."""
    P1d, P2d = (np.asarray(p, np.float64).reshape(3, 4) for p in seq.proj())
    P1 = P1d if P1 is None else np.asarray(P1, np.float64).reshape(3, 4)
    P2 = P2d if P2 is None else np.asarray(P2, np.float64).reshape(3, 4)
    rng = np.random.default_rng(seed)
    Twc = seq.poses_wc().numpy()[:n_frames]
    T0 = np.linalg.inv(Twc[0])
    poses = np.stack([T0 @ T for T in Twc])                          # world := camera 0
    X, born = [], []
    for t in range(0, n_frames - 1, every):
        uv = np.stack([rng.uniform(0, seq.w - 1, 8 * births), rng.uniform(0, seq.h - 1, 8 * births)], 1)
        Z = seq.depth(t, 0, torch.from_numpy(uv[:, 0].copy()), torch.from_numpy(uv[:, 1].copy())).numpy()
        keep = np.flatnonzero((Z > 0.5) & (Z <= max_depth))[:births]
        assert len(keep) == births
        o, M = (a.numpy() for a in seq.camera(t, 0))
        Xw = o + Z[keep, None] * (np.c_[uv[keep], np.ones(births)] @ M.T)
        X.append(Xw @ T0[:3, :3].T + T0[:3, 3])
        born.append(np.full(births, t))
    X, born = np.concatenate(X), np.concatenate(born)
    ids = ID_OFFSET + ID_STRIDE * np.arange(len(X), dtype=np.int64)
    obs, inside = [], []
    for t in range(n_frames):
        T_cw = np.linalg.inv(poses[t])
        (l, dl), (r, dr) = project(P1, T_cw, X), project(P2, T_cw, X)
        ok = (dl > 0.5) & (dr > 0.5)                                  # in front of both cameras
        for p in (l, r):
            ok &= (p[:, 0] >= margin) & (p[:, 0] <= seq.w - 1 - margin) & (p[:, 1] >= margin) & (p[:, 1] <= seq.h - 1 - margin)
        obs.append((l.astype(np.float32), r.astype(np.float32)))
        inside.append(ok)
    pairs = []
    for a in range(n_frames - 1):
        b = a + 1
        idx = np.flatnonzero((born <= a) & inside[a] & inside[b])
        pairs.append(dict(a=a, b=b, idx=idx, ids=ids[idx].copy(), t1_left=obs[a][0][idx], t1_right=obs[a][1][idx],
                          t2_left=obs[b][0][idx], t2_right=obs[b][1][idx], pose_a=poses[a].copy(), pose_b=poses[b].copy()))
    return dict(P1=P1, P2=P2, poses=poses, X=X, ids=ids, born=born, pairs=pairs)


def K_of(P1):
    return np.asarray(P1, np.float64).reshape(3, 4)[:, :3].copy()


def slot_truth(pose):
    """The 12 numbers of a window slot (R row-major, t of Y = R X + t) of a world-from-camera truth pose."""
    M = np.linalg.inv(pose)
    return np.concatenate([M[:3, :3].ravel(), M[:3, 3]])


def dev(a, b):
    """Largest absolute element difference."""
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max(initial=0.0))


class Run:
    """The chain of stages over a generated case, the stages handed in as callables so that the numpy twins and the HIP stage
    calls run through the same steps:
        triangulate(P1, P2, x1, x2) -> (n, 3) float32          pnp(X, xy, K) -> dict(ok, R, tvec, rvec, n_inliers, mask, ...)
        compose(pose_a, R, t) -> the pair's chain pose 4 x 4    kf_chain: a _keyframe_ref.Chain whose solve is pnp
        update(tab or None, W, pair, tri, pose_a, pose_b) -> table      solve(tab) -> (result dict, table)
        join(tab_ids, tab_X, trk_ids, trk_xy) -> dict(X, xy, trk, row), optional: called before every step that has a keyframe;
        the last result is self.joined, for a solve that takes its lists from there.
    steps[k]: what step k made, and its largest deviations from the truth."""

    def __init__(self, case, W, triangulate, pnp, compose, kf_chain, update, solve, join=None):
        import _keyframe_ref as KR
        P1, P2, K = case["P1"], case["P2"], K_of(case["P1"])
        pose, tab, self.steps = np.eye(4), None, []
        self.frames = []                                            # the frame index of every slot of the table
        for pr in case["pairs"]:
            pose_a = pose
            tri = np.asarray(triangulate(P1, P2, pr["t1_left"], pr["t1_right"]))
            s = pnp(tri, pr["t2_left"], K)
            pose_pair = np.asarray(compose(pose_a, s["R"], s["tvec"]), np.float64).reshape(4, 4)
            table = (kf_chain.ids.copy(), kf_chain.X.copy()) if kf_chain.valid else None
            self.joined = join(table[0], table[1], pr["ids"], pr["t2_left"]) if join is not None and table is not None else None
            k = kf_chain.step(pr["b"], int(s["ok"]), pose_pair, pose_a, pr["ids"], pr["t2_left"], tri)
            pose = k["pose"].copy()
            n_before = 0 if tab is None else int(tab["n"])
            rows_before = set() if tab is None else set(int(i) for i in np.asarray(tab["ids"])[:tab["m"]])
            mid = update(tab, W, pr, tri, pose_a, pose)
            self.frames = [pr["a"], pr["b"]] if n_before == 0 else (self.frames[1:] if n_before == W else self.frames) + [pr["b"]]
            res, tab = solve(mid)
            new = np.array([int(i) not in rows_before for i in np.asarray(mid["ids"])[:mid["m"]]], bool)
            e = dict(pair=pr, tri=tri, pnp=s, pose_pair=pose_pair, kf=k, kf_table=table, joined=self.joined, pose=pose, mid=mid, res=res, tab=tab, new_rows=new,
                     frames=list(self.frames), applied=k["status"] == KR.APPLIED)
            truth = np.stack([slot_truth(case["poses"][f]) for f in self.frames])
            e["dev"] = dict(pose_pair=dev(pose_pair, pr["pose_b"]), pose=dev(pose, pr["pose_b"]),
                            pose_kf=dev(k["pose"], pr["pose_b"]) if e["applied"] else 0.0,
                            slots_before=dev(np.asarray(mid["poses"])[:len(truth)], truth),
                            slots_after=dev(np.asarray(tab["poses"])[:len(truth)], truth))
            self.steps.append(e)

    def worst(self):
        return {k: max(e["dev"][k] for e in self.steps) for k in self.steps[0]["dev"]}


MIN_TRACKS = 30                    # joined tracks a keyframe solve needs: low enough that frame 0 serves all 11 steps at max_gap 0
BA = dict(rounds=4, iters=2, sigma=1.0, min_obs=10)                  # the fused path's settings in tests/test_gpu_window.py


def twin_run(oracle, case, W, max_gap, min_tracks=MIN_TRACKS):
    """Run over the references alone: the oracle's triangulation and solvePnPRansac, _pose_ref, _keyframe_ref, _window_ref."""
    import _keyframe_ref as KR
    import _pose_ref as PR
    import _window_ref as WR
    prm = oracle.make_params(case["P1"], case["P2"])
    kf = KR.Chain(min_tracks, max_gap, prm.inlier_rate, prm.max_t2, lambda X, xy: oracle.pnp_ransac(X, xy, K_of(case["P1"])))

    def update(tab, W, pr, tri, pose_a, pose_b):
        return WR.update(WR.empty() if tab is None else tab, W, pr["t1_left"], pr["t1_right"], pr["t2_left"], pr["t2_right"], pr["ids"],
                         tri, pose_a, pose_b)

    def solve(tab):
        r = WR.solve(tab, case["P1"], case["P2"], **BA)
        return r, dict(tab, poses=r["poses"], X=r["X"], active=r["active"])

    return Run(case, W, oracle.triangulate, oracle.pnp_ransac, lambda pose_a, R, t: PR.mul4(pose_a, PR.inv_rt(R, t)), kf, update, solve)
