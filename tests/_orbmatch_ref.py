"""Reference twin of the guided ORB matcher (include/svo_abi.h, "guided ORB matcher"): numpy only.

Stage S (stereo, once per frame) and stage T (temporal, per pair) stated step by step as the ABI comment states them, every
float operation a float32 operation with one rounding.  Inputs are keypoint records (oracle.KP_DTYPE fields x, y, octave),
(n, 32) uint8 descriptors and the UNBLURRED pyramid levels of the images (oracle.orb_pyramid_level)."""
import numpy as np

F = np.float32
TH_STEREO, TH_TRACK, RATIO = 75, 100, 0.9
_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


def scales(scale_factor=1.2, nlevels=8):
    """OrbGeom.scale as orb_make_geom computes it (float product through a double), and inv = 1.0f / scale."""
    sc = np.zeros(nlevels, F)
    sc[0] = F(1.0)
    sf = float(F(scale_factor))
    for i in range(1, nlevels):
        sc[i] = F(float(sc[i - 1]) * sf)
    return sc, (F(1.0) / sc).astype(F)


def rnd(x):
    return int(np.floor(F(F(x) + F(0.5))))


def hamming(a, b):
    """Hamming distances of descriptor a (32,) against rows b (m, 32)."""
    return _POP[np.bitwise_xor(b, a[None, :])].sum(1)


def patch_of(kp, levels, inv):
    """(valid, pu, pv, 11 x 11 raw bytes) of a left keypoint on its own octave."""
    o = int(kp["octave"])
    img = levels[o]
    h, w = img.shape
    pu, pv = rnd(F(kp["x"]) * inv[o]), rnd(F(kp["y"]) * inv[o])
    if not (5 <= pu < w - 5 and 5 <= pv < h - 5):
        return False, pu, pv, np.zeros((11, 11), np.uint8)
    return True, pu, pv, img[pv - 5:pv + 6, pu - 5:pu + 6].copy()


def sad(patch, J, cu, cv):
    T = patch.astype(np.int32) - int(patch[5, 5])
    W = J[cv - 5:cv + 6, cu - 5:cu + 6].astype(np.int32) - int(J[cv, cu])
    return int(np.abs(T - W).sum())


def parabola(d1, d2, d3):
    d1, d2, d3 = F(d1), F(d2), F(d3)
    den = F(F(2.0) * F(F(d1 + d3) - F(F(2.0) * d2)))
    return F(0.0) if den == 0 else F(F(d1 - d3) / den)


def median_cut(sads):
    """Indices (into `sads`) that survive: (float)sad < (1.5f * 1.4f) * (float)med, med = element n/2 of the sorted list."""
    sads = np.asarray(sads, np.int64)
    if len(sads) == 0:
        return np.zeros(0, bool)
    med = np.sort(sads)[len(sads) // 2]
    thr = F(F(F(1.5) * F(1.4)) * F(med))
    return sads.astype(F) < thr


def stereo(kL, dL, kR, dR, levL, levR, max_disparity, th_stereo=TH_STEREO, scale_factor=1.2, return_j=False):
    """Stage S.  Returns (uR float32 (n,), sad int32 (n,), patches uint8 (n, 121)); uR -1 / sad -1: no stereo match.  With
    return_j also the chosen right index per left keypoint (the packed minimum's j, before any threshold; -1: no candidate)."""
    sc, inv = scales(scale_factor, len(levL))
    n = len(kL)
    maxD = F(max_disparity)
    uR = np.full(n, -1.0, F)
    sd = np.full(n, -1, np.int32)
    patches = np.zeros((n, 121), np.uint8)
    jbest = np.full(n, -1, np.int32)
    xR, yR, oR = kR["x"].astype(F), kR["y"].astype(F), kR["octave"].astype(np.int64)
    rj = (F(2.0) * sc[oR]).astype(F)
    lo, hi = np.floor((yR - rj).astype(F)), np.ceil((yR + rj).astype(F))
    jj = np.arange(len(kR))
    for i in range(n):
        uL, vL, oL = F(kL["x"][i]), F(kL["y"][i]), int(kL["octave"][i])
        valid, pu, pv, patch = patch_of(kL[i], levL, inv)
        if valid:
            patches[i] = patch.reshape(-1)
        if len(kR) == 0:
            continue
        tv = np.trunc(vL)
        cand = (lo <= tv) & (tv <= hi) & (np.abs(oR - oL) <= 1) & (F(uL - maxD) <= xR) & (xR <= uL)
        if not cand.any():
            continue
        keys = (hamming(dL[i], dR[cand]).astype(np.int64) << 16) | jj[cand]
        key = int(keys.min())
        best, j = key >> 16, key & 0xFFFF
        jbest[i] = j
        if best >= th_stereo:
            continue
        J = levR[oL]
        w = J.shape[1]
        sr = rnd(xR[j] * inv[oL])
        if not valid or sr - 10 < 0 or sr + 11 >= w:
            continue
        d = [sad(patch, J, sr + k, pv) for k in range(-5, 6)]
        kb = int(np.argmin(d))                     # first minimum
        if kb == 0 or kb == 10:
            continue
        delta = parabola(d[kb - 1], d[kb], d[kb + 1])
        u = F(sc[oL] * F(F(F(sr) + F(kb - 5)) + delta))
        disp = F(uL - u)
        if not (F(0.0) <= disp < maxD):
            continue
        if disp <= 0:
            u = F(uL - F(0.01))
        uR[i], sd[i] = u, d[kb]
    acc = np.nonzero(uR >= 0)[0]
    keep = median_cut(sd[acc])
    uR[acc[~keep]] = F(-1.0)
    sd[acc[~keep]] = -1
    return (uR, sd, patches, jbest) if return_j else (uR, sd, patches)


def track(kP, dP, uR, patches, kC, dC, levC, th_track=TH_TRACK, ratio=RATIO, radius=0.0, scale_factor=1.2):
    """Stage T.  Returns (t1_left, t1_right, t2_left (m, 2) float32, idx_prev, idx_cur int32 (m,))."""
    sc, inv = scales(scale_factor, len(levC))
    ratio, radius = F(ratio), F(radius)
    xC, yC, oC = kC["x"].astype(F), kC["y"].astype(F), kC["octave"].astype(np.int64)
    jj = np.arange(len(kC))
    kept = {}                                       # i -> (b, j)
    for i in range(len(kP)):
        if not uR[i] >= 0 or len(kC) == 0:
            continue
        cand = np.abs(oC - int(kP["octave"][i])) <= 1
        if radius > 0:
            cand &= (np.abs((xC - F(kP["x"][i])).astype(F)) <= radius) & (np.abs((yC - F(kP["y"][i])).astype(F)) <= radius)
        if not cand.any():
            continue
        dist = hamming(dP[i], dC[cand]).astype(np.int64)
        keys = np.sort((dist << 16) | jj[cand])
        b, j = int(keys[0]) >> 16, int(keys[0]) & 0xFFFF
        if b > th_track:
            continue
        if len(keys) > 1 and not F(b) < F(ratio * F(int(keys[1]) >> 16)):
            continue
        kept[i] = (b, j)
    winner = {}
    for i, (b, j) in kept.items():                  # ascending i: a tie keeps the lowest i
        if j not in winner or b < winner[j][0]:
            winner[j] = (b, i)
    out = []
    for i in sorted(kept):
        b, j = kept[i]
        if winner[j][1] != i:
            continue
        o = int(kP["octave"][i])
        J = levC[o]
        h, w = J.shape
        cu, cv = rnd(xC[j] * inv[o]), rnd(yC[j] * inv[o])
        if not (7 <= cu < w - 7 and 7 <= cv < h - 7):
            continue
        patch = patches[i].reshape(11, 11)
        D = np.array([[sad(patch, J, cu + dx, cv + dy) for dx in range(-2, 3)] for dy in range(-2, 3)])
        by, bx = divmod(int(np.argmin(D)), 5)       # first minimum in raster order
        if by in (0, 4) or bx in (0, 4):
            continue
        ddx = parabola(D[by, bx - 1], D[by, bx], D[by, bx + 1])
        ddy = parabola(D[by - 1, bx], D[by, bx], D[by + 1, bx])
        t2 = (F(sc[o] * F(F(F(cu) + F(bx - 2)) + ddx)), F(sc[o] * F(F(F(cv) + F(by - 2)) + ddy)))
        out.append((i, j, t2))
    m = len(out)
    t1l, t1r, t2l = np.zeros((m, 2), F), np.zeros((m, 2), F), np.zeros((m, 2), F)
    ip, ic = np.zeros(m, np.int32), np.zeros(m, np.int32)
    for k, (i, j, t2) in enumerate(out):
        t1l[k] = (kP["x"][i], kP["y"][i])
        t1r[k] = (uR[i], kP["y"][i])
        t2l[k] = t2
        ip[k], ic[k] = i, j
    return t1l, t1r, t2l, ip, ic


def levels_of(oracle, img, scale_factor=1.2, nlevels=8):
    return [oracle.orb_pyramid_level(img, l, scale_factor=scale_factor, nlevels=nlevels) for l in range(nlevels)]


def frame_stereo(oracle, left, right, max_disparity, th_stereo=TH_STEREO, orb=None):
    """Extraction + stage S of one frame: dict with the left / right features, the left levels and stage S's outputs.
    orb: oracle.orb_extract keywords (nfeatures, scale_factor, nlevels, ini_th, min_th) of a non-default extractor."""
    orb = dict(orb or {})
    sf, nl = orb.get("scale_factor", 1.2), orb.get("nlevels", 8)
    kL, dL, _ = oracle.orb_extract(left, **orb)
    kR, dR, _ = oracle.orb_extract(right, **orb)
    levL, levR = levels_of(oracle, left, sf, nl), levels_of(oracle, right, sf, nl)
    uR, sd, patches, j = stereo(kL, dL, kR, dR, levL, levR, max_disparity, th_stereo, scale_factor=sf, return_j=True)
    return dict(kL=kL, dL=dL, kR=kR, dR=dR, levL=levL, levR=levR, uR=uR, sad=sd, patches=patches, j=j, scale_factor=sf)


def pair_tracks(prev, cur, **kw):
    kw.setdefault("scale_factor", cur.get("scale_factor", 1.2))
    return track(prev["kL"], prev["dL"], prev["uR"], prev["patches"], cur["kL"], cur["dL"], cur["levL"], **kw)


def ref_sequence(oracle, seq, frames, minmove=0.05, maxmove=10.0, num_features_tracking=5, inlier_rate=0.01, pose0=None,
                 first_has_stereo=True, orb=None, **kw):
    """The fused ORB step with the guided matcher, frame by frame: twin -> oracle.triangulate -> oracle.pnp_ransac ->
    oracle.gate_and_accumulate.  Returns ([(record dict, pose)], [per-frame stage S dicts])."""
    P1, P2 = seq.proj()
    K = np.asarray(P1, np.float64).reshape(3, 4)[:, :3]
    maxd = kw.pop("max_disparity", 0.0) or float(F(np.asarray(P1, np.float64).reshape(-1)[0]))
    th_stereo = kw.pop("th_stereo", TH_STEREO)
    fr = [frame_stereo(oracle, L, R, maxd, th_stereo, orb) for L, R in frames]
    pose = np.eye(4) if pose0 is None else np.asarray(pose0, np.float64).reshape(4, 4).copy()
    out = []
    for t in range(1, len(frames)):
        prev, cur = fr[t - 1], fr[t]
        if t == 1 and not first_has_stereo:
            prev = dict(prev, uR=np.full(len(prev["kL"]), -1.0, F))
        t1l, t1r, t2l, _, _ = pair_tracks(prev, cur, **kw)
        r = dict(ok=0, fail_stage=0, n_prev_kps=len(prev["kL"]), n_cur_kps=len(cur["kL"]), n_tracked=len(t1l), n_inliers=0,
                 R=np.zeros((3, 3)), tvec=np.zeros(3), tracks=(t1l, t1r, t2l))
        if len(t1l) < num_features_tracking:
            r["fail_stage"] = 2
        else:
            X = oracle.triangulate(P1, P2, t1l, t1r)
            p = oracle.pnp_ransac(X, t2l, K)
            r.update(n_inliers=p["n_inliers"], R=p["R"], tvec=p["tvec"], ransac_iters=p["ransac_iters"])
            if p["n_inliers"] / len(t1l) < inlier_rate:
                r["fail_stage"] = 3
            else:
                g, new_pose, _ = oracle.gate_and_accumulate(p["R"], p["tvec"], pose, min_t2=minmove ** 2, max_t2=maxmove ** 2)
                if g < 0:
                    r["fail_stage"] = -g
                else:
                    r["ok"] = 1
                    pose = new_pose
        out.append((r, pose.copy()))
    return out, fr
