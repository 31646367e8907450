"""Inputs of the guided ORB matcher's edge tests (tests/test_orbmatch_ref.py proves on the CPU that each one reaches the path it
is named after; tests/test_gpu_orbmatch_edges.py runs them on the GPU): deterministic builders, numpy only.

An exact integer shift of a one-level image gives SAD 0 at every keypoint, the median is 0 and the cut drops every match (that
is median_pair's purpose) -- so every other case adds a little noise to the shifted image."""
import numpy as np

from conftest import rand_image

# extractor settings (oracle.orb_extract keywords) of the cases that leave the defaults
CHUNK_ORB = dict(nlevels=1, scale_factor=1.2, nfeatures=3000, ini_th=9, min_th=5)
CHUNK3_ORB = dict(nlevels=3, scale_factor=1.2, nfeatures=4000, ini_th=9, min_th=5)
CHUNK_MAXD = 100.0
TILED_MAXD = 90.0
SCALE_ORBS = {
    "5x1.5": dict(nlevels=5, scale_factor=1.5, nfeatures=1200, ini_th=30, min_th=10),
    "8x1.1": dict(nlevels=8, scale_factor=1.1, nfeatures=300, ini_th=12, min_th=12),
    "1": dict(nlevels=1, nfeatures=800),
    "2x2.0": dict(nlevels=2, scale_factor=2.0, nfeatures=600),
}
# (th_stereo, max_disparity) of stage S and set_orb_matcher keywords of stage T on shift_pair, beside the defaults
STEREO_SETTINGS = [(30, 300.0), (256, 300.0), (1, 300.0), (75, 12.5), (75, 11.0)]
STEREO_DEFAULT = (75, 300.0)
TRACK_SETTINGS = [dict(th_track=30), dict(th_track=256, ratio=1.0), dict(ratio=0.5), dict(radius=3.0), dict(radius=1.0),
                  dict(radius=0.5), dict(radius=4.0, ratio=1.0)]


class Rig:
    """seq.proj() of a plain rectified rig (principal point at the image centre) for the pairs that come from no renderer."""

    def __init__(self, w, h, f=718.856, base=0.537):
        self.P1 = [f, 0.0, 0.5 * w, 0.0, 0.0, f, 0.5 * h, 0.0, 0.0, 0.0, 1.0, 0.0]
        self.P2 = [f, 0.0, 0.5 * w, -f * base, 0.0, f, 0.5 * h, 0.0, 0.0, 0.0, 1.0, 0.0]

    def proj(self):
        return self.P1, self.P2


def ctx_orb(orb):
    """The svo_config fields of an oracle.orb_extract keyword dict."""
    return {"orb_" + k: v for k, v in orb.items()}


def noisy(img, seed, amp=3):
    rng = np.random.default_rng(seed)
    return np.clip(img.astype(np.int64) + rng.integers(-amp, amp + 1, img.shape), 0, 255).astype(np.uint8)


def _c(*imgs):
    return tuple(np.ascontiguousarray(x) for x in imgs)


def chunk_pair():
    """Two 500 x 300 frames with more than 2048 keypoints per image under CHUNK_ORB / CHUNK3_ORB (max_disparity CHUNK_MAXD):
    stage S's second LDS chunk, and j >= 2048 in stage T's winner table, the sub-pixel kernel and the emit kernel."""
    big = rand_image(300, 520, 31)
    L, R = big[:, :500], noisy(big[:, 7:507], 1)
    L2 = big[2:, 3:503]
    L2 = noisy(np.concatenate([L2, L2[-1:], L2[-1:]], 0), 2)
    R2 = noisy(L2, 3)
    return [_c(L, R), _c(L2, R2)]


def shift_pair(seed=22, d=12):
    """Two 416 x 128 frames: the right image is the left one moved d pixels, the successor both moved by (2, -3) (rows, columns)."""
    big = rand_image(128, 440, seed)
    L, R = big[:, :416], noisy(big[:, d:d + 416], 5)
    L2, R2 = noisy(np.roll(L, (2, -3), (0, 1)), 6), noisy(np.roll(R, (2, -3), (0, 1)), 7)
    return [_c(L, R), _c(L2, R2)]


def tiled_pair():
    """Two frames tiled from one 96-pixel-wide block (max_disparity TILED_MAXD): descriptors repeat every 96 pixels, so several
    previous keypoints claim one current keypoint, often at the same distance."""
    block = rand_image(128, 96, 21)
    big = np.tile(block, (1, 6))
    L, R = big[:, :416], noisy(big[:, 9:425], 8)
    return [_c(L, R), _c(noisy(L, 9, 1), noisy(R, 10, 1))]


def median_pair():
    """An identical pair: on a one-level pyramid every accepted SAD is 0, the median is 0 and the cut drops every match."""
    img = rand_image(128, 416, 21)
    return _c(img, img.copy())


def clamp_pair():
    """A pair (zero shift plus noise) on which stage S's disp == 0 branch (uR = uL - 0.01f) fires."""
    img = rand_image(128, 416, 21)
    return _c(img, noisy(img, 4))


def flat_sequence(frames, value=60):
    """[f0, f1, (flat, flat), f2, (f3.left, flat), f3] of four frames: empty keypoint lists beside full ones."""
    flat = np.full_like(frames[0][0], value)
    f0, f1, f2, f3 = frames[:4]
    return [f0, f1, (flat, flat), f2, (f3[0], flat.copy()), f3]


PAIRS = {"chunk": (chunk_pair, CHUNK_MAXD), "shift": (shift_pair, 300.0), "tiled": (tiled_pair, TILED_MAXD)}
_CACHE = {}


def cached(key, make):
    """make() once per session under `key`: the CPU and the GPU tests share the twin's outputs and leave them unchanged."""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def frames_of(name):
    return cached(("frames", name), PAIRS[name][0])


def twin(oracle, name, orb=None):
    """The twin's stage S (frame_stereo dicts) of both frames of a named pair at th_stereo 75 and the pair's max_disparity."""
    import _orbmatch_ref as M
    key = ("twin", name, tuple(sorted((orb or {}).items())))
    return cached(key, lambda: [M.frame_stereo(oracle, L, R, PAIRS[name][1], orb=orb) for L, R in frames_of(name)])


def restereo(fr, max_disparity, th_stereo):
    """Stage S again on a frame_stereo dict's features with other settings: a new dict, the old one untouched."""
    import _orbmatch_ref as M
    uR, sd, patches, j = M.stereo(fr["kL"], fr["dL"], fr["kR"], fr["dR"], fr["levL"], fr["levR"], max_disparity, th_stereo,
                                  scale_factor=fr["scale_factor"], return_j=True)
    return dict(fr, uR=uR, sad=sd, patches=patches, j=j)


def flat_ref(oracle, seq, frames):
    """The twin's records and stage S of flat_sequence(frames) (M.ref_sequence's return value)."""
    import _orbmatch_ref as M
    return cached("flat", lambda: M.ref_sequence(oracle, seq, flat_sequence(frames)))


def small_ref(oracle, seq, frames):
    """The twin's records and stage S of the session's small sequence."""
    import _orbmatch_ref as M
    return cached("small", lambda: M.ref_sequence(oracle, seq, frames))


def accepted(fr):
    return int((fr["uR"] >= 0).sum())


def stereo_best(fr):
    """The best Hamming distance of every accepted left keypoint of a frame_stereo dict."""
    import _orbmatch_ref as M
    return np.array([M.hamming(fr["dL"][i], fr["dR"][fr["j"][i]][None, :])[0] for i in np.nonzero(fr["uR"] >= 0)[0]], np.int64)


def track_best(prev, cur, tracks):
    """The Hamming distance of every track (idx_prev, idx_cur) of a pair."""
    import _orbmatch_ref as M
    return np.array([M.hamming(prev["dL"][i], cur["dL"][j][None, :])[0] for i, j in zip(tracks[3], tracks[4])], np.int64)


def stereo_candidates(fr, max_disparity):
    """Per left keypoint of a frame_stereo dict: stage S's candidate counts among the right keypoints below index 2048 (the
    kernel's first LDS chunk) and from it on, as two arrays."""
    import _orbmatch_ref as M
    sc, _ = M.scales(fr["scale_factor"], len(fr["levL"]))
    F = np.float32
    kL, kR = fr["kL"], fr["kR"]
    xR, yR, oR = kR["x"].astype(F), kR["y"].astype(F), kR["octave"].astype(np.int64)
    rj = (F(2.0) * sc[oR]).astype(F)
    lo, hi = np.floor((yR - rj).astype(F)), np.ceil((yR + rj).astype(F))
    below, above = np.zeros(len(kL), np.int64), np.zeros(len(kL), np.int64)
    for i in range(len(kL)):
        uL, tv, oL = F(kL["x"][i]), np.trunc(F(kL["y"][i])), int(kL["octave"][i])
        cand = (lo <= tv) & (tv <= hi) & (np.abs(oR - oL) <= 1) & (F(uL - F(max_disparity)) <= xR) & (xR <= uL)
        below[i], above[i] = cand[:2048].sum(), cand[2048:].sum()
    return below, above


def track_candidates(prev, cur, radius):
    """Per previous keypoint with a stereo match: the number of stage T candidates at `radius` (> 0)."""
    F = np.float32
    kP, kC = prev["kL"], cur["kL"]
    xC, yC, oC = kC["x"].astype(F), kC["y"].astype(F), kC["octave"].astype(np.int64)
    out = []
    for i in np.nonzero(prev["uR"] >= 0)[0]:
        c = np.abs(oC - int(kP["octave"][i])) <= 1
        c &= (np.abs((xC - F(kP["x"][i])).astype(F)) <= F(radius)) & (np.abs((yC - F(kP["y"][i])).astype(F)) <= F(radius))
        out.append(int(c.sum()))
    return np.array(out, np.int64)


def contested(prev, cur, **kw):
    """Stage T's contention on a pair: (number of current keypoints kept by more than one previous keypoint, number of those whose
    two smallest kept distances are equal).  Restates the twin's first pass."""
    import _orbmatch_ref as M
    F = np.float32
    th_track, ratio, radius = kw.get("th_track", M.TH_TRACK), F(kw.get("ratio", M.RATIO)), F(kw.get("radius", 0.0))
    kP, dP, kC, dC = prev["kL"], prev["dL"], cur["kL"], cur["dL"]
    xC, yC, oC = kC["x"].astype(F), kC["y"].astype(F), kC["octave"].astype(np.int64)
    claims = {}
    for i in np.nonzero(prev["uR"] >= 0)[0]:
        cand = np.abs(oC - int(kP["octave"][i])) <= 1
        if radius > 0:
            cand &= (np.abs((xC - F(kP["x"][i])).astype(F)) <= radius) & (np.abs((yC - F(kP["y"][i])).astype(F)) <= radius)
        if not cand.any():
            continue
        keys = np.sort((M.hamming(dP[i], dC[cand]).astype(np.int64) << 16) | np.nonzero(cand)[0])
        b, j = int(keys[0]) >> 16, int(keys[0]) & 0xFFFF
        if b > th_track or (len(keys) > 1 and not F(b) < F(ratio * F(int(keys[1]) >> 16))):
            continue
        claims.setdefault(j, []).append(b)
    multi = [sorted(v) for v in claims.values() if len(v) > 1]
    return len(multi), sum(v[0] == v[1] for v in multi)
