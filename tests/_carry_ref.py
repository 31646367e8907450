"""numpy twin of track carry (svo_set_track_carry / svo_carry_merge): rules C1-C5 of include/svo_abi.h on plain arrays, and
the frame-to-frame chain (C5-C8) on keypoint records.  The HIP kernel must equal it bit for bit."""
import numpy as np

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"),
                     ("class_id", "<i4")])


def near_matrix(a, b, min_distance):
    """near(a[i], b[j]) for (n, 2) / (m, 2) float32 arrays (C2): dx, dy in float32, the squares and their sum in double."""
    a = np.asarray(a, np.float32).reshape(-1, 2)
    b = np.asarray(b, np.float32).reshape(-1, 2)
    with np.errstate(invalid="ignore", over="ignore"):
        dx = (a[:, None, 0] - b[None, :, 0]).astype(np.float32).astype(np.float64)
        dy = (a[:, None, 1] - b[None, :, 1]).astype(np.float32).astype(np.float64)
        d2 = dx * dx + dy * dy
        return d2 < float(min_distance) * float(min_distance)


def near(a, b, min_distance):
    return bool(near_matrix([a], [b], min_distance)[0, 0])


def candidates(w, h, max_age, q, age, keep):
    """C1: the candidate mask over the tracks."""
    q = np.asarray(q, np.float32).reshape(-1, 2)
    age = np.asarray(age, np.int64)
    with np.errstate(invalid="ignore"):
        inside = (np.isfinite(q).all(1) & (q[:, 0] >= np.float32(0)) & (q[:, 0] <= np.float32(w - 1)) &
                  (q[:, 1] >= np.float32(0)) & (q[:, 1] <= np.float32(h - 1)))
    young = np.ones(len(q), bool) if max_age == 0 else age + 1 <= max_age
    return (np.asarray(keep) != 0) & inside & young


def merge(w, h, min_distance, max_age, trk_xy, trk_resp, trk_id, trk_age, trk_keep, det_xy, det_resp, next_id, cap):
    """One pair.  Returns dict(xy, resp, id, age, src, n_carried, next_id): the new list (src: the track index, or n_trk + the
    detection index), the carried count and the counter afterwards."""
    q = np.asarray(trk_xy, np.float32).reshape(-1, 2)
    d = np.asarray(det_xy, np.float32).reshape(-1, 2)
    n_trk, n_det = len(q), len(d)
    assert cap >= n_trk
    cand = np.flatnonzero(candidates(w, h, max_age, q, trk_age, trk_keep))
    # C3: no EARLIER candidate near, carried or not
    nm = near_matrix(q[cand], q[cand], min_distance)
    carried = cand[~np.tril(nm, -1).any(1)] if len(cand) else cand
    # C4: detections against the carried points only
    kept = np.flatnonzero(~near_matrix(d, q[carried], min_distance).any(1)) if n_det else np.zeros(0, np.int64)
    kept = kept[:cap - len(carried)]                                # only trailing detections fall off
    n_c, n_k = len(carried), len(kept)
    out = dict(
        xy=np.concatenate([q[carried], d[kept]]).astype(np.float32).reshape(-1, 2),
        resp=np.concatenate([np.asarray(trk_resp, np.float32).reshape(-1)[carried], np.asarray(det_resp, np.float32).reshape(-1)[kept]]),
        id=np.concatenate([np.asarray(trk_id, np.int64).reshape(-1)[carried], next_id + np.arange(n_k, dtype=np.int64)]),
        age=np.concatenate([np.asarray(trk_age, np.int32).reshape(-1)[carried] + 1, np.zeros(n_k, np.int32)]).astype(np.int32),
        src=np.concatenate([carried, n_trk + kept]).astype(np.int32),
        n_carried=n_c, next_id=int(next_id) + n_k)
    return out


class Chain:
    """A stream's (or the online ring's) list from frame to frame.  Records are KP_DTYPE arrays; `cap` is max_keypoints."""

    def __init__(self, w, h, min_distance=3.0, max_age=0, cap=8192):
        self.w, self.h, self.md, self.max_age, self.cap = w, h, float(min_distance), int(max_age), int(cap)
        self.reset()

    def reset(self):
        self.next_id = 0
        self.kps = self.ids = self.ages = None

    def store_plain(self, kps):
        """a frame stored while carry was off: a list without ids (C6)"""
        self.kps, self.ids, self.ages = np.asarray(kps, KP_DTYPE).copy(), None, None

    def number(self):
        """C6: a list without ids is numbered in list order, age 0, by the step that first sees it"""
        if self.ids is None:
            n = len(self.kps)
            self.ids = self.next_id + np.arange(n, dtype=np.int64)
            self.ages = np.zeros(n, np.int32)
            self.next_id += n

    def first(self, det):
        """a chain's first frame: its detections (none when the detector overflowed, C7), numbered"""
        det = np.asarray(det, KP_DTYPE)
        self.kps = det[:0].copy() if len(det) > self.cap else det.copy()
        self.ids = None
        self.number()

    def step(self, q, keep, det):
        """one pair: q / keep per entry of the current list, det = the new frame's detections.  Returns the track ids / ages
        at t1 in compaction order; the list becomes the new frame's."""
        self.number()
        det = np.asarray(det, KP_DTYPE)
        if len(det) > self.cap:
            det = det[:0]
        keep = np.asarray(keep) != 0
        trk = (self.ids[keep].copy(), self.ages[keep].copy())
        dxy = np.stack([det["x"], det["y"]], 1) if len(det) else np.zeros((0, 2), np.float32)
        m = merge(self.w, self.h, self.md, self.max_age, q, self.kps["response"], self.ids, self.ages, keep, dxy, det["response"],
                  self.next_id, self.cap)
        n_trk = len(self.kps)
        new = np.zeros(len(m["src"]), KP_DTYPE)
        from_trk = m["src"] < n_trk
        new[from_trk] = self.kps[m["src"][from_trk]]
        new[~from_trk] = det[m["src"][~from_trk] - n_trk]
        new["x"], new["y"] = m["xy"][:, 0], m["xy"][:, 1]
        self.kps, self.ids, self.ages, self.next_id = new, m["id"], m["age"], m["next_id"]
        return trk
