"""CPU test: every rule of the keyframe twin (tests/_keyframe_ref.py, rules K1-K7 of include/svo_abi.h) on hand-built cases.
The solve is a stub that returns a prepared record, so each gate is reached on purpose."""
import numpy as np
import pytest

import _keyframe_ref as KR


def _X(n, seed=0):
    return np.random.default_rng(seed).random((n, 3)).astype(np.float32) * 10


def _xy(n, seed=1):
    return np.random.default_rng(seed).random((n, 2)).astype(np.float32) * 100


# ---- K2 ------------------------------------------------------------------------------------------------------------------------
def test_join_disjoint_identical_interleaved():
    X, xy = _X(6), _xy(6)
    ids = np.arange(6, dtype=np.int64) * 2
    j = KR.join(ids, X, ids + 1, xy)                                 # disjoint
    assert all(len(j[k]) == 0 for k in ("ids", "X", "xy", "trk", "row"))
    j = KR.join(ids, X, ids, xy)                                     # identical
    assert j["trk"].tolist() == j["row"].tolist() == list(range(6)) and j["X"].tobytes() == X.tobytes() and j["xy"].tobytes() == xy.tobytes()
    trk = np.array([-3, 0, 1, 4, 5, 10, 11, 99], np.int64)           # interleaved: rows 0, 2, 5 are hit by tracks 1, 3, 5
    j = KR.join(ids, X, trk, _xy(8))
    assert j["trk"].tolist() == [1, 3, 5] and j["row"].tolist() == [0, 2, 5] and j["ids"].tolist() == [0, 4, 10]
    assert j["X"].tobytes() == X[[0, 2, 5]].tobytes() and j["xy"].tobytes() == _xy(8)[[1, 3, 5]].tobytes()
    assert j["trk"].dtype == j["row"].dtype == np.int32 and j["X"].dtype == j["xy"].dtype == np.float32
    for a, b in ((ids[:0], ids), (ids, ids[:0]), (ids[:0], ids[:0])):   # an empty side
        assert len(KR.join(a, _X(len(a)), b, _xy(len(b)))["trk"]) == 0


def test_join_compares_64_bits():
    big = 1 << 32
    ids = np.array([5, big + 5, 2 * big + 5, (1 << 40) + 5], np.int64)    # equal in their low 32 bits
    j = KR.join(ids, _X(4), np.array([5, 2 * big + 5, 3 * big + 5], np.int64), _xy(3))
    assert j["trk"].tolist() == [0, 1] and j["row"].tolist() == [0, 2]
    j = KR.join(ids, _X(4), np.array([(1 << 40) + 5], np.int64), _xy(1))
    assert j["row"].tolist() == [3]


# ---- the chain: a camera that moves 1 m forward per frame -----------------------------------------------------------------------
def _pose(z, ry=0.0):
    P = np.eye(4)
    c, s = np.cos(ry), np.sin(ry)
    P[:3, :3] = [[c, 0, s], [0, 1, 0], [-s, 0, c]]
    P[2, 3] = z
    return P


def _true_solve(pose_K, pose_b, **kw):
    """the record a perfect solve gives: [R t] = inverse(pose_b) pose_K"""
    M = np.linalg.inv(pose_b) @ pose_K
    d = dict(ok=1, R=M[:3, :3].copy(), tvec=M[:3, 3].copy(), rvec=np.array([0.1, 0.2, 0.3]), n_inliers=5, ransac_iters=7, lm_iters=3, mask=None)
    d.update(kw)
    return d


class _Stub:
    def __init__(self):
        self.next, self.calls = None, []

    def __call__(self, X, xy):
        self.calls.append((X.copy(), xy.copy()))
        d = dict(self.next)
        if d["mask"] is None:
            d["mask"] = np.ones(len(X), np.uint8)
        return d


def _chain(min_tracks=4, max_gap=0, inlier_rate=0.01):
    stub = _Stub()
    return KR.Chain(min_tracks, max_gap, inlier_rate, 100.0, stub), stub


IDS = np.arange(10, dtype=np.int64) + (1 << 33)


def _first(ch, tri=None):
    """step 0 -> 1 of a fresh chain: no keyframe yet, frame 0 becomes it"""
    tri = _X(10) if tri is None else tri
    r = ch.step(1, 1, _pose(1), _pose(0), IDS, _xy(10), tri)
    assert r["status"] == KR.NONE and r["switched"] == 1 and r["kf_index"] == -1 and r["gap"] == 0 and r["n_rows"] == 0 and r["n_join"] == 0
    assert np.array_equal(r["pose"], _pose(1)) and not r["pose_K"].any()
    return tri


def test_first_step_takes_frame_a_and_drops_non_finite_points():
    ch, stub = _chain()
    tri = _X(10)
    tri[3, 1], tri[7, 2] = np.nan, np.inf
    _first(ch, tri)                                                  # K6, cause 1: the state was not valid
    assert ch.valid and ch.kf_index == 0 and np.array_equal(ch.pose_K, _pose(0)) and not stub.calls
    keep = [0, 1, 2, 4, 5, 6, 8, 9]
    assert ch.ids.tolist() == IDS[keep].tolist() and ch.X.tobytes() == tri[keep].tobytes()


def test_short_one_below_min_tracks_and_solve_at_min_tracks():
    for n_common, want in ((3, KR.SHORT), (4, KR.APPLIED)):
        ch, stub = _chain(min_tracks=4)
        tri = _first(ch)
        ids = np.concatenate([IDS[:n_common], IDS[-1:] + 1 + np.arange(3)])
        stub.next = _true_solve(_pose(0), _pose(2), n_inliers=n_common)
        r = ch.step(2, 1, _pose(2.5), _pose(1), ids, _xy(len(ids), 3), _X(len(ids), 4))
        assert r["status"] == want and r["n_join"] == n_common and r["gap"] == 2 and r["kf_index"] == 0 and r["n_rows"] == 10
        if want == KR.SHORT:
            assert not stub.calls and r["switched"] == 1 and r["n_inliers"] == 0 and not r["rvec"].any() and not r["mask"].any()
            assert np.array_equal(r["pose"], _pose(2.5)) and ch.kf_index == 1 and ch.ids.tolist() == ids.tolist()     # K6, cause 2
        else:
            assert len(stub.calls) == 1 and stub.calls[0][0].tobytes() == tri[:4].tobytes() and stub.calls[0][1].tobytes() == _xy(len(ids), 3)[:4].tobytes()
            assert r["switched"] == 0 and r["n_inliers"] == 4 and r["ransac_iters"] == 7 and r["lm_iters"] == 3 and r["mask"].all()
            assert np.abs(r["pose"] - _pose(2)).max() < 1e-12 and np.array_equal(r["pose_pair"], _pose(2.5))
            assert ch.kf_index == 0 and ch.ids.tolist() == IDS.tolist()                                               # the keyframe stays


@pytest.mark.parametrize("why", ["solve_failed", "inlier_rate", "rotation", "translation"])
def test_rejected_by_each_gate(why):
    ch, stub = _chain(inlier_rate=0.5)
    _first(ch)
    good = _true_solve(_pose(0), _pose(2))                          # 5 inliers of 10: exactly at the rate, accepted
    stub.next = {"solve_failed": dict(good, ok=0), "inlier_rate": dict(good, n_inliers=4),
                 "rotation": _true_solve(_pose(0), _pose(2, ry=0.12)), "translation": _true_solve(_pose(0), _pose(12))}[why]
    r = ch.step(2, 1, _pose(2.25), _pose(1), IDS, _xy(10), _X(10, 5))
    assert r["status"] == KR.REJECTED and r["n_join"] == 10 and len(stub.calls) == 1
    assert np.array_equal(r["pose"], _pose(2.25))                    # the record is untouched
    assert r["switched"] == 1 and ch.kf_index == 1 and np.array_equal(ch.pose_K, _pose(1)) and ch.X.tobytes() == _X(10, 5).tobytes()
    # ... and each prepared record fails one gate only: the same record without its defect is applied
    ch2, stub2 = _chain(inlier_rate=0.5)
    _first(ch2)
    stub2.next = good
    assert ch2.step(2, 1, _pose(2.25), _pose(1), IDS, _xy(10), _X(10, 5))["status"] == KR.APPLIED
    if why == "rotation":                                           # 0.12 rad is the implied motion's angle, not the solve's alone
        F = KR.implied_motion(stub.next["R"], stub.next["tvec"], KR.inv_t4(_pose(0)), _pose(1))
        assert abs(float(KR.euler(F[:3, :3])[1])) > 0.1 and KR.gates(F, 1e9) is False
    if why == "translation":                                        # 11 m from a: above max_move2 = 100; there is no lower bound
        F = KR.implied_motion(stub.next["R"], stub.next["tvec"], KR.inv_t4(_pose(0)), _pose(1))
        assert abs(F[2, 3] + 11) < 1e-12 and KR.gates(KR.implied_motion(np.eye(3), np.zeros(3), np.eye(4), np.eye(4)), 100.0)


def test_switch_by_max_gap():
    ch, stub = _chain(max_gap=3)
    _first(ch)
    for b in (2, 3, 4):
        stub.next = _true_solve(ch.pose_K, _pose(b))
        r = ch.step(b, 1, _pose(b + 0.5), _pose(b - 1), IDS, _xy(10), _X(10, b))
        assert r["status"] == KR.APPLIED and np.abs(r["pose"] - _pose(b)).max() < 1e-12
        if b < 4:
            assert (r["gap"], r["switched"], ch.kf_index) == ([2, 3][b - 2], [0, 1][b - 2], [0, 2][b - 2])          # K6, cause 3 at gap 3
        else:
            assert (r["gap"], r["kf_index"], r["switched"]) == (2, 2, 0) and np.array_equal(r["pose_K"], _pose(2))
    assert ch.X.tobytes() == _X(10, 3).tobytes()                    # the table is the switching pair's
    ch0, stub0 = _chain(max_gap=0)                                   # 0: no limit
    _first(ch0)
    for b in range(2, 12):
        stub0.next = _true_solve(ch0.pose_K, _pose(b))
        assert ch0.step(b, 1, _pose(b), _pose(b - 1), IDS, _xy(10), _X(10))["switched"] == 0
    assert ch0.kf_index == 0


def test_failed_pair_keeps_the_state():
    ch, stub = _chain()
    tri = _first(ch)
    stub.next = _true_solve(_pose(0), _pose(2))
    r = ch.step(2, 0, _pose(1), _pose(1), IDS, _xy(10), _X(10, 9))   # K7: joined, solved, reported, not used
    assert r["status"] == KR.PAIR_FAILED and r["switched"] == 0 and r["n_join"] == 10 and r["n_inliers"] == 5 and len(stub.calls) == 1
    assert np.array_equal(r["pose"], _pose(1)) and ch.valid and ch.kf_index == 0 and ch.X.tobytes() == tri.tobytes()
    r = ch.step(3, 0, _pose(1), _pose(1), IDS[:2], _xy(2), _X(2))     # a failed step that is short as well: SHORT, and still no switch
    assert r["status"] == KR.SHORT and r["switched"] == 0 and ch.kf_index == 0
    stub.next = _true_solve(_pose(0), _pose(4))
    r = ch.step(4, 1, _pose(2), _pose(1), IDS, _xy(10), _X(10))       # the gap has simply grown
    assert r["status"] == KR.REJECTED or r["status"] == KR.APPLIED
    assert r["gap"] == 4 and r["kf_index"] == 0
    ch.clear()                                                       # K1
    assert not ch.valid and ch.step(5, 0, _pose(1), _pose(1), IDS, _xy(10), _X(10))["status"] == KR.NONE and not ch.valid


def test_composition_equals_a_plain_numpy_product():
    rng = np.random.default_rng(3)

    def rot(v):
        th = np.linalg.norm(v)
        k = v / th
        Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx

    for _ in range(20):
        pose_K, pose_a = np.eye(4), np.eye(4)
        pose_K[:3, :3], pose_K[:3, 3] = rot(rng.normal(size=3)), rng.normal(size=3) * 50
        pose_a[:3, :3], pose_a[:3, 3] = rot(rng.normal(size=3)), rng.normal(size=3) * 50
        M = np.eye(4)
        M[:3, :3], M[:3, 3] = rot(rng.normal(size=3) * 0.1), rng.normal(size=3)
        scale = max(1.0, np.abs(pose_K).max())
        assert np.abs(KR.mul4(pose_K, KR.inv_rt(M[:3, :3], M[:3, 3])) - pose_K @ np.linalg.inv(M)).max() <= 1e-12              # K5
        assert np.abs(KR.inv_t4(pose_K) - np.linalg.inv(pose_K)).max() <= 1e-12 * scale                                      # T4
        F = KR.implied_motion(M[:3, :3], M[:3, 3], KR.inv_t4(pose_K), pose_a)
        assert np.abs(F - M @ np.linalg.inv(pose_K) @ pose_a).max() <= 1e-12 * scale * scale                                 # K4
