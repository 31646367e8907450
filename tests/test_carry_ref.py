"""CPU test: properties of the numpy twin of track carry (tests/_carry_ref.py) -- the rules the HIP kernel is held to."""
import numpy as np
import pytest

import _carry_ref as CR

W, H = 512, 264


def _case(seed, n_trk, n_det, spread=1.0):
    rng = np.random.default_rng(seed)
    q = (rng.random((n_trk, 2)) * [W * spread, H * spread]).astype(np.float32)
    ids = np.sort(rng.choice(10 * n_trk + 10, n_trk, replace=False)).astype(np.int64)
    ages = rng.integers(0, 6, n_trk).astype(np.int32)
    keep = (rng.random(n_trk) < 0.8).astype(np.uint8)
    det = np.stack([rng.integers(0, W, n_det), rng.integers(0, H, n_det)], 1).astype(np.float32)
    return dict(q=q, resp=rng.integers(1, 255, n_trk).astype(np.float32), ids=ids, ages=ages, keep=keep, det=det,
                dresp=rng.integers(1, 255, n_det).astype(np.float32), next_id=int(ids.max(initial=0)) + 1)


def _merge(c, md, max_age=0, cap=None):
    cap = len(c["q"]) + len(c["det"]) if cap is None else cap
    return CR.merge(W, H, md, max_age, c["q"], c["resp"], c["ids"], c["ages"], c["keep"], c["det"], c["dresp"], c["next_id"], cap)


@pytest.mark.parametrize("md", [1.0, 3.0, 20.5])
@pytest.mark.parametrize("seed", [1, 2])
def test_merged_list_properties(seed, md):
    c = _case(seed, 700, 900)
    m = _merge(c, md)
    n_c, n_trk = m["n_carried"], len(c["q"])
    car, det = m["xy"][:n_c], m["xy"][n_c:]
    assert 0 < n_c < n_trk and len(det) > 0
    # no two carried points near each other; no listed detection near a carried point
    nm = CR.near_matrix(car, car, md)
    assert not (nm & ~np.eye(n_c, dtype=bool)).any()
    assert not CR.near_matrix(det, car, md).any()
    # every dropped detection IS near a carried point, every dropped candidate near an earlier candidate
    listed = m["src"][n_c:] - n_trk
    dropped = np.setdiff1d(np.arange(len(c["det"])), listed)
    assert CR.near_matrix(c["det"][dropped], car, md).any(1).all()
    # carried points keep id and order, ages + 1; the detections get the next ids in order, age 0
    src = m["src"][:n_c]
    assert (np.diff(src) > 0).all() and (c["keep"][src] != 0).all()
    assert np.array_equal(m["id"][:n_c], c["ids"][src]) and np.array_equal(m["age"][:n_c], c["ages"][src] + 1)
    assert np.array_equal(m["id"][n_c:], c["next_id"] + np.arange(len(det))) and not m["age"][n_c:].any()
    assert (np.diff(listed) > 0).all() and m["next_id"] == c["next_id"] + len(det)
    assert len(np.unique(m["id"])) == len(m["id"]) and (np.diff(m["id"]) > 0).all()
    assert m["xy"].dtype == np.float32 and m["id"].dtype == np.int64 and m["age"].dtype == np.int32


def test_chain_rule_keeps_only_the_oldest():
    """a ~ b, b ~ c, a !~ c: b falls to a, and c falls to b although b is not carried (C3 is an index rule)"""
    q = np.array([[10, 10], [12, 10], [14, 10]], np.float32)
    assert CR.near(q[0], q[1], 3.0) and CR.near(q[1], q[2], 3.0) and not CR.near(q[0], q[2], 3.0)
    m = CR.merge(W, H, 3.0, 0, q, [5, 6, 7], [40, 41, 42], [2, 1, 0], [1, 1, 1], np.zeros((0, 2)), [], 43, 8)
    assert m["n_carried"] == 1 and m["id"].tolist() == [40] and m["age"].tolist() == [3] and m["src"].tolist() == [0]
    # a greedy pass would have kept c: the rule drops a little more
    m = CR.merge(W, H, 3.0, 0, q, [5, 6, 7], [40, 41, 42], [2, 1, 0], [1, 0, 1], np.zeros((0, 2)), [], 43, 8)
    assert m["id"].tolist() == [40, 42]                                # b is no candidate now


def test_distance_boundary_is_strict():
    one_in = np.nextafter(np.float32(13.0), np.float32(0))
    q = np.array([[10, 10], [13, 10], [10, 20], [one_in, 20]], np.float32)
    m = CR.merge(W, H, 3.0, 0, q, np.ones(4), np.arange(4), np.zeros(4), np.ones(4), np.array([[10, 13], [10, 17.5]]), [9, 9], 4, 8)
    assert m["src"].tolist() == [0, 1, 2, 4]        # d2 == 9: kept; one ulp inside: dropped; detection at distance 3: kept, 2.5: dropped


def test_candidate_rules_and_truncation():
    q = np.array([[0, 0], [W - 1, H - 1], [W - 0.5, 5], [np.nan, 5], [5, np.inf], [-0.25, 5], [50, 50], [60, 60]], np.float32)
    ages = np.array([0, 2, 0, 0, 0, 0, 3, 0], np.int32)
    keep = np.array([1, 1, 1, 1, 1, 1, 1, 0], np.uint8)
    det = np.array([[100, 100], [101, 100], [200, 100]], np.float32)
    args = (q, np.ones(8), np.arange(8), ages, keep, det, [1, 2, 3], 8)
    assert CR.merge(W, H, 3.0, 0, *args, 11)["src"].tolist() == [0, 1, 6, 8, 9, 10]
    assert CR.merge(W, H, 3.0, 3, *args, 11)["src"].tolist() == [0, 1, 8, 9, 10]       # age 3 + 1 > 3
    assert CR.merge(W, H, 3.0, 1, *args, 11)["src"].tolist() == [0, 8, 9, 10]
    m = CR.merge(W, H, 3.0, 0, *args, 8)                                               # cap = n_trk: five detections' worth cut to five entries
    assert m["src"].tolist() == [0, 1, 6, 8, 9, 10][:8] and m["next_id"] == 11
    q2 = np.tile(np.array([[5, 5]], np.float32), (4, 1)) + np.arange(4, dtype=np.float32)[:, None] * 10
    m = CR.merge(W, H, 3.0, 0, q2, np.ones(4), np.arange(4), np.zeros(4), np.ones(4), det, [1, 2, 3], 4, 5)
    assert m["src"].tolist() == [0, 1, 2, 3, 4] and m["id"].tolist() == [0, 1, 2, 3, 4] and m["next_id"] == 5   # the cut detections get no id


def test_chain_numbers_reset_and_overflow():
    kp = lambda xs: np.array([(x, 7, 7, -1, 50, 0, -1) for x in xs], CR.KP_DTYPE)
    ch = CR.Chain(W, H, 3.0, 0, cap=4)
    ch.first(kp([10, 20, 30]))
    assert ch.ids.tolist() == [0, 1, 2] and not ch.ages.any()
    q = np.array([[10.5, 7], [200, 700], [30.25, 7]], np.float32)
    trk = ch.step(q, [1, 1, 1], kp([11, 100, 110, 120]))
    assert trk[0].tolist() == [0, 1, 2] and ch.ids.tolist() == [0, 2, 3, 4] and ch.ages.tolist() == [1, 1, 0, 0] and ch.next_id == 5
    assert ch.kps["x"].tolist() == [10.5, 30.25, 100, 110] and (ch.kps["response"] == 50).all()
    ch.step(np.zeros((4, 2), np.float32), [0, 0, 0, 0], kp([1, 2, 3, 4, 5]))            # C7: an overflowed detector
    assert len(ch.kps) == 0 and ch.next_id == 5
    ch.store_plain(kp([40, 50]))                                                       # C6: a frame from before the switch
    ch.step(np.array([[41, 7], [51, 7]], np.float32), [1, 1], kp([]))
    assert ch.ids.tolist() == [5, 6] and ch.ages.tolist() == [1, 1]
    ch.reset()
    ch.first(kp([10]))
    assert ch.ids.tolist() == [0]
