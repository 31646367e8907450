"""tests/_truth.py's helpers on the CPU: round trips to 1e-9 px on the KITTI-like 416 x 128 rig and on an unrectified one, the
right camera against the rig's own P2, and chain_stats() on a hand-made chain whose errors are known."""
import numpy as np
import pytest
import torch

import _rigs
import _truth as TR

RIGS = {"default": {}, "R3": {k: v for k, v in _rigs.RIGS["R3"].items()}}


@pytest.fixture(scope="module", params=sorted(RIGS))
def seq(synth, request):
    return synth.StereoSequence(width=416, height=128, n_frames=12, seed=11, **RIGS[request.param])


def _pixels(n, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(0, 415, n), rng.uniform(0, 127, n)], 1)


@pytest.mark.parametrize("cam", [0, 1])
def test_world_point_and_project_round_trip(seq, cam):
    xy = _pixels(500, 1)
    for t in (0, 7):
        X = TR.world_point(seq, t, cam, xy)
        back, Z = TR.project(seq, t, cam, X)
        assert np.abs(back - xy).max() <= 1e-9 and (Z > 0).all()
        assert np.abs(Z - seq.depth(t, cam, *(torch.from_numpy(xy[:, k].copy()) for k in (0, 1))).numpy()).max() <= 1e-9 * Z.max()
        # the points lie on the corridor's four planes
        on = np.minimum.reduce([np.abs(X[:, 1] - seq.cam_height), np.abs(X[:, 1] + seq.ceil_height), np.abs(np.abs(X[:, 0]) - seq.half_width)])
        assert on.max() <= 1e-9 * max(1.0, np.abs(X).max())


def test_project_is_the_rigs_projection_matrices(seq):
    """project() goes through seq.camera(); P1 / P2 of seq.proj() applied to the point in the left camera frame must agree."""
    xy = _pixels(300, 2)
    X = TR.world_point(seq, 3, 0, xy)
    T = np.linalg.inv(seq.poses_wc().numpy()[5])
    Xc = X @ T[:3, :3].T + T[:3, 3]
    for cam, P in enumerate(seq.proj()):
        P = np.asarray(P, np.float64).reshape(3, 4)
        h = Xc @ P[:, :3].T + P[:, 3]
        got, Z = TR.project(seq, 5, cam, X)
        assert np.abs(got - h[:, :2] / h[:, 2:3]).max() <= 1e-9 and np.abs(Z - h[:, 2]).max() <= 1e-9 * Z.max()


def test_transfer_error_is_zero_on_true_transfers_and_the_offset_otherwise(seq):
    xy = _pixels(400, 3)
    for (ta, ca), (tb, cb) in (((2, 0), (3, 0)), ((0, 0), (11, 0)), ((4, 0), (4, 1)), ((6, 1), (5, 0))):
        to, _ = TR.project(seq, tb, cb, TR.world_point(seq, ta, ca, xy))
        assert TR.transfer_error(seq, ta, xy, tb, to, ca, cb).max() <= 1e-9
        assert np.abs(TR.transfer_error(seq, ta, xy, tb, to + [3.0, -4.0], ca, cb) - 5.0).max() <= 1e-9
    assert TR.transfer_error(seq, 2, xy, 2, xy).max() <= 1e-9


def test_chain_stats_on_a_hand_made_chain(synth):
    """Three pairs; 40 ids from frame 0 that slide 0.5 px a frame in x, 10 ids from frame 1 that are exact, one id whose last
    observation is 20 px off and no inlier; a table 0.25 px of disparity off."""
    seq = synth.StereoSequence(width=416, height=128, n_frames=4, seed=11)
    rng = np.random.default_rng(4)
    xy0 = np.stack([rng.uniform(150, 260, 41), rng.uniform(70, 120, 41)], 1)        # the ground ahead: in view for four frames
    xy1 = np.stack([rng.uniform(150, 260, 10), rng.uniform(70, 120, 10)], 1)
    at = lambda t0, xy, t: TR.project(seq, t, 0, TR.world_point(seq, t0, 0, xy))[0]
    steps = []
    for k in range(3):
        a = [at(0, xy0, k) + [0.5 * k, 0], at(0, xy0, k + 1) + [0.5 * (k + 1), 0]]
        ids, inl = list(range(100, 141)), np.ones(41, np.uint8)
        if k == 2:
            a[1][40] += [0, 20.0]
            inl[40] = 0
        if k >= 1:
            a = [np.r_[a[0], at(1, xy1, k)], np.r_[a[1], at(1, xy1, k + 1)]]
            ids, inl = ids + list(range(200, 210)), np.r_[inl, np.ones(10, np.uint8)]
        z = np.zeros_like(a[0])
        steps.append(dict(tracks=[a[0], z, z, a[1], inl], ids=np.array(ids), table=None))
    Xk = TR.world_point(seq, 0, 0, xy0)                                # frame 0 is the world frame
    d = seq.fx * seq.baseline / Xk[:, 2] + 0.25
    steps[0]["table"] = (0, Xk * (seq.fx * seq.baseline / d / Xk[:, 2])[:, None])
    st = TR.chain_stats(seq, steps)
    assert st["age_n"] == {1: 51, 2: 51, 3: 41} and st["pair"]["n"] == 41 + 51 + 50 and st["beyond10"] == dict(share=0.0, n=142)
    assert abs(st["age"][1] - 0.5) < 1e-6 and abs(st["age"][2] - 1.0) < 1e-6 and abs(st["age"][3] - 1.5) < 1e-6
    assert 0.25 < st["pair"]["median"] <= st["pair"]["max"] <= 0.5 + 1e-6      # one pair: the slide of one frame, seen from a point already off
    assert abs(st["table"]["median_abs"] - 0.25) < 1e-6 and abs(st["table"]["abs_mean"] - 0.25) < 1e-6 and st["table"]["n"] == 41
