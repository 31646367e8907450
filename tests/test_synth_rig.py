"""The renderer's general stereo rig (CPU): right-camera intrinsics K2, R_rl and t_rl (synth.StereoSequence fx2, fy2,
cx2, cy2, R_rl, t_rl; tests/_rigs.py's R0-R3).

  * the default rig, given explicitly, renders the bytes the rectified path renders (test_synth_natural.py pins those
    against the committed golden frames);
  * the right view is the camera P2 describes: a left pixel back-projected with the left depth and projected with a
    numpy-built P2 lands where the right camera sees the same surface point, and the right image equals a left-camera
    rendering (the original code path) from the right camera's pose with K2;
  * anisotropic intrinsics (fy != fx) project consistently with the returned P1."""
import numpy as np
import pytest
import torch

import _rigs

W, H = _rigs.W, _rigs.H


def _grid(n=41, m=17, margin=4.0):
    u, v = np.meshgrid(np.linspace(margin, W - 1 - margin, n), np.linspace(margin, H - 1 - margin, m))
    return u.ravel(), v.ravel()


def test_default_rig_given_explicitly_renders_the_same_bytes(synth):
    seq = synth.StereoSequence(width=W, height=H, n_frames=3, seed=20200710)
    b = synth.KITTI_BASELINE
    exp = synth.StereoSequence(width=W, height=H, n_frames=3, seed=20200710, fx2=seq.fx, fy2=seq.fy, cx2=seq.cx,
                               cy2=seq.cy, R_rl=np.eye(3), t_rl=(-b, 0.0, 0.0))
    assert seq.rectified and exp.rectified
    assert exp.proj() == seq.proj() == synth.proj_matrices(seq.fx, seq.fy, seq.cx, seq.cy, b)
    for t in (0, 2):
        for a, c in zip(seq.render(t), exp.render(t)):
            assert torch.equal(a, c)
    # a general rig is reported as one, and the default's P2 is K1 [I | (-b, 0, 0)] in the general construction too
    P1, P2 = _rigs.matrices("R0")
    assert np.allclose(np.asarray(seq.proj()[1]).reshape(3, 4), P2, rtol=0, atol=1e-12)
    assert not _rigs.sequence(synth, "R3", 2).rectified and not _rigs.sequence(synth, "R2", 2).rectified


@pytest.mark.parametrize("name", ["R0", "R1", "R2", "R3", "R3X"])
def test_proj_is_the_reference_construction(synth, name):
    """proj() = (K1 [I|0], K2 [R_rl | t_rl]) with every entry of the numpy product (1 ulp: the product's rounding)."""
    seq = _rigs.sequence(synth, name, 2)
    P1, P2 = _rigs.matrices(name)
    g1, g2 = (np.asarray(p, np.float64).reshape(3, 4) for p in seq.proj())
    assert np.array_equal(g1, P1)
    assert np.all(np.abs(g2 - P2) <= np.spacing(np.abs(P2)))


@pytest.mark.parametrize("name", ["R0", "R1", "R2", "R3", "R3X"])
def test_right_camera_is_the_one_p2_describes(synth, name):
    """Left pixel + left depth -> 3-D point -> P2 (numpy) -> right pixel: the right camera's depth there is the point's
    depth in the right camera.  The corridor is seen from inside, so nothing is occluded: every sample must agree.  A
    right camera still placed by the rectified formula is off by several pixels on R2 / R3 and fails this by far."""
    seq = _rigs.sequence(synth, name, 6)
    P1, P2 = _rigs.matrices(name)
    K1 = P1[:, :3]
    u, v = _grid()
    for t in (0, 5):
        Z = seq.depth(t, 0, torch.from_numpy(u), torch.from_numpy(v)).numpy()
        X = Z * (np.linalg.inv(K1) @ np.stack([u, v, np.ones_like(u)]))
        x2 = P2 @ np.vstack([X, np.ones_like(u)])
        u2, v2, z2 = x2[0] / x2[2], x2[1] / x2[2], x2[2]
        Zr = seq.depth(t, 1, torch.from_numpy(u2), torch.from_numpy(v2)).numpy()
        assert np.abs(Zr - z2).max() <= 1e-9 * np.abs(z2).max(), (t, np.abs(Zr - z2).max())
        if name in ("R2", "R3"):
            # the rectified placement would put this point at (u - fx * b / Z, v): several pixels off here
            off = np.hypot(u2 - (u - K1[0, 0] * 0.537 / Z), v2 - v)
            assert np.median(off) > 2.0, np.median(off)


@pytest.mark.parametrize("name", ["R1", "R2", "R3"])
def test_right_view_equals_a_left_camera_rendering_from_the_right_pose(synth, name):
    """The right image of a general rig against the left-camera code path, given K2 as its intrinsics and the right
    camera's pose T_wc [R_rl^T | -R_rl^T t_rl]: the same float32 rays up to their last bits (a ray grazing a plane
    edge may pick the other plane: tens of pixels per frame at most).  The rectified placement moves most pixels."""
    seq = _rigs.sequence(synth, name, 3)
    _, P2 = _rigs.matrices(name)
    rig = _rigs.RIGS[name]
    R, tr = np.asarray(rig.get("R_rl", np.eye(3))), np.asarray(rig.get("t_rl", (-0.537, 0.0, 0.0)))
    Kr = np.array([[seq.fx2, 0, seq.cx2], [0, seq.fy2, seq.cy2], [0, 0, 1.0]])
    assert np.allclose(Kr @ np.c_[R, tr], P2, rtol=1e-15, atol=1e-12)
    twin = synth.StereoSequence(width=W, height=H, n_frames=3, seed=20200710, fx=seq.fx2, fy=seq.fy2, cx=seq.cx2, cy=seq.cy2)
    T_lr = np.eye(4)
    T_lr[:3, :3], T_lr[:3, 3] = R.T, -R.T @ tr
    twin._poses = seq.poses_wc() @ torch.from_numpy(T_lr)
    for t in (0, 2):
        got = seq.render(t)[1].numpy().astype(int)
        want = twin.render(t)[0].numpy().astype(int)
        d = np.abs(got - want)
        assert (d > 0).mean() < 3e-4, (t, d.max(), (d > 0).mean())


def test_anisotropic_intrinsics_project_with_p1(synth):
    """R1 (fy = 0.85 fx, off-centre principal point), frame 0 (camera = world): ground, wall and ceiling points
    projected with the returned P1 are seen by the left camera at exactly their depth; so are they by the right camera
    through the returned P2.  Swapping fx and fy anywhere moves each pixel by up to ~100 px."""
    seq = _rigs.sequence(synth, "R1", 1)
    assert abs(seq.fy / seq.fx - 0.85) < 1e-12 and seq.cx != _rigs.CX
    rng = np.random.default_rng(3)
    n = 300
    z = rng.uniform(4, 40, n)
    pts = np.concatenate([np.c_[rng.uniform(-6.5, 6.5, n), np.full(n, seq.cam_height), z],           # ground
                          np.c_[np.full(n, seq.half_width), rng.uniform(-5.5, 1.5, n), z],            # right wall
                          np.c_[rng.uniform(-6.5, 6.5, n), np.full(n, -seq.ceil_height), z]])         # ceiling
    for cam, P in enumerate(seq.proj()):
        P = np.asarray(P).reshape(3, 4)
        x = P @ np.c_[pts, np.ones(len(pts))].T
        u, v = x[0] / x[2], x[1] / x[2]
        inside = (u > 0) & (u < W - 1) & (v > 0) & (v < H - 1)
        assert inside.sum() > 400
        Z = seq.depth(0, cam, torch.from_numpy(u[inside]), torch.from_numpy(v[inside])).numpy()
        assert np.allclose(Z, x[2][inside], rtol=1e-10, atol=0), cam
