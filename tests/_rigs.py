"""Stereo rigs beyond KITTI's rectified one, shared by the renderer, oracle and GPU parity tests.

Each rig is a dict of synth.StereoSequence keyword arguments at 1241x376 (the reference's construction P1 = K1 [I|0],
P2 = K2 [R_rl | t_rl], src/parameter.cpp):
  R0  KITTI (the control): fx = fy, K2 = K1, R_rl = I, t_rl = (-0.537, 0, 0);
  R1  anisotropic: fy = 0.85 fx, principal point off centre, still rectified;
  R2  unequal cameras: fx2 = 1.03 fx1, cx2 = cx1 + 12, cy2 = cy1 - 2.5, R_rl = I;
  R3  unrectified: a rotation of 0.012 rad (yaw, roll and some pitch) and t_rl with y and z components of 2 cm, so that
      the stereo epipolar filters of both track modes (|y_L - y_R| against feature_match_error) reject a real share of
      the candidates while the steps still succeed (oracle, three of its 8 pairs: LK 30 %, ORB 56 %);
  R3X R3 with a pitch of 0.03 rad: every stereo pair lies ~20 px off its row, the filters reject (nearly) all of them
      and the step stops at stage 2."""
import numpy as np
from scipy.spatial.transform import Rotation

W, H = 1241, 376
FX, CX, CY = 718.856, 607.193, 185.216

R3_ROTVEC = (0.0035, 0.009, 0.007)         # |r| = 0.012 rad
R3_T = (-0.537, 0.02, 0.02)

RIGS = {
    "R0": dict(),
    "R1": dict(fx=FX, fy=0.85 * FX, cx=631.5, cy=171.25),
    "R2": dict(fx2=1.03 * FX, fy2=FX, cx2=CX + 12.0, cy2=CY - 2.5),
    "R3": dict(R_rl=Rotation.from_rotvec(R3_ROTVEC).as_matrix(), t_rl=R3_T),
    "R3X": dict(R_rl=Rotation.from_rotvec((0.03, 0.009, 0.007)).as_matrix(), t_rl=R3_T),
}


def sequence(synth, name, n_frames, device="cpu", seed=20200710, **kw):
    return synth.StereoSequence(width=W, height=H, n_frames=n_frames, seed=seed, device=device, **RIGS[name], **kw)


def matrices(name):
    """(P1, P2) as 3x4 float64 arrays, built in numpy from the rig's parameters (not through the renderer)."""
    r = RIGS[name]
    fx, fy = r.get("fx", FX), r.get("fy", r.get("fx", FX))
    cx, cy = r.get("cx", CX), r.get("cy", CY)
    K1 = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]])
    K2 = np.array([[r.get("fx2", fx), 0, r.get("cx2", cx)], [0, r.get("fy2", fy), r.get("cy2", cy)], [0, 0, 1.0]])
    R = np.asarray(r.get("R_rl", np.eye(3)), np.float64)
    t = np.asarray(r.get("t_rl", (-0.537, 0.0, 0.0)), np.float64)
    return np.hstack([K1, np.zeros((3, 1))]), K2 @ np.hstack([R, t[:, None]])


def general_matrices(seed):
    """Random full 3x4 P1, P2 without structure (non-zero skew, fourth columns and third rows), the points in front
    of both cameras: (P1, P2, X (n, 3))."""
    rng = np.random.default_rng(seed)
    P1 = rng.normal(size=(3, 4)) * [[500], [500], [1]]
    P2 = rng.normal(size=(3, 4)) * [[500], [500], [1]]
    X = rng.uniform(-5, 5, (400, 3))
    d1 = (P1 @ np.c_[X, np.ones(len(X))].T)[2]
    d2 = (P2 @ np.c_[X, np.ones(len(X))].T)[2]
    keep = (np.abs(d1) > 0.3) & (np.abs(d2) > 0.3)
    return P1, P2, X[keep]
