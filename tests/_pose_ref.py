"""numpy twin of the rigid-pose algebra of the pose stage (csrc/pose_device.h): 4 x 4 products and inverses, the Euler-angle
gates and the pose chain, each in the association order the kernels keep.  The HIP code must equal it bit for bit (the
arctan2 of the Euler angles is compared through the gates' decisions only).  tests/_keyframe_ref.py and tests/_window_ref.py
build on it."""
import numpy as np


def mul4(A, B):
    """4 x 4 product in the chain's association order: k ascending, separate multiply and add, from 0"""
    A, B = np.asarray(A, np.float64).reshape(4, 4), np.asarray(B, np.float64).reshape(4, 4)
    C = np.zeros((4, 4))
    for i in range(4):
        for j in range(4):
            s = np.float64(0)
            for k in range(4):
                s = s + A[i, k] * B[k, j]
            C[i, j] = s
    return C


def inv_t4(P):
    """rule T4: camera from world of a world-from-camera pose: R = Rw^T, t_i = -((R_i0 tw_0 + R_i1 tw_1) + R_i2 tw_2)"""
    P = np.asarray(P, np.float64).reshape(4, 4)
    out = np.eye(4)
    for i in range(3):
        r = P[:3, i]
        out[i, :3] = r
        out[i, 3] = -((r[0] * P[0, 3] + r[1] * P[1, 3]) + r[2] * P[2, 3])
    return out


def inv_rt(R, t):
    """inverse([R t]) in the closed form of T_rel_inv (finalize_pair): R^T, -(R^T t) summed left to right"""
    R, t = np.asarray(R, np.float64).reshape(3, 3), np.asarray(t, np.float64).reshape(3)
    out = np.eye(4)
    out[:3, :3] = R.T
    for i in range(3):
        out[i, 3] = -(R[0, i] * t[0] + R[1, i] * t[1] + R[2, i] * t[2])
    return out


def euler(R):
    """rotationMatrixToEulerAngles as the pair's gate computes it: floats holding double expressions"""
    R = np.asarray(R, np.float64).reshape(3, 3)
    sy = np.float32(np.sqrt(R[0, 0] * R[0, 0] + R[1, 0] * R[1, 0]))
    if not float(sy) < 1e-6:
        return (np.float32(np.arctan2(R[2, 1], R[2, 2])), np.float32(np.arctan2(-R[2, 0], float(sy))), np.float32(np.arctan2(R[1, 0], R[0, 0])))
    return (np.float32(np.arctan2(-R[1, 2], R[1, 1])), np.float32(np.arctan2(-R[2, 0], float(sy))), np.float32(0))


def gates(F, max_move2):
    """K4's gates on the implied motion: every Euler angle below 0.1, |t|^2 below max_move2 (no lower bound)"""
    ex, ey, ez = euler(F[:3, :3])
    n2 = F[0, 3] * F[0, 3] + F[1, 3] * F[1, 3] + F[2, 3] * F[2, 3]
    return bool(abs(float(ey)) < 0.1 and abs(float(ex)) < 0.1 and abs(float(ez)) < 0.1 and n2 < max_move2)


def chain(T, ok, pose0=None):
    """svo_chain_relative / the batch's pose chain: poses[p] = pose0 T[q0] T[q1] ... over the q <= p with ok[q], folded from
    the left with mul4; pose0 None: the identity.  T (n, 16) or (n, 4, 4); returns (n, 4, 4)."""
    T = np.asarray(T, np.float64).reshape(-1, 4, 4)
    P = np.eye(4) if pose0 is None else np.asarray(pose0, np.float64).reshape(4, 4).copy()
    out = np.zeros_like(T)
    for p in range(len(T)):
        if ok[p]:
            P = mul4(P, T[p])
        out[p] = P
    return out


def rigid_motions(rng, n):
    """Test input: n rigid 4 x 4 motions, float64 Rodrigues rotations of <= 0.05 rad about random axes, translations of <= 1"""
    T = np.zeros((n, 4, 4))
    for k in range(n):
        axis, t = rng.standard_normal(3), rng.standard_normal(3)
        axis /= np.linalg.norm(axis)
        th = rng.uniform(0.0, 0.05)
        K = np.array([[0.0, -axis[2], axis[1]], [axis[2], 0.0, -axis[0]], [-axis[1], axis[0], 0.0]])
        T[k, :3, :3] = np.eye(3) + np.sin(th) * K + (1.0 - np.cos(th)) * (K @ K)
        T[k, :3, 3] = t / np.linalg.norm(t) * rng.uniform(0.0, 1.0)
        T[k, 3, 3] = 1.0
    return T


CHAIN_N = (1, 63, 64, 65, 130)          # the chain stages 64 pairs a trip: a short trip, one short of a trip, a full trip, one over, three trips


def chain_cases(seed=20241):
    """{(n, seeded): (T, ok, pose0)} for n in CHAIN_N: ok = 0 at pairs 0, 63, 64 and n - 1 where they exist; pose0 None or a motion"""
    rng = np.random.default_rng(seed)
    cases = {}
    for n in CHAIN_N:
        T = rigid_motions(rng, n)
        ok = np.ones(n, np.int32)
        ok[[i for i in (0, 63, 64, n - 1) if i < n]] = 0
        cases[n, False] = (T, ok, None)
        cases[n, True] = (T, ok, rigid_motions(rng, 1)[0])
    return cases
