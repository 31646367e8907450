"""Synthetic KITTI-like stereo sequences with ground-truth poses (test/bench data plumbing).

There is no KITTI data in the build or GPU environment, so BASELINE
config #1/#2 run on "S0": a procedurally textured corridor (ground, two walls, a ceiling) rendered
by ray casting through the reference rig of config/default.yaml:33-57 (fx = fy = 718.856,
cx = 607.193, cy = 185.216, baseline 0.537 m) along a forward trajectory with a slowly oscillating
yaw.  Left and right views are rendered from the two camera centres, so stereo disparity, temporal
flow and the PnP geometry are all consistent with the known SE(3) motion.

Two options, both off by default (the default rendering is unchanged byte for byte): `texture=` replaces the hashed
value noise with a 2-D image in [0, 1] sampled bilinearly with wrap-around (natural content: flat and saturated areas,
smooth gradients), and per-camera photometry (`gain`, `offset`, `gamma`, each a scalar or a (left, right) pair)
applied to the intensity before the clamp to uint8 (exposure differences, and stereo without brightness constancy).

The right camera may also be a general one (`fx2`, `fy2`, `cx2`, `cy2`, `R_rl`, `t_rl`, all off by default): proj() then
returns P1 = K1 [I|0] and P2 = K2 [R_rl | t_rl], the reference's construction (t_lr* / R_lr* row-major, src/parameter.cpp),
and the right view is cast from C_r = -R_rl^T t_rl along R_wc R_rl^T K2^-1 [u v 1]^T.  The default rig keeps the float32
rectified code path, so its bytes do not change either.

Written with torch so the same code renders small CPU cases for tests and full-size frames on
cuda for bench.py.  Only integer hashing and float32 arithmetic that is independent of reduction
order is used, but CPU and GPU renderings are NOT required to match bit for bit: every consumer
(HIP path, oracle) is handed the SAME rendered uint8 frames.
"""
import math

import torch

KITTI_K = dict(fx=718.856, fy=718.856, cx=607.193, cy=185.216)
KITTI_BASELINE = 0.537


def proj_matrices(fx=KITTI_K["fx"], fy=KITTI_K["fy"], cx=KITTI_K["cx"], cy=KITTI_K["cy"],
                  baseline=KITTI_BASELINE):
    """P1 = K[I|0], P2 = K[I|t], t = (-baseline, 0, 0)  (reference src/parameter.cpp:42-45)."""
    P1 = [fx, 0.0, cx, 0.0, 0.0, fy, cy, 0.0, 0.0, 0.0, 1.0, 0.0]
    P2 = [fx, 0.0, cx, fx * (-baseline), 0.0, fy, cy, 0.0, 0.0, 0.0, 1.0, 0.0]
    return P1, P2


def _hash01(u, v, k):
    """Integer lattice hash -> float in [0,1).  u, v int64 tensors, k python int."""
    h = (u * 73856093) ^ (v * 19349663) ^ (k * 83492791)
    h = (h ^ (h >> 13)) * 1274126177
    h = h ^ (h >> 16)
    return (h & 0xFFFF).to(torch.float32) / 65536.0


def _per_cam(v):
    """A scalar for both cameras, or a (left, right) pair -> (left, right) floats."""
    if isinstance(v, (tuple, list)):
        assert len(v) == 2, v
        return float(v[0]), float(v[1])
    return float(v), float(v)


class StereoSequence:
    """Procedural corridor seen by a forward-moving rectified stereo rig."""

    def __init__(self, width=1241, height=376, n_frames=101, seed=20200710, device="cpu",
                 fx=None, fy=None, cx=None, cy=None, baseline=KITTI_BASELINE,
                 step=1.0, yaw_amp=0.02, yaw_period=48.0, scales=(0.35, 1.4, 5.6),
                 weights=(0.55, 0.3, 0.15), supersample=2, half_width=7.0, cam_height=1.65,
                 ceil_height=6.0, fog=90.0, texture=None, texel=0.03, gain=1.0, offset=0.0, gamma=1.0,
                 fx2=None, fy2=None, cx2=None, cy2=None, R_rl=None, t_rl=None):
        # default intrinsics: KITTI at full size, scaled with the image width otherwise
        s = width / 1241.0
        self.w, self.h = int(width), int(height)
        self.fx = fx if fx is not None else KITTI_K["fx"] * s
        self.fy = fy if fy is not None else KITTI_K["fy"] * s
        self.cx = cx if cx is not None else KITTI_K["cx"] * s
        if cy is None:
            cy = KITTI_K["cy"] * s if abs(height - 376.0 * s) < 2.0 else (height - 1) * 0.5
        self.cy = cy
        self.baseline = baseline
        self.n_frames = n_frames
        self.seed = int(seed)
        self.device = torch.device(device)
        self.step, self.yaw_amp, self.yaw_period = step, yaw_amp, yaw_period
        self.scales, self.weights, self.ss = scales, weights, int(supersample)
        self.half_width, self.cam_height, self.ceil_height, self.fog = half_width, cam_height, ceil_height, fog
        self.tex = None
        if texture is not None:
            tex = torch.as_tensor(texture, dtype=torch.float32)
            assert tex.dim() == 2 and tex.shape[0] >= 2 and tex.shape[1] >= 2, tex.shape
            assert float(tex.min()) >= 0.0 and float(tex.max()) <= 1.0, "texture values must lie in [0, 1]"
            self.tex = tex.to(self.device).contiguous()
        self.texel = float(texel)                  # metres per texel of `texture` (3 cm: finer aliases into value noise far off)
        self.gain, self.offset, self.gamma = _per_cam(gain), _per_cam(offset), _per_cam(gamma)
        # the right camera: K2 [R_rl | t_rl] (x_right = R_rl x_left + t_rl), by default the rectified K1 [I | (-b, 0, 0)]
        self.fx2 = float(fx2) if fx2 is not None else float(self.fx)
        self.fy2 = float(fy2) if fy2 is not None else float(self.fy)
        self.cx2 = float(cx2) if cx2 is not None else float(self.cx)
        self.cy2 = float(cy2) if cy2 is not None else float(self.cy)
        self.R_rl = torch.eye(3, dtype=torch.float64) if R_rl is None else \
            torch.as_tensor(R_rl, dtype=torch.float64).reshape(3, 3).clone()
        self.t_rl = torch.tensor([-float(baseline), 0.0, 0.0], dtype=torch.float64) if t_rl is None else \
            torch.as_tensor(t_rl, dtype=torch.float64).reshape(3).clone()
        self.rectified = ((self.fx2, self.fy2, self.cx2, self.cy2) == (float(self.fx), float(self.fy), float(self.cx), float(self.cy))
                          and torch.equal(self.R_rl, torch.eye(3, dtype=torch.float64))
                          and self.t_rl.tolist() == [-float(baseline), 0.0, 0.0])
        self._poses = self._make_poses()

    # ---- trajectory ------------------------------------------------------------------------
    def _make_poses(self):
        """T_wc (camera -> world) per frame, float64, world = KITTI convention (x right, y down,
        z forward).  Step length varies in [0.8, 1.2]*step, yaw oscillates."""
        g = torch.Generator().manual_seed(self.seed)
        steps = (0.8 + 0.4 * torch.rand(self.n_frames, generator=g, dtype=torch.float64)) * self.step
        poses = []
        x = z = 0.0
        for t in range(self.n_frames):
            yaw = self.yaw_amp * math.sin(2.0 * math.pi * t / self.yaw_period)
            c, s = math.cos(yaw), math.sin(yaw)
            T = torch.tensor([[c, 0.0, s, x], [0.0, 1.0, 0.0, 0.0], [-s, 0.0, c, z],
                              [0.0, 0.0, 0.0, 1.0]], dtype=torch.float64)
            poses.append(T)
            x += s * float(steps[t])
            z += c * float(steps[t])
        return torch.stack(poses)

    def poses_wc(self):
        return self._poses.clone()

    def relative_gt(self, t):
        """T mapping camera t-1 coordinates to camera t coordinates (what PnP estimates)."""
        return torch.linalg.inv(self._poses[t]) @ self._poses[t - 1]

    def proj(self):
        if self.rectified:
            return proj_matrices(self.fx, self.fy, self.cx, self.cy, self.baseline)
        K2 = self.K(1)
        P1 = [self.fx, 0.0, self.cx, 0.0, 0.0, self.fy, self.cy, 0.0, 0.0, 0.0, 1.0, 0.0]
        P2 = (K2 @ torch.cat([self.R_rl, self.t_rl[:, None]], 1)).reshape(12).tolist()
        return P1, P2

    def K(self, cam):
        """3x3 float64 intrinsics of camera `cam` (0 left, 1 right)."""
        fx, fy, cx, cy = (self.fx, self.fy, self.cx, self.cy) if cam == 0 else (self.fx2, self.fy2, self.cx2, self.cy2)
        return torch.tensor([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]], dtype=torch.float64)

    def camera(self, t, cam):
        """(centre (3,), M (3, 3)) in world coordinates, float64: the ray through pixel (u, v) of camera `cam` at frame t
        is centre + s * M [u v 1]^T.  Right camera: centre p + R_wc C_r with C_r = -R_rl^T t_rl, M = R_wc R_rl^T K2^-1."""
        T = self._poses[t]
        R, p = T[:3, :3], T[:3, 3]
        if cam == 0:
            return p.clone(), R @ torch.linalg.inv(self.K(0))
        return p + R @ (-self.R_rl.T @ self.t_rl), R @ self.R_rl.T @ torch.linalg.inv(self.K(1))

    def depth(self, t, cam, u, v):
        """Camera-frame depth Z of the nearest surface seen through pixel coordinates (u, v) (float64 tensors of one
        shape, no supersampling) of camera `cam` at frame t, ray-cast in float64 through camera()."""
        o, M = self.camera(t, cam)
        u = torch.as_tensor(u, dtype=torch.float64)
        v = torch.as_tensor(v, dtype=torch.float64)
        d = [M[i, 0] * u + M[i, 1] * v + M[i, 2] for i in range(3)]
        s = self._hit(float(o[0]), float(o[1]), float(o[2]), *d)
        Rc = self._poses[t][:3, :3] if cam == 0 else self._poses[t][:3, :3] @ self.R_rl.T
        # camera-frame direction = Rc^T d: its z component scales the hit distance to depth
        dz = Rc[0, 2] * d[0] + Rc[1, 2] * d[1] + Rc[2, 2] * d[2]
        return s * dz

    # ---- rendering -------------------------------------------------------------------------
    def _texture(self, u, v, plane):
        if self.tex is not None:
            return self._sample(u, v, plane)
        val = torch.zeros_like(u)
        for k, (sc, wt) in enumerate(zip(self.scales, self.weights)):
            iu = torch.floor(u / sc).to(torch.int64)
            iv = torch.floor(v / sc).to(torch.int64)
            val = val + wt * _hash01(iu, iv, self.seed % 65521 + 131 * plane + 17 * k)
        return val

    def _sample(self, u, v, plane):
        """Bilinear lookup of `texture` with wrap-around at `texel` metres per texel; each plane starts at its own
        offset into the image so that the four surfaces do not repeat each other."""
        th, tw = self.tex.shape
        fu = u / self.texel + (0.37 * plane) * tw
        fv = v / self.texel + (0.61 * plane) * th
        u0, v0 = torch.floor(fu), torch.floor(fv)
        au, av = fu - u0, fv - v0
        iu0 = torch.remainder(u0.to(torch.int64), tw)
        iv0 = torch.remainder(v0.to(torch.int64), th)
        iu1 = torch.remainder(iu0 + 1, tw)
        iv1 = torch.remainder(iv0 + 1, th)
        t = self.tex
        top = t[iv0, iu0] * (1.0 - au) + t[iv0, iu1] * au
        bot = t[iv1, iu0] * (1.0 - au) + t[iv1, iu1] * au
        return top * (1.0 - av) + bot * av

    def _planes(self, ox, oy, oz, dx, dy, dz):
        """Ray parameters of the ground (y = cam_height), ceiling (y = -ceil_height) and walls (x = +-half_width)."""
        big = 1e9
        eps = 1e-9
        sg = torch.where(dy > eps, (self.cam_height - oy) / dy, torch.full_like(dy, big))
        sc = torch.where(dy < -eps, (-self.ceil_height - oy) / dy, torch.full_like(dy, big))
        sl = torch.where(dx < -eps, (-self.half_width - ox) / dx, torch.full_like(dx, big))
        sr = torch.where(dx > eps, (self.half_width - ox) / dx, torch.full_like(dx, big))
        return sg, sc, sl, sr

    def _hit(self, ox, oy, oz, dx, dy, dz):
        sg, sc, sl, sr = self._planes(ox, oy, oz, dx, dy, dz)
        return torch.minimum(torch.minimum(sg, sc), torch.minimum(sl, sr))

    def _shade(self, ox, oy, oz, dx, dy, dz):
        """Nearest hit among the four planes; returns intensity in [0,1]."""
        sg, sc, sl, sr = self._planes(ox, oy, oz, dx, dy, dz)
        s = torch.minimum(torch.minimum(sg, sc), torch.minimum(sl, sr))
        X, Y, Z = ox + s * dx, oy + s * dy, oz + s * dz
        tex = torch.where(s == sg, self._texture(X, Z, 0),
                          torch.where(s == sc, self._texture(X, Z, 1),
                                      torch.where(s == sl, self._texture(Z, Y, 2),
                                                  self._texture(Z, Y, 3))))
        fogw = torch.exp(-s / self.fog)
        return tex * fogw + 0.5 * (1.0 - fogw)

    def render(self, t):
        """Returns (left, right) uint8 tensors of shape (h, w) on self.device."""
        dev = self.device
        T = self._poses[t].to(torch.float32)
        R = T[:3, :3].to(dev)
        p = T[:3, 3]
        ss = self.ss
        offs = [(i + 0.5) / ss - 0.5 for i in range(ss)]
        vs = torch.arange(self.h, device=dev, dtype=torch.float32)
        us = torch.arange(self.w, device=dev, dtype=torch.float32)
        out = []
        for cam in range(2):
            acc = torch.zeros(self.h, self.w, device=dev, dtype=torch.float32)
            if cam == 0 or self.rectified:
                # camera centre in world: left at p, right at p + R * (baseline, 0, 0)
                o = p + T[:3, 0] * (self.baseline * cam)
                for oy_ in offs:
                    for ox_ in offs:
                        xc = ((us + ox_) - self.cx) / self.fx
                        yc = ((vs + oy_) - self.cy) / self.fy
                        xcg, ycg = torch.meshgrid(xc, yc, indexing="xy")
                        dx = R[0, 0] * xcg + R[0, 1] * ycg + R[0, 2]
                        dy = R[1, 0] * xcg + R[1, 1] * ycg + R[1, 2]
                        dz = R[2, 0] * xcg + R[2, 1] * ycg + R[2, 2]
                        acc += self._shade(float(o[0]), float(o[1]), float(o[2]), dx, dy, dz)
            else:
                # a general right camera (camera()): float32 rays from its own centre through R_wc R_rl^T K2^-1
                o, M = self.camera(t, 1)
                M = M.to(torch.float32).to(dev)
                for oy_ in offs:
                    for ox_ in offs:
                        ug, vg = torch.meshgrid(us + ox_, vs + oy_, indexing="xy")
                        dx = M[0, 0] * ug + M[0, 1] * vg + M[0, 2]
                        dy = M[1, 0] * ug + M[1, 1] * vg + M[1, 2]
                        dz = M[2, 0] * ug + M[2, 1] * vg + M[2, 2]
                        acc += self._shade(float(o[0]), float(o[1]), float(o[2]), dx, dy, dz)
            val = acc / (ss * ss)
            # the photometry; each step is skipped at its identity so that the default bytes are unchanged
            if self.gamma[cam] != 1.0:
                val = val.clamp(min=0.0).pow(self.gamma[cam])
            val = val * 255.0
            if self.gain[cam] != 1.0:
                val = val * self.gain[cam]
            if self.offset[cam] != 0.0:
                val = val + self.offset[cam]
            img = val.clamp(0, 255).round().to(torch.uint8)
            out.append(img)
        return out[0], out[1]

    def render_range(self, t0, t1):
        """Stacked (left, right) of frames [t0, t1): two uint8 tensors (n, h, w)."""
        Ls, Rs = [], []
        for t in range(t0, t1):
            L, R = self.render(t)
            Ls.append(L)
            Rs.append(R)
        return torch.stack(Ls), torch.stack(Rs)
