"""The four slots of an lk_kernel wave doing different things at the same time.  A wave tracks four points in lockstep and
carries their flags (live, iterating, re-stage, converged, status) as lane masks; a slot that stops hands the shared
reduction whatever its registers hold.  So the dangerous inputs are waves whose slots part ways: here every wave of the
point list holds points of four ROLES, and every role takes every slot position 0..3:

  * TRACKED   -- kept through all four calls of the circular chain;
  * FLAT      -- degenerate at level 0 (the window lies inside a flat region): status 0 in call 0, point left where the
                 upper levels put it;
  * LEAVES    -- within a few pixels of the left border, content moving outward by 12 px: the window leaves level 0
                 during the iterations (status 0, point more than 10 px outside);
  * NOEPI     -- a block shifted vertically by 5 px in the right image: tracked in call 0 (status 1), rejected by the
                 epipolar test |y0 - y1| > 3 afterwards.

Frames: 416 x 128, whole-pixel views of one smoothed blocky texture (right eye 3 px, next frame 2 px), a flat rectangle
in all four images, the border strip and the shifted block in the right image of the first pair.  The candidates of a
role are fixed by the geometry; what each of them does is read from the ORACLE's outputs alone (`_roles`), and before
anything touches the GPU the test asserts that every role occurs at least 8 times and that a wave with all four exists.

One pair goes through ctx.circular_match (the latency shape of the launch): with more than 3 x 3072 points a wave takes
four consecutive points, so the list -- 128 waves of four roles, the roles rotated from wave to wave -- is repeated
19 times.  The first 1, 2 and 3 points of an all-four-roles wave run alone as well (then every point has a wave of its
own).  Kept tracks byte for byte against the oracle, in the exact order and in the three float orders with the oracle
in the matching accumulation mode.  The references are computed once per module and only read."""
import numpy as np
import pytest

from test_gpu_lk_wave_mapping import FLOAT_ORDERS, H, W, _check_circular, _circular_reference
from test_gpu_parity_lk_sse2 import accum_oracle

pytestmark = pytest.mark.gpu

TRACKED, FLAT, LEAVES, NOEPI = range(4)
N_WAVES, REPEAT = 128, 19                       # 512 distinct points; 19 x 512 = 9728 > 3 x 3072: four points per wave
FLAT_X, FLAT_Y = (150, 214), (24, 104)          # the flat rectangle [x0, x1) x [y0, y1)
STRIP_W, STRIP_SHIFT = 60, 12                   # left strip of the right image: content moved 12 px to the left
BLOCK_X, BLOCK_Y, BLOCK_DY = (290, 390), (8, 120), 5


@pytest.fixture(scope="module")
def tc():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU; the hot path has no CPU fallback"
    return torch


def _frames():
    """(L0, R0, L1, R1): views of one canvas, so whole-pixel shifts bring real content in at the borders."""
    r = np.random.default_rng(1)
    c = r.integers(0, 256, ((H + 67) // 4, (W + 67) // 4), dtype=np.uint8).repeat(4, 0).repeat(4, 1)[:H + 64, :W + 64].astype(np.float32)
    for _ in range(2):                           # soften the block edges so that LK converges
        c = (c + np.roll(c, 1, 0) + np.roll(c, -1, 0) + np.roll(c, 1, 1) + np.roll(c, -1, 1)) / 5
    c = c.astype(np.uint8)

    def view(dx, dy=0):
        return np.array(c[32 + dy:32 + dy + H, 32 + dx:32 + dx + W])

    L0, R0, L1, R1 = view(0), view(3), view(2), view(5)
    R0[:, :STRIP_W] = view(STRIP_SHIFT)[:, :STRIP_W]
    by, bx = slice(*BLOCK_Y), slice(*BLOCK_X)
    R0[by, bx] = view(3, BLOCK_DY)[by, bx]
    for im in (L0, R0, L1, R1):
        im[FLAT_Y[0]:FLAT_Y[1], FLAT_X[0]:FLAT_X[1]] = 128
    return tuple(np.ascontiguousarray(im) for im in (L0, R0, L1, R1))


def _grid(xs, ys):
    gx, gy = np.meshgrid(np.asarray(xs, np.float32), np.asarray(ys, np.float32))
    return np.stack([gx.ravel(), gy.ravel()], 1)


def _points():
    """The 512 distinct points: wave k holds candidate k of every role, role (k + slot) % 4 in slot `slot`."""
    cand = [None] * 4
    cand[TRACKED] = _grid(np.arange(236, 284, 6), np.arange(20, 116, 6))        # 8 x 16, between the flat region and the block
    cand[FLAT] = _grid(np.arange(166, 198, 4), np.arange(40, 88, 3))            # window (+ 1 px of Scharr support) inside the flat region
    cand[LEAVES] = _grid(np.arange(2, 6), np.arange(16, 112, 3))                # 4 x 32, x = 2..5
    cand[NOEPI] = _grid(np.arange(312, 368, 7), np.arange(30, 94, 4))           # well inside the shifted block
    assert all(len(c) == N_WAVES for c in cand), [len(c) for c in cand]
    pts = np.empty((N_WAVES, 4, 2), np.float32)
    intended = np.empty((N_WAVES, 4), np.int64)
    for k in range(N_WAVES):
        for slot in range(4):
            role = (k + slot) % 4
            pts[k, slot] = cand[role][k]
            intended[k, slot] = role
    return pts.reshape(-1, 2), intended.reshape(-1)


def _roles(tracks, keep, st0):
    """What every point does, from the oracle's outputs alone (-1: none of the four roles).  A status 0 of call 0 has
    three causes: a window outside level 0 (nextPt more than 10 px outside the image -- at the level's start, during an
    iteration or in the final check) or the degenerate 2x2 system; prevPt itself lies inside the image."""
    p0, p1 = tracks[0], tracks[1]
    outside = (p1[:, 0] < -11) | (p1[:, 0] >= W + 10) | (p1[:, 1] < -11) | (p1[:, 1] >= H + 10)
    role = np.full(len(p0), -1)
    role[keep] = TRACKED
    role[(st0 == 0) & ~outside] = FLAT
    role[(st0 == 0) & outside] = LEAVES
    role[(st0 == 1) & ~keep & (np.abs(p0[:, 1] - p1[:, 1]) > 3.0) & (p1[:, 0] >= 0) & (p1[:, 1] >= 0)] = NOEPI
    return role


def _reference(oracle, imgs, pts):
    tracks, keep = _circular_reference(oracle, imgs, pts)
    pL0, pR0 = oracle.PyramidHandle(imgs[0]), oracle.PyramidHandle(imgs[1])
    _, st0 = oracle.lk_track(pL0, pR0, pts)
    role = _roles(tracks, keep, st0)
    role.setflags(write=False)
    return tracks, keep, role


@pytest.fixture(scope="module")
def scene(oracle):
    imgs = _frames()
    pts, intended = _points()
    ref = {"exact": _reference(oracle, imgs, pts.copy())}
    for name, (_, mode) in FLOAT_ORDERS.items():
        with accum_oracle(oracle, mode):
            ref[name] = _reference(oracle, imgs, pts.copy())
    return imgs, intended, ref


def _guard(intended, role):
    """Each role at least 8 times IN EVERY SLOT POSITION where the geometry put it, and a wave with all four: from the
    oracle's outputs alone.  Returns the first point of the first all-four-roles wave."""
    r = role.reshape(-1, 4)
    hit = (r == intended.reshape(-1, 4))
    for ro in range(4):
        n_role = int((role == ro).sum())
        assert n_role >= 8, (ro, n_role)
        for slot in range(4):
            assert int((hit[:, slot] & (r[:, slot] == ro)).sum()) >= 1, (ro, slot)
    full = np.flatnonzero(hit.all(axis=1))
    assert len(full) >= 1, "no wave holds all four roles"
    return 4 * int(full[0]), len(full)


def _accum_kw(pkg, accum):
    return {} if accum == "exact" else {"lk_accum": getattr(pkg, FLOAT_ORDERS[accum][0])}


@pytest.mark.parametrize("accum", ["exact"] + list(FLOAT_ORDERS))
def test_waves_of_four_roles(pkg, tc, scene, accum):
    imgs, intended, ref = scene
    tracks, keep, role = ref[accum]
    _, n_full = _guard(intended, role)
    idx = np.tile(np.arange(len(role)), REPEAT)
    assert len(idx) > 3 * 3072                  # four points per wave, wave w = points 4 w .. 4 w + 3
    kept = _check_circular(pkg, imgs, tracks, keep, idx, max_keypoints=16384, **_accum_kw(pkg, accum))
    assert kept == REPEAT * int((role == TRACKED).sum()) and n_full >= 8


@pytest.mark.parametrize("n", [1, 2, 3])
@pytest.mark.parametrize("accum", ["exact"] + list(FLOAT_ORDERS))
def test_first_points_of_a_four_role_wave_alone(pkg, tc, scene, accum, n):
    imgs, intended, ref = scene
    tracks, keep, role = ref[accum]
    first, _ = _guard(intended, role)
    _check_circular(pkg, imgs, tracks, keep, first + np.arange(n), max_keypoints=1024, **_accum_kw(pkg, accum))
