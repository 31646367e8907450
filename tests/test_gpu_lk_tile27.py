"""lk_kernel's slot tiles are 27 columns wide (csrc/lk.hip ExactTile): the staged source dwords carry 28, and the last one is
neither stored nor read.  Every case below compares with oracle.lk_track / oracle.circular_keep byte for byte on 416 x 128
frames (three pyramid levels: scales 1, 2, 4).

(a) I tile, column 26.  The I tile starts at the 4-byte aligned column at or left of ipx - 1, so a lane's last column is
    offI + 7 * 2 + 9 with offI = (ipx - 1) mod 4: column 26 is read only when offI = 3, and a stray store of column 27 would
    land in the NEXT slot's column 0, which that slot reads only when its offI = 0.  The points therefore come in groups of
    four (one wave) whose offI are four different values at EVERY level, at integer and half-pixel x, on byte noise (every
    column of every tile differs).  A single pair runs in the latency shape, which hands a wave one point while there are
    more waves than points: n = 4 and n = 8 points run as they are (one point per wave, slot 0), and again repeated to more
    than 3 x 3072 entries, where wave k carries the points 4 k .. 4 k + 3 in its slots 0 .. 3.  Once more with the first three
    points of every group outside the image: slot 3 alone works, at the end of the wave's LDS region.
(b) J tile, drift in x.  A window may drift 3 columns left and 2 columns right of where its tile was staged (5 - 3); one more
    re-stages.  Single calls ctx.lk_track(0, 1, pts) on a smooth texture shifted by whole pixels: x by +-16, +-24, +-32, +-40
    (+-4, 6, 8, 10 columns at the top level, so every window passes the columns that stay AND the one that re-stages, in both
    directions, several times for the larger shifts; half of that at level 1 where the top level fell short), y by +-16 and
    +-24 (the y rule: 3 rows either way).  The texture is built so that the ORACLE ALONE solves these cases: status 1 and
    within 0.5 px of the true shift for at least 80 % of the points at every shift, asserted on the CPU before anything runs
    on the GPU -- a window that loses its way compares garbage with garbage.
(c) The chain.  svo_circular_match and svo_track_batch on dense noise frames (more than 3072 corners) whose right eye and
    later frames are whole-pixel shifts: 3 and 2 px, and 24 and 16 px.  B = 1 is the latency shape (four-wave workgroups),
    B = 4 and 8 the throughput shape (single-wave workgroups: slot 3's tile ends the workgroup's LDS).  The float orders sse2
    and sse2_legacy (lk_sse2_kernel: its 26-column tiles are unchanged) run once each against the oracle in their mode.

The references are computed once per module and only read."""
import numpy as np
import pytest

from test_gpu_lk_setup_edges import LATENCY_WAVES
from test_gpu_lk_wave_mapping import FLOAT_ORDERS, H, W, _batch, _check_circular, _circular_reference
from test_gpu_parity_lk_sse2 import accum_oracle
from test_gpu_parity_sequence import _oracle_lk_sequence

pytestmark = pytest.mark.gpu

N_LEVELS = 3
HALF_WIN = 10
X_SHIFTS = (16, -16, 24, -24, 32, -32, 40, -40)
Y_SHIFTS = (16, -16, 24, -24)


@pytest.fixture(scope="module")
def tc():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU; the hot path has no CPU fallback"
    return torch


def _noise_frames(n_frames, disparity, step):
    """Uniform byte noise; the right eye and the later frames are whole-pixel shifts of it."""
    base = np.random.default_rng(7).integers(0, 256, (H, W), dtype=np.uint8)
    out = []
    for t in range(n_frames):
        left = np.roll(base, step * t, axis=1)
        out.append((np.ascontiguousarray(left), np.ascontiguousarray(np.roll(left, -disparity, axis=1))))
    return out


# ---- (a) I tile, column 26 --------------------------------------------------------------------------------------
def off_i(x):
    """(ipx - 1) mod 4 of the points x at every level: csrc/lk_common.h request_I / i_tile_x0 in float32."""
    x = np.asarray(x, np.float32)
    ipx = [np.floor(x * np.float32(0.5 ** l) - np.float32(HALF_WIN)).astype(np.int64) for l in range(N_LEVELS)]
    return np.stack([(i - 1) % 4 for i in ipx])                        # (level, point)


def residue_groups():
    """24 groups of four points: x drawn from the half-pixel grid (seeded), a draw kept where the four offI of the group differ
    at every level; y differs inside a group and takes integer and half-pixel values."""
    rng = np.random.default_rng(3)
    grid = np.arange(40.0, 376.0, 0.5)
    groups = []
    while len(groups) < 24:
        xs = rng.choice(grid, 4, replace=False)
        if all(len(set(r)) == 4 for r in off_i(xs)):
            i = len(groups)
            ys = 30.0 + 9.5 * ((np.arange(4) + i) % 4) + 3.0 * (i % 7)
            groups.append(np.stack([xs, ys], 1))
    return np.asarray(groups, np.float32)                               # (group, slot, xy)


def tile_over_waves(pts):
    """Whole groups of four, repeated to more than 3 x 3072 entries: the latency shape then gives wave k the points 4 k .. 4 k + 3."""
    assert len(pts) % 4 == 0
    reps = (3 * LATENCY_WAVES) // len(pts) + 1
    return np.arange(reps * len(pts)) % len(pts)


@pytest.fixture(scope="module")
def residues(oracle):
    frames = _noise_frames(2, 3, 2)
    imgs = (frames[0][0], frames[0][1], frames[1][0], frames[1][1])
    assert oracle.PyramidHandle(imgs[0]).nlevels == N_LEVELS
    groups = residue_groups()
    assert len(groups) >= 8
    flat = groups.reshape(-1, 2)
    r = off_i(flat[:, 0])
    # every residue at every level, at integer and at half-pixel x; slot 3 reads column 26 and slot 0 follows an offI = 3
    # neighbour's would-be column 27 in some group, at every level
    half = flat[:, 0] != np.floor(flat[:, 0])
    for l in range(N_LEVELS):
        assert set(r[l][half]) == {0, 1, 2, 3} and set(r[l][~half]) == {0, 1, 2, 3}, l
        per_group = r[l].reshape(-1, 4)
        assert (per_group[:, 3] == 3).any() and ((per_group[:, :3] == 3) & (per_group[:, 1:] == 0)).any(), l
    # the same groups with slots 0..2 outside the image (negative x: the point is tracked nowhere and rejected)
    lone = groups.copy()
    lone[:, :3, 0] = -50.0 - lone[:, :3, 0]
    cases = {}
    for name, pts in (("groups", flat), ("slot3", lone.reshape(-1, 2))):
        pts = np.ascontiguousarray(pts, np.float32)
        first = oracle.lk_track(imgs[0], imgs[1], pts)
        for a in first:
            a.setflags(write=False)
        cases[name] = (_circular_reference(oracle, imgs, pts.copy()), first)
    (_, keep), (_, st) = cases["groups"]
    assert st.all() and keep.sum() * 10 >= 9 * len(keep)                # the points are tracked: the patches matter
    (_, keep), (_, st) = cases["slot3"]
    assert not st.reshape(-1, 4)[:, :3].any() and st.reshape(-1, 4)[:, 3].all() and not keep.reshape(-1, 4)[:, :3].any()
    return imgs, cases


def _check_points(pkg, imgs, case, idx):
    """The circular chain and the first call alone (every status byte and output point) on the points tracks[0][idx]."""
    (tracks, keep), (want_next, want_st) = case
    kept = _check_circular(pkg, imgs, tracks, keep, idx, max_keypoints=16384)
    ctx = pkg.Context(W, H, device=0, max_keypoints=16384)
    for s, im in enumerate(imgs[:2]):
        ctx.build_pyramid(s, im)
    got, st = ctx.lk_track(0, 1, np.ascontiguousarray(tracks[0][idx]))
    ctx.close()
    assert st.tobytes() == want_st[idx].tobytes()
    assert got.tobytes() == want_next[idx].tobytes()
    return kept


@pytest.mark.parametrize("n", [4, 8])
@pytest.mark.parametrize("four_per_wave", [False, True])
def test_i_tile_column_26(pkg, tc, residues, n, four_per_wave):
    imgs, cases = residues
    idx = np.arange(n)                                                  # the first group, the first two
    assert _check_points(pkg, imgs, cases["groups"], tile_over_waves(idx) if four_per_wave else idx) > 0


def test_i_tile_column_26_all_groups(pkg, tc, residues):
    """All groups in one launch: neighbouring waves of a four-wave workgroup carry different groups."""
    imgs, cases = residues
    n = len(cases["groups"][1][0])
    assert _check_points(pkg, imgs, cases["groups"], tile_over_waves(np.arange(n))) > 0


def test_only_slot_3_live(pkg, tc, residues):
    imgs, cases = residues
    n = len(cases["slot3"][1][0])
    kept = _check_points(pkg, imgs, cases["slot3"], tile_over_waves(np.arange(n)))
    assert kept * 4 * 10 >= 9 * len(tile_over_waves(np.arange(n)))      # the fourth points survive the chain


# ---- (b) J tile, drift in x ---------------------------------------------------------------------------------------
def smooth_texture():
    """Plane waves of five octaves (wavelengths 208 .. 13 px, amplitudes falling), whole cycles over the frame so that
    np.roll is a true shift.  The long waves carry the top level over 10 columns; the short ones fix the last half pixel."""
    rng = np.random.default_rng(7)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    t = np.zeros((H, W))
    for lam, amp in zip((208, 104, 52, 26, 13), (1.0, 1.0, 0.7, 0.5, 0.3)):
        for _ in range(6):
            th, ph = rng.uniform(0, np.pi), rng.uniform(0, 2 * np.pi)
            kx, ky = np.rint(W / lam * np.cos(th)), np.rint(H / lam * np.sin(th))
            t += amp * np.cos(2 * np.pi * (kx * x / W + ky * y / H) + ph)
    return np.clip(np.rint(128 + 120 * t / np.abs(t).max()), 0, 255).astype(np.uint8)


def drift_points():
    xs, ys = np.arange(64.0, 352.0, 12.5), np.arange(40.0, 90.0, 8.25)
    pts = np.asarray([(x, y) for y in ys for x in xs] + [(201.25, 63.75)], np.float32)
    assert len(pts) % 2 == 1
    return pts


def every_slot_index(m):
    """Indices into m distinct points (m odd) that fill whole four-slot waves in the latency shape and put every point into
    every slot: a repeat shifts a point's slot by m mod 4, an odd number."""
    reps = 4 * ((3 * LATENCY_WAVES) // (4 * m) + 1)
    idx = np.arange(reps * m) % m
    slots = np.zeros((m, 4), bool)
    slots[idx, np.arange(len(idx)) % 4] = True
    assert m % 2 == 1 and len(idx) > 3 * LATENCY_WAVES and len(idx) % 4 == 0 and slots.all()
    return idx


@pytest.fixture(scope="module")
def drift(oracle):
    img = smooth_texture()
    pts = drift_points()
    ref = {}
    for axis, shifts in ((1, X_SHIFTS), (0, Y_SHIFTS)):
        for s in shifts:
            nxt = np.ascontiguousarray(np.roll(img, s, axis=axis))
            got, st = oracle.lk_track(img, nxt, pts)
            true = pts.copy()
            true[:, 1 - axis] += s
            solved = (st == 1) & (np.abs(got - true).max(1) < 0.5)
            # the condition on the texture, from the oracle alone
            assert solved.mean() >= 0.8, (axis, s, float(solved.mean()))
            got.setflags(write=False); st.setflags(write=False)
            ref[(axis, s)] = (nxt, got, st)
    return img, pts, every_slot_index(len(pts)), ref


@pytest.mark.parametrize("axis,shift", [(1, s) for s in X_SHIFTS] + [(0, s) for s in Y_SHIFTS])
def test_j_window_drift(pkg, tc, drift, axis, shift):
    img, pts, idx, ref = drift
    nxt, want, want_st = ref[(axis, shift)]
    ctx = pkg.Context(W, H, device=0, max_keypoints=16384)
    ctx.build_pyramid(0, img)
    ctx.build_pyramid(1, nxt)
    got, st = ctx.lk_track(0, 1, np.ascontiguousarray(pts[idx]))        # four points per wave, every point in every slot
    one, st1 = ctx.lk_track(0, 1, pts)                                  # one point per wave
    ctx.close()
    assert st.tobytes() == want_st[idx].tobytes() and got.tobytes() == want[idx].tobytes()
    assert st1.tobytes() == want_st.tobytes() and one.tobytes() == want.tobytes()


# ---- (c) the chain ------------------------------------------------------------------------------------------------
SHIFTS = {"3-2": (3, 2), "24-16": (24, 16)}                             # right-eye and frame-to-frame shift, px


@pytest.fixture(scope="module")
def chain(oracle, synth):
    seq = synth.StereoSequence(width=W, height=H, n_frames=2, seed=7)   # its projection matrices only
    out = {}
    for name, (disparity, step) in SHIFTS.items():
        frames = _noise_frames(9, disparity, step)
        imgs = (frames[0][0], frames[0][1], frames[1][0], frames[1][1])
        kp = oracle.fast(imgs[0])
        pts = np.stack([kp["x"], kp["y"]], 1).astype(np.float32)
        assert len(pts) > 3072
        out[name] = (frames, imgs, _circular_reference(oracle, imgs, pts), _oracle_lk_sequence(oracle, seq, frames))
    # the small shifts keep most tracks through all four calls
    _, _, (_, keep), _ = out["3-2"]
    assert 2 * int(keep.sum()) >= len(keep)
    return seq, out


@pytest.mark.parametrize("shifts", list(SHIFTS))
def test_circular_match_dense(pkg, tc, chain, shifts):
    """One pair, all corners (two points per wave) and 13001 points (four per wave, a second chunk)."""
    _, (frames, imgs, (tracks, keep), _) = chain[0], chain[1][shifts]
    n_corners = len(tracks[0])
    for n in (n_corners, 13001):
        _check_circular(pkg, imgs, tracks, keep, np.arange(n) % n_corners, max_keypoints=16384)


@pytest.mark.parametrize("B", [1, 4, 8])
@pytest.mark.parametrize("shifts", list(SHIFTS))
def test_track_batch_dense(pkg, tc, chain, shifts, B):
    seq, cases = chain
    frames, _, _, ref = cases[shifts]
    _batch(pkg, tc, seq, frames[:B + 1], ref, max_keypoints=8192)


@pytest.fixture(scope="module")
def chain_float(oracle, chain):
    """The 3 / 2 px frames through the oracle in the two float accumulation orders."""
    seq, cases = chain
    frames, imgs, (tracks, _), _ = cases["3-2"]
    ref = {}
    for name in ("sse2", "sse2_legacy"):
        with accum_oracle(oracle, FLOAT_ORDERS[name][1]):
            ref[name] = (_circular_reference(oracle, imgs, tracks[0].copy()), _oracle_lk_sequence(oracle, seq, frames[:5]))
    return ref


@pytest.mark.parametrize("accum", ["sse2", "sse2_legacy"])
def test_float_orders_unchanged(pkg, tc, chain, chain_float, accum):
    seq, cases = chain
    frames, imgs, _, _ = cases["3-2"]
    (tracks, keep), ref = chain_float[accum]
    kw = {"lk_accum": getattr(pkg, FLOAT_ORDERS[accum][0])}
    assert _check_circular(pkg, imgs, tracks, keep, np.arange(len(tracks[0])), max_keypoints=16384, **kw) > 0
    _batch(pkg, tc, seq, frames[:5], ref, max_keypoints=8192, **kw)
