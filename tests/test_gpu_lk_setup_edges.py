"""Edges of the LK kernels' level set-up and of the weights an iteration hands to its slots (csrc/lk_common.h), on one 416 x 128
pair through svo_circular_match (and the first call alone through svo_lk_track, which also returns the status bytes),
against the oracle byte for byte in the exact order and the three float orders.

(a) Weights at their corners.  The fourth bilinear weight is formed from the other three, iw11 = 2^14 - iw00 - iw01 - iw10, and
    rides in the upper half of a packed weight word as a SIGNED 16-bit value: it is -1 when the three rounded weights add up to
    2^14 + 1.  The first iteration of the top level samples J at prevPt / S - 10 (S = the top level's scale), so points at
    S (n + f) put the fraction f straight into the weights: f = 0 (iw00 = 2^14, the others 0), 0.5, and the floats around 2^-15
    and 1 - 2^-15, where a product with 2^14 rounds to 0 or to 1.  A 416 x 128 frame has THREE levels (the fourth, 52 x 16,
    would not exceed the 21-pixel window), so S = 4 here, not 8.
(b) Near-degenerate patches.  The minEig test compares the numerator with a threshold instead of dividing, and the three A
    sums of a slot come out of one twelve-value reduce-scatter into the slot's own row.  A texture whose contrast rises
    from nothing to strong across the image puts a grid of points on both sides of the test.

A single pair runs in the latency shape: its points are spread over up to 3072 waves (2048 / 1536 in the float orders), one
per wave while they last -- only slot 0 would ever work.  Both point lists are therefore repeated to more than 3 x 3072
entries, a multiple of four: every wave then carries four points (slot = index % 4), and with an ODD number of distinct points
the k-th repeat shifts a point's slot by one, so every point meets every slot.  The oracle tracks the distinct points once.
"""
import numpy as np
import pytest

from test_gpu_lk_wave_mapping import FLOAT_ORDERS, H, W, _check_circular, _circular_reference, _dense_frames
from test_gpu_parity_lk_sse2 import accum_oracle

pytestmark = pytest.mark.gpu

W_BITS = 14
TOP_SCALE = 4                                                  # 416 x 128: levels 0..2 (checked against the oracle's pyramid below)
ORDERS = {"exact": (None, 0), **FLOAT_ORDERS}                 # lk_accum name -> (the package's constant, the oracle's mode)
LATENCY_WAVES = 3072                                           # waves of a single pair in lk_kernel's latency shape (the float orders: fewer)


@pytest.fixture(scope="module")
def tc():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU; the hot path has no CPU fallback"
    return torch


def whole_wave_index(m):
    """Indices into m distinct points that fill whole four-slot waves and put every point into every slot."""
    assert m % 2 == 1 and 4 * m > 3 * LATENCY_WAVES, m
    idx = np.arange(4 * m) % m
    slots = np.zeros((m, 4), bool)
    slots[idx, np.arange(4 * m) % 4] = True
    assert len(idx) % 4 == 0 and slots.all()
    return idx


def bilinear_weights(a, b):
    """csrc/lk_common.h bilinear_weights in numpy float32: iw = the integer that x + 1.5 * 2^23 leaves in the low mantissa
    bits = x rounded to nearest even; iw11 from the other three."""
    a, b = np.float32(a), np.float32(b)
    one, scale = np.float32(1), np.float32(1 << W_BITS)
    a1, b1, b0 = one - a, (one - b) * scale, b * scale
    magic = np.float32(12582912.0)

    def rounded(x):
        u = (x.astype(np.float32) + magic).astype(np.float32).view(np.uint32)
        return (u & 0xFFFF).astype(np.int64)
    iw00, iw01, iw10 = rounded(a1 * b1), rounded(a * b1), rounded(a1 * b0)
    return iw00, iw01, iw10, (1 << W_BITS) - iw00 - iw01 - iw10


def corner_points():
    """Points TOP_SCALE (n + f): every pair (fx, fy) of the fraction set at a grid of top-level positions n, plus one more point to
    make the count odd.  Returns the points and the weights of the first J sample of the top level."""
    def axis(ns):
        out = []
        for n in ns:
            S, eps = TOP_SCALE, TOP_SCALE * 2.0 ** -15                                 # f = 2^-15, 1 - 2^-15
            lo, hi = np.float32(S * n + eps), np.float32(S * n + S - eps)
            assert float(lo) == S * n + eps and float(hi) == S * n + S - eps
            out.append([np.float32(S * n), np.float32(S * n + S / 2),
                        np.nextafter(lo, np.float32(0)), lo, np.nextafter(lo, np.float32(1e9)),
                        np.nextafter(hi, np.float32(0)), hi, np.nextafter(hi, np.float32(1e9))])
        return np.asarray(out, np.float32)
    xs, ys = axis([8, 26, 44, 62, 80, 94]), axis([4, 8, 12, 16, 20, 24])
    pts = np.asarray([(x, y) for xr in xs for yr in ys for x in xr for y in yr], np.float32)
    pts = np.concatenate([pts, np.float32([[201.25, 63.75]])])
    # top level: nextPt = prevPt / S (exact), the J window corner is nextPt - 10 and its fraction the weights' (a, b)
    q = pts * np.float32(1.0 / TOP_SCALE) - np.float32(10)
    frac = q - np.floor(q)
    assert frac.dtype == np.float32
    return pts, bilinear_weights(frac[:, 0], frac[:, 1])


def contrast_ramp_frames():
    """Uniform byte noise, softened once, times a contrast that rises with the cube of x from 0 to 1: flat on the left (the 8-bit
    image is constant there), strong on the right; the right eye and the later frame are whole-pixel shifts."""
    rng = np.random.default_rng(21)
    n = rng.integers(0, 256, (H, W)).astype(np.float64) - 127.5
    n = (n + np.roll(n, 1, 0) + np.roll(n, 1, 1) + np.roll(n, (1, 1), (0, 1))) / 4
    ramp = (np.arange(W) / (W - 1.0)) ** 3
    left = np.clip(np.rint(128 + n * ramp[None, :]), 0, 255).astype(np.uint8)
    frames = []
    for t in range(2):
        l = np.roll(left, 2 * t, axis=1)
        frames.append((np.ascontiguousarray(l), np.ascontiguousarray(np.roll(l, -3, axis=1))))
    return frames


def ramp_points():
    xs = np.linspace(24.0, 392.0, 179)
    ys = np.linspace(18.0, 110.0, 13)
    pts = np.asarray([(x, y) for y in ys for x in xs], np.float32)
    assert len(pts) % 2 == 1
    return pts


def _references(oracle, imgs, pts):
    """Per accumulation order: the circular chain's reference and the first call's (points, status) on the distinct points."""
    ref = {}
    for name, (_, mode) in ORDERS.items():
        with accum_oracle(oracle, mode):
            first = oracle.lk_track(imgs[0], imgs[1], pts)
            ref[name] = (_circular_reference(oracle, imgs, pts.copy()), first)
        for a in first:
            a.setflags(write=False)
    return ref


@pytest.fixture(scope="module")
def corners(oracle):
    frames = _dense_frames(2)
    imgs = (frames[0][0], frames[0][1], frames[1][0], frames[1][1])
    assert 1 << (oracle.PyramidHandle(imgs[0]).nlevels - 1) == TOP_SCALE
    pts, (iw00, iw01, iw10, iw11) = corner_points()
    # the corners the case is about are in the list, before anything runs on the GPU
    assert int((iw11 == -1).sum()) >= 8, int((iw11 == -1).sum())
    assert int(((iw11 == 0) & (iw00 == 1 << W_BITS)).sum()) >= 8
    assert iw11.min() == -1 and iw11.max() > (1 << W_BITS) - 4 and ((iw00 == 4096) & (iw11 == 4096)).any()
    idx = whole_wave_index(len(pts))
    return imgs, idx, _references(oracle, imgs, pts)


@pytest.fixture(scope="module")
def ramp(oracle):
    frames = contrast_ramp_frames()
    imgs = (frames[0][0], frames[0][1], frames[1][0], frames[1][1])
    pts = ramp_points()
    idx = whole_wave_index(len(pts))
    ref = _references(oracle, imgs, pts)
    # from the oracle's status bytes alone: both outcomes of the level-0 degeneracy test occur, in every order
    for name, (_, (_, st)) in ref.items():
        assert int((st == 0).sum()) >= 32 and int((st == 1).sum()) >= 32, (name, int((st == 0).sum()), int((st == 1).sum()))
    return imgs, idx, ref


def _check(pkg, case, accum):
    imgs, idx, ref = case
    (tracks, keep), (want_next, want_st) = ref[accum]
    kw = {} if accum == "exact" else {"lk_accum": getattr(pkg, ORDERS[accum][0])}
    kept = _check_circular(pkg, imgs, tracks, keep, idx, max_keypoints=16384, **kw)
    assert kept > 0
    # the first call alone: every status byte and every output point, failed ones included
    ctx = pkg.Context(W, H, device=0, max_keypoints=16384, **kw)
    for s, im in enumerate(imgs[:2]):
        ctx.build_pyramid(s, im)
    got, st = ctx.lk_track(0, 1, np.ascontiguousarray(tracks[0][idx]))
    ctx.close()
    assert st.tobytes() == want_st[idx].tobytes()
    assert got.tobytes() == want_next[idx].tobytes()


@pytest.mark.parametrize("accum", list(ORDERS))
def test_weights_at_their_corners(pkg, tc, corners, accum):
    _check(pkg, corners, accum)


@pytest.mark.parametrize("accum", list(ORDERS))
def test_near_degenerate_patches(pkg, tc, ramp, accum):
    _check(pkg, ramp, accum)
