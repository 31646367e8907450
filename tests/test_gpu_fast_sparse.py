"""FAST from sparse tile records (fast.hip): Context.fast_detect against oracle.fast, the whole list of x, y, response and
the count, element for element (all-integer: the bar is BIT-EXACT).

Shapes.  The score kernel works on 64x32 tiles (64x16 before it) and the emit kernel on groups of 1024 (row, tile column)
counts, so the shapes go from one partial tile to several groups: widths and heights below, at and one past a tile, odd remainders, and one
full 1241x376 frame (20 x 376 = 7520 counts, eight groups, the last one partial).  A context refuses a side below 32 pixels
(svo_create; test_gpu_parity_frame_sizes.py pins that boundary), so a wanted side below it -- 7x7, 8x9, 63x16, 65x17 -- is
raised by whole tiles, which keeps its remainder in the last tile of either height: 7 -> 71 wide / 39 high, 8 -> 72,
9 -> 41, 16 -> 48, 17 -> 49.  32x32, the smallest frame a context takes, stands for "smaller than one tile both ways".

Contents: a flat image (no corner, every count byte still has to be written), uniform noise (dense: up to 115 corners per
64x16 tile at 333x77 with seed 3 and threshold 7, and plenty of equal scores, so strict NMS ties across tile borders), and
bright pixels on a 4-pixel lattice (every lattice point a corner, one common score, 64 per full tile)."""
import sys

import ctypes as C
import numpy as np
import pytest

from conftest import rand_image

pytestmark = pytest.mark.gpu

SHAPES = [(32, 32), (71, 39), (72, 41), (63, 48), (64, 64), (65, 49), (129, 33), (333, 77), (1241, 376)]
THRESHOLDS = (7, 20)


def lattice_image(h, w):
    img = np.full((h, w), 40, np.uint8)
    img[3::4, 3::4] = 200
    return img


@pytest.fixture(scope="module")
def tc():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU; the hot path has no CPU fallback"
    return torch


def _same(got, ref, what):
    assert len(got) == len(ref), (what, len(got), len(ref))
    for f in ("x", "y", "response"):
        assert np.array_equal(got[f], ref[f]), (what, f)
    assert got.tobytes() == ref.tobytes(), what


@pytest.mark.parametrize("w,h", SHAPES, ids=[f"{w}x{h}" for w, h in SHAPES])
def test_fast_sparse_matches_oracle(pkg, oracle, tc, w, h):
    cap = w * h
    c = pkg.Context(w, h, device=0, max_keypoints=cap)
    images = {"flat": np.full((h, w), 99, np.uint8), "noise": rand_image(h, w, 3, blocks=False), "lattice": lattice_image(h, w)}
    for name, img in images.items():
        dev = tc.from_numpy(img).cuda()                             # read in place: pitch = w, aligned only where w is
        for thr in THRESHOLDS:
            for nms in (True, False):
                ref = oracle.fast(img, thr, nms, cap=cap)
                if name == "flat":
                    assert len(ref) == 0
                elif name == "lattice" or thr == 7:
                    assert len(ref) > 0
                _same(c.fast_detect(dev, thr, nms, cap=cap), ref, (name, thr, nms, "device"))
                _same(c.fast_detect(img, thr, nms, cap=cap), ref, (name, thr, nms, "host"))
    c.close()


def test_reference_densities(oracle):
    """The figures the contents were chosen for (CPU only, cheap): they keep the records' bound in play."""
    kp = oracle.fast(rand_image(77, 333, 3, blocks=False), 7, True)
    per_tile = np.bincount((kp["y"].astype(int) // 16) * 6 + kp["x"].astype(int) // 64)
    assert per_tile.max() == 115
    kp = oracle.fast(lattice_image(77, 333), 7, True)
    assert len(np.unique(kp["response"])) == 1
    full = (kp["x"] >= 64) & (kp["x"] < 128) & (kp["y"] >= 16) & (kp["y"] < 32)
    assert full.sum() == 64
    x, y = np.meshgrid(np.arange(3, 333 - 3, 4), np.arange(3, 77 - 3, 4))
    assert len(kp) == x.size and np.array_equal(kp["x"], x.ravel()) and np.array_equal(kp["y"], y.ravel())


def test_strided_view_unaligned_pitch_and_pointer(pkg, oracle, tc):
    """A window of a larger device image: odd pitch, pointer off by 3 bytes -- the byte-staging branch of the score kernel."""
    w, h = 129, 33
    big = rand_image(h + 9, w + 8, 5, blocks=False)
    big[10:30, 20:90] = lattice_image(20, 70)
    view = big[6:6 + h, 3:3 + w]
    dview = tc.from_numpy(big).cuda()[6:6 + h, 3:3 + w]
    assert dview.stride(0) == w + 8 and dview.data_ptr() % 4 != 0 and (w + 8) % 4 != 0
    c = pkg.Context(w, h, device=0, max_keypoints=w * h)
    for thr in THRESHOLDS:
        for nms in (True, False):
            ref = oracle.fast(np.ascontiguousarray(view), thr, nms)
            assert len(ref) > 0
            _same(c.fast_detect(dview, thr, nms), ref, (thr, nms, "device view"))
            _same(c.fast_detect(view, thr, nms), ref, (thr, nms, "host view"))
    c.close()


def test_capacity_below_equal_and_above(pkg, oracle, tc):
    """n_out is the number found even above the capacity, a list that does not fit is an error, and one that just fits is
    complete -- for the context's own max_keypoints (what the emit kernel writes up to) and for the caller's array."""
    w, h = 129, 33
    b = sys.modules[pkg.__name__ + ".binding"]
    img = rand_image(h, w, 3, blocks=False)
    ref = oracle.fast(img, 7, True)
    n = len(ref)
    assert n > 64                                                   # max_keypoints may not go below 64

    def raw(c, cap):
        out = np.zeros(max(cap, 1), dtype=b.KP_DTYPE)
        got = C.c_int(-1)
        p, pitch, mem = c._img(img)
        rc = c.lib.svo_fast_detect(c.h, p, pitch, mem, 7, 1, C.c_void_p(out.ctypes.data), cap, C.byref(got))
        return rc, got.value, out

    for dev_cap in (n - 1, n, n + 1):
        c = pkg.Context(w, h, device=0, max_keypoints=dev_cap)
        rc, got, out = raw(c, n + 1)
        assert got == n, dev_cap
        if dev_cap < n:
            assert rc != 0
            with pytest.raises(pkg.SvoError):
                c.fast_detect(img, 7, True, cap=n + 1)
        else:
            assert rc == 0
            _same(out[:n], ref, dev_cap)
            assert not out[n:].view(np.uint8).any()
            for cap in (n - 1, n, n + 1):
                rc, got, out = raw(c, cap)
                assert got == n and (rc != 0) == (cap < n), (dev_cap, cap)
                if cap >= n:
                    _same(out[:n], ref, (dev_cap, cap))
        c.close()


def test_two_image_batch_counts(pkg, oracle, tc):
    """svo_track_batch runs FAST on both left images in one launch: the per-image offsets of records, counts and lists."""
    w, h = 129, 33
    L = np.stack([rand_image(h, w, 11), rand_image(h, w, 12, blocks=False)])
    R = np.stack([rand_image(h, w, 13), rand_image(h, w, 14)])
    n0, n1 = (len(oracle.fast(L[i], 20, True)) for i in (0, 1))
    assert n0 != n1 and min(n0, n1) > 0
    c = pkg.Context(w, h, device=0, max_batch=1, max_keypoints=w * h, fast_threshold=20)
    res = c.track_batch(tc.from_numpy(L).cuda(), tc.from_numpy(R).cuda())
    assert (int(res[0]["n_prev_kps"]), int(res[0]["n_cur_kps"])) == (n0, n1)
    c.close()
