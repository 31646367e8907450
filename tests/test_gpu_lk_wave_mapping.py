"""Which wave of lk_kernel tracks which four points is a pure re-mapping: whatever the workgroup shape (one, two or
four waves; the latency shape and the throughput shape are separate instantiations), the point count and the batch
size, every output byte is the oracle's.  The shapes are the smallest at which the mapping takes another path:

  * one pair (svo_circular_match: the latency shape, points spread over up to 3072 waves) with n around the wave
    (4 points) and the four-wave workgroup (16) boundaries, 64 +- 1, n == max_keypoints not a multiple of 4;
  * the same shape with more points than waves, so a wave carries 2, 3 and 4 points and finally loops over chunks
    (n > 4 * 3072) -- dense noise frames, points repeated where the frame has too few corners;
  * svo_track_batch of B pairs around the mapping's branches: B < 4 (latency shape, 3072 / B waves per item), B = 4, 7
    (plain order), 8 (one item per XCD), 9 and 17 (XCD-aware part + plain remainder);
  * svo_track_batch on the dense frames (> 3072 corners per frame): B = 1, 2, 3 give 2, 4 and 4 points per wave with
    a second chunk at B = 3; B = 4 is the throughput shape, whose 768 waves per item loop over chunks.

The item mapping and the per-item loop are one driver shared by lk_kernel and the float-order lk_sse2_kernel (csrc/lk_common.h),
so the one-pair and the batch cases run again with lk_accum = sse2, simd128 and sse2_legacy against the oracle in the matching
accumulation mode (single-wave workgroups, 2048 / 1536 waves in the latency shape).

The references are computed once per module and only read."""
import numpy as np
import pytest

from test_gpu_parity_lk_sse2 import accum_oracle
from test_gpu_parity_sequence import CHAIN_TIGHT, _check_record, _oracle_lk_sequence, _render, relfro

pytestmark = pytest.mark.gpu

W, H = 416, 128
DISPARITY, STEP = 3, 2          # whole-pixel shifts of the dense frames: right eye, and frame to frame
# lk_accum name -> (the package's constant, the oracle's accumulation mode)
FLOAT_ORDERS = {"sse2": ("LK_ACCUM_SSE2", 2), "simd128": ("LK_ACCUM_SIMD128", 4), "sse2_legacy": ("LK_ACCUM_SSE2_LEGACY", 3)}


@pytest.fixture(scope="module")
def tc():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU; the hot path has no CPU fallback"
    return torch


def _circular_reference(oracle, imgs, pts):
    """(the four tracks of every point, keep mask) of the chain L1 -> R1 -> R2 -> L2 -> L1' on imgs = (L0, R0, L1, R1)."""
    pL0, pR0, pL1, pR1 = [oracle.PyramidHandle(x) for x in imgs]
    t1r, s1 = oracle.lk_track(pL0, pR0, pts)
    t2r, s2 = oracle.lk_track(pR0, pR1, t1r)
    t2l, s3 = oracle.lk_track(pR1, pL1, t2r)
    ret, s4 = oracle.lk_track(pL1, pL0, t2l)
    keep, m = oracle.circular_keep(pts, t1r, t2r, t2l, ret, s1, s2, s3, s4, 3.0)
    for a in (pts, t1r, t2r, t2l, keep):
        a.setflags(write=False)
    return (pts, t1r, t2r, t2l), keep.astype(bool)


def _check_circular(pkg, imgs, tracks, keep, idx, max_keypoints, **ctx_kw):
    """svo_circular_match on the points tracks[0][idx] == the oracle's rows idx that it keeps, in order, byte for byte."""
    ctx = pkg.Context(W, H, device=0, max_keypoints=max_keypoints, **ctx_kw)
    for s, im in enumerate(imgs):
        ctx.build_pyramid(s, im)
    got = ctx.circular_match((0, 1, 2, 3), np.ascontiguousarray(tracks[0][idx]))
    k = keep[idx]
    assert got[0].shape[0] == int(k.sum())
    for g, r in zip(got, tracks):
        assert g.tobytes() == r[idx][k].tobytes()
    ctx.close()
    return int(k.sum())


# ---- one pair, few points -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sparse(oracle, small_seq):
    seq, frames = small_seq
    imgs = (frames[0][0], frames[0][1], frames[1][0], frames[1][1])
    kp = oracle.fast(imgs[0])
    pts = np.stack([kp["x"], kp["y"]], 1).astype(np.float32)
    assert len(pts) >= 67
    return imgs, _circular_reference(oracle, imgs, pts)


@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, 15, 16, 17, 63, 64, 65])
def test_first_n_corners_of_one_pair(pkg, tc, sparse, n):
    """Partial waves, waves without points, n_fixed: the first n oracle FAST corners."""
    imgs, (tracks, keep) = sparse
    _check_circular(pkg, imgs, tracks, keep, np.arange(n), max_keypoints=1024)


@pytest.fixture(scope="module")
def sparse_float(oracle, sparse):
    """The same corners through the oracle in each float accumulation order."""
    imgs, (tracks, _) = sparse
    ref = {}
    for name, (_, mode) in FLOAT_ORDERS.items():
        with accum_oracle(oracle, mode):
            ref[name] = _circular_reference(oracle, imgs, tracks[0])
    return ref


@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, 15, 16, 17, 63, 64, 65])
@pytest.mark.parametrize("accum", list(FLOAT_ORDERS))
def test_first_n_corners_of_one_pair_float_order(pkg, tc, sparse, sparse_float, accum, n):
    """The same partial waves through lk_sse2_kernel: the shared driver under the float-order call."""
    imgs, (exact, _) = sparse
    tracks, keep = sparse_float[accum]
    kept = _check_circular(pkg, imgs, tracks, keep, np.arange(n), max_keypoints=1024, lk_accum=getattr(pkg, FLOAT_ORDERS[accum][0]))
    if n == 65:
        # the mode was in force: every track array of these points differs from the exact order's, and points survive
        assert kept > 0
        for t, e in zip(tracks[1:], exact[1:]):
            assert t[:n].tobytes() != e[:n].tobytes()


def test_n_equals_capacity_not_a_multiple_of_four(pkg, tc, sparse):
    imgs, (tracks, keep) = sparse
    assert _check_circular(pkg, imgs, tracks, keep, np.arange(67), max_keypoints=67) > 0


# ---- dense frames: more points than waves ---------------------------------------------------------------------
def _dense_frames(n_frames):
    """Uniform byte noise, the right eye and the later frames as whole-pixel shifts of it (a fronto-parallel plane seen
    by a rig that moves sideways), so tracks survive all four calls."""
    base = np.random.default_rng(7).integers(0, 256, (H, W), dtype=np.uint8)
    out = []
    for t in range(n_frames):
        left = np.roll(base, STEP * t, axis=1)
        out.append((np.ascontiguousarray(left), np.ascontiguousarray(np.roll(left, -DISPARITY, axis=1))))
    return out


@pytest.fixture(scope="module")
def dense(oracle):
    frames = _dense_frames(5)
    imgs = (frames[0][0], frames[0][1], frames[1][0], frames[1][1])
    kp = oracle.fast(imgs[0])
    pts = np.stack([kp["x"], kp["y"]], 1).astype(np.float32)
    tracks, keep = _circular_reference(oracle, imgs, pts)
    assert len(pts) > 3072 and 2 * int(keep.sum()) >= len(pts), (len(pts), int(keep.sum()))
    return frames, imgs, tracks, keep


@pytest.mark.parametrize("n", [None, 7001, 13001])
def test_one_dense_pair_more_points_than_waves(pkg, tc, dense, n):
    """All corners of the frame (> 3072: two points per wave), 7001 points (three) and 13001 (four, and the waves loop
    over a second chunk); beyond the frame's corners the points repeat, and so does the reference."""
    frames, imgs, tracks, keep = dense
    n_corners = len(tracks[0])
    idx = np.arange(n_corners if n is None else n) % n_corners
    assert _check_circular(pkg, imgs, tracks, keep, idx, max_keypoints=16384) >= len(idx) // 2


@pytest.fixture(scope="module")
def dense_batch_ref(oracle, synth, dense):
    frames = dense[0]
    seq = synth.StereoSequence(width=W, height=H, n_frames=2, seed=7)        # its projection matrices only
    ref = _oracle_lk_sequence(oracle, seq, frames)
    assert all(r[0]["n_prev_kps"] > 3072 and 2 * r[0]["n_tracked"] >= r[0]["n_prev_kps"] for r in ref)
    return seq, frames, ref


def _batch(pkg, tc, seq, frames, ref, **ctx_kw):
    """svo_track_batch on the frames: records and chained poses at the bars of test_gpu_parity_sequence._check_batch,
    then the matched tracks and the inlier mask of every pair byte for byte."""
    B = len(frames) - 1
    P1, P2 = seq.proj()
    c = pkg.Context(W, H, device=0, P1=P1, P2=P2, max_batch=B, **ctx_kw)
    L = tc.stack([tc.from_numpy(f[0]) for f in frames]).cuda()
    R = tc.stack([tc.from_numpy(f[1]) for f in frames]).cuda()
    res = c.track_batch(L, R)
    worst = 0.0
    for p, (r, X, pnp, pose) in enumerate(ref[:B]):
        _check_record(res[p], r, pnp)
        worst = max(worst, relfro(res[p]["pose"].reshape(4, 4), pose))
        got = c.batch_tracks(p, cap=8192)
        for g, want in zip(got[:4], r["tracks"]):
            assert g.tobytes() == want.tobytes(), p
        assert got[4].tobytes() == pnp["mask"].tobytes(), p
    assert worst <= CHAIN_TIGHT, worst
    c.close()


@pytest.mark.parametrize("B", [1, 2, 3, 4])
def test_dense_batches_loop_over_chunks(pkg, tc, dense_batch_ref, B):
    seq, frames, ref = dense_batch_ref
    _batch(pkg, tc, seq, frames[:B + 1], ref, max_keypoints=8192)


# ---- batch sizes around the mapping's branches ------------------------------------------------------------------
@pytest.fixture(scope="module")
def seq17(oracle, synth, tc):
    seq, frames = _render(synth, tc, W, H, 18, 23)
    return seq, frames, _oracle_lk_sequence(oracle, seq, frames)


@pytest.mark.parametrize("B", [1, 2, 3, 4, 7, 8, 9, 17])
def test_batch_sizes_around_the_xcd_mapping(pkg, tc, seq17, B):
    seq, frames, ref = seq17
    _batch(pkg, tc, seq, frames[:B + 1], ref)


@pytest.fixture(scope="module")
def seq17_float(oracle, seq17):
    """The first nine pairs of seq17 through the oracle in each float accumulation order."""
    seq, frames, _ = seq17
    ref = {}
    for name, (_, mode) in FLOAT_ORDERS.items():
        with accum_oracle(oracle, mode):
            ref[name] = _oracle_lk_sequence(oracle, seq, frames[:10])
    return ref


@pytest.mark.parametrize("B", [1, 3, 4, 8, 9])
@pytest.mark.parametrize("accum", list(FLOAT_ORDERS))
def test_batch_sizes_around_the_xcd_mapping_float_order(pkg, tc, seq17, seq17_float, accum, B):
    """Latency shape (B = 1, 3), plain order (4), one item per XCD (8), XCD-aware part + plain remainder (9) through
    lk_sse2_kernel."""
    seq, frames, _ = seq17
    _batch(pkg, tc, seq, frames[:B + 1], seq17_float[accum], lk_accum=getattr(pkg, FLOAT_ORDERS[accum][0]))
