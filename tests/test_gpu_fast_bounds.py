"""FAST's sparse records at their record, group and batch bounds (fast.hip, fast_scratch.h): Context.fast_detect against
oracle.fast on the inputs of tests/_fast_cases.py -- the whole list of x, y, response and the count, byte for byte, through
the host-image and the device-image path (all-integer: the bar is BIT-EXACT) -- and the two pipeline tests on what the
fused entry points show: the counts and the result records.  tests/test_fast_cases.py shows on the CPU that every input
reaches the bound it is here for.

  records : 64 one-byte records without NMS and 32 two-byte records with it fill a tile row's 64 bytes exactly; the last
            one (rank 63 / rank 31) must stay inside them and the count byte must hold 64 / 32        test_saturated_records
  groups  : the emit kernel serves 1024 count bytes per workgroup, four per thread; the last dword is masked and the last
            group publishes n_out, corners or not                                                      test_emit_group_edges
  thr     : thr + 1 == 256 in the packed quick test, the clamp of svo_fast_detect, scores of 254 in a record's high
            byte and the score of 0 that is no keypoint                                                test_threshold_extremes
  scratch : records and counts are never cleared between calls                                        test_stale_scratch
  batch   : several groups AND several images; an image over capacity between images under it
                                                test_multi_group_batch_counts, test_lk_capacity_overflow_inside_a_batch"""
import numpy as np
import pytest

import _fast_cases as fc
from conftest import rand_image
from test_gpu_fast_sparse import _same

pytestmark = pytest.mark.gpu

W, H = 135, 39
NINE = tuple(range(3, 36, 4))


@pytest.fixture(scope="module")
def tc():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU; the hot path has no CPU fallback"
    return torch


def _both(c, oracle, tc, img, thr, nms, what, cap=None):
    """fast_detect on the device image (read in place) and on the host image (staged), each against the oracle."""
    cap = cap or c.width * c.height
    ref = oracle.fast(img, thr, nms, cap=cap)
    dev = tc.from_numpy(img).cuda()
    _same(c.fast_detect(dev, thr, nms, cap=cap), ref, (what, thr, nms, "device"))
    _same(c.fast_detect(img, thr, nms, cap=cap), ref, (what, thr, nms, "host"))
    return ref


SATURATED = [
    # id, (w, h), rows, builder arguments, {thr: saturated tile columns}
    ("y3", (W, H), (3,), {}, {0: (1,), 7: (1,)}),
    ("y19", (W, H), (19,), {}, {0: (1,), 7: (1,)}),
    ("y31", (W, H), (31,), {}, {0: (1,), 7: (1,)}),
    ("y35", (W, H), (35,), {}, {0: (1,), 7: (1,)}),
    ("nine", (W, H), NINE, {}, {0: (1,), 7: (1,)}),
    ("199-clipped", (199, 39), (19,), dict(x_hi=191), {0: (1,), 7: (1,)}),
    ("199-both", (199, 39), (19,), dict(x_hi=191, steps=(5, 6)), {0: (1, 2), 7: ()}),
    ("199-col2", (199, 39), (19,), dict(x_lo=125, x_hi=191), {0: (2,), 7: (2,)}),
]


@pytest.mark.parametrize("case", SATURATED, ids=[s[0] for s in SATURATED])
def test_saturated_records(pkg, oracle, tc, case):
    """Tile rows at the bound of their records: 64 corners without NMS, 32 survivors with it, in one tile column, in two
    side by side and beside a column with a few live records (the three 199x39 images: test_fast_cases.py says why three),
    on the first testable row, either side of the tile-row border and on nine rows of one frame."""
    _, (w, h), rows, kw, saturated = case
    img = fc.staircase_rows(w, h, rows, **kw)
    c = pkg.Context(w, h, device=0, max_keypoints=w * h)
    for thr in (0, 7):
        for nms in (True, False):
            counts = fc.per_tile_row(oracle.fast(img, thr, nms, cap=w * h), w, h)
            for y0 in rows:
                for tx in saturated[thr]:
                    assert counts[y0, tx] == (32 if nms else 64), (y0, tx, thr, nms)
            assert counts.max() <= (32 if nms else 64)
            ref = _both(c, oracle, tc, img, thr, nms, case[0])
            assert len(ref) > 0
    c.close()


@pytest.mark.parametrize("w,h", fc.EMIT_SHAPES, ids=[f"{w}x{h}" for w, h in fc.EMIT_SHAPES])
def test_emit_group_edges(pkg, oracle, tc, w, h):
    """A total of exactly one group, a last group of one dead row, totals of 1, 2 and 3 modulo 4 in a second group, one
    tile column (a thread's four counts are four rows) and three; then a flat image on the same context: every count
    byte is rewritten to 0 and the last group publishes n_out = 0 over the dense frame's count."""
    img = fc.emit_image(w, h)
    flat = np.full((h, w), 99, np.uint8)
    c = pkg.Context(w, h, device=0, max_keypoints=w * h)
    for thr in (7, 20):
        for nms in (True, False):
            ref = _both(c, oracle, tc, img, thr, nms, "noise")
            assert len(ref) > 1024
            assert len(_both(c, oracle, tc, flat, thr, nms, "flat")) == 0
    c.close()


def test_threshold_extremes(pkg, oracle, tc):
    """thr 255 (thr + 1 == 256 in the packed 16-bit quick test), thresholds outside 0 .. 255 (clamped by svo_fast_detect as
    by the oracle), responses of 254 in the record's high byte, and the corner whose score is 0: a keypoint without NMS,
    none with it."""
    w, h = 71, 39
    c = pkg.Context(w, h, device=0, max_keypoints=w * h)
    lat = fc.lattice(w, h, 0, 255)
    one = fc.minus_one(w, h, 35, 19)
    noise = rand_image(h, w, 3, blocks=False)
    for nms in (True, False):
        for thr in (-5, 0, 1, 127, 128, 254, 255, 300):
            ref = _both(c, oracle, tc, lat, thr, nms, "lattice")
            assert len(ref) == (153 if thr < 255 else 0)
            assert thr >= 255 or (ref["response"] == (254 if nms else 0)).all()
        for thr in (0, 1):
            ref = _both(c, oracle, tc, one, thr, nms, "minus one")
            assert len(ref) == (1 if thr == 0 and not nms else 0)
        for thr in (0, 1, 128):
            assert len(_both(c, oracle, tc, noise, thr, nms, "noise")) > 0
    c.close()


def test_stale_scratch(pkg, oracle, tc):
    """One context, no clearing in between: two-byte records, then one-byte records over the rows just saturated, a flat
    frame after a dense one, noise over both, and a lone corner of score 0; the first call again at the end gives its
    first result."""
    c = pkg.Context(W, H, device=0, max_keypoints=W * H)
    stairs = fc.staircase_rows(W, H, NINE)
    flat = np.full((H, W), 99, np.uint8)
    calls = [("stairs", stairs, 7, True), ("stairs", stairs, 7, False), ("flat", flat, 7, True),
             ("noise", rand_image(H, W, 3, blocks=False), 7, True), ("stairs", stairs, 7, False), ("flat", flat, 7, False),
             ("minus one", fc.minus_one(W, H, 67, 19), 0, True)]
    first = c.fast_detect(stairs, 7, True, cap=W * H)
    assert len(first) == 9 * 35
    for step, (name, img, thr, nms) in enumerate(calls):
        ref = _both(c, oracle, tc, img, thr, nms, (step, name))
        assert (len(ref) > 0) == (name in ("stairs", "noise"))
    again = c.fast_detect(stairs, 7, True, cap=W * H)
    assert again.tobytes() == first.tobytes()
    c.close()


def test_multi_group_batch_counts(pkg, oracle, tc):
    """192x345: 1035 counts, two emit groups per image -- in svo_track_batch's launch over two and then one image
    (blockIdx.y, rowcount_stride and the 16-byte `before` loads of the second group), and online frame by frame."""
    w, h = 192, 345
    L = [rand_image(h, w, s, blocks=False) for s in (2, 3, 4)]
    R = [rand_image(h, w, s, blocks=False) for s in (12, 13, 14)]
    refs = [oracle.fast(img, 20, True, cap=w * h) for img in L]
    n = [len(r) for r in refs]
    assert len(set(n)) == 3 and min(n) > 1024
    assert all(fc.per_group(r, w, h)[1] > 0 for r in refs)          # the second group of every image has corners to place
    c = pkg.Context(w, h, device=0, max_batch=2, max_keypoints=w * h, fast_threshold=20)
    res = c.track_batch(tc.from_numpy(np.stack(L)).cuda(), tc.from_numpy(np.stack(R)).cuda())
    assert [(int(r["n_prev_kps"]), int(r["n_cur_kps"])) for r in res] == [(n[0], n[1]), (n[1], n[2])]
    c.close()
    c = pkg.Context(w, h, device=0, max_batch=2, max_keypoints=w * h, fast_threshold=20)
    got = []
    for l, r in zip(L, R):
        _, rec = c.add_frame(l, r)
        got.append((int(rec["n_prev_kps"]), int(rec["n_cur_kps"])))
    assert got == [(0, n[0]), (n[0], n[1]), (n[1], n[2])]
    _same(c.frame_keypoints(cap=w * h), refs[2], "frame_keypoints after the last add_frame")
    c.close()


def _chain_step(pose, rec):
    """finalize_chain_kernel: pose * T_rel_inv for a pair that is ok, the pose unchanged for one that failed."""
    return pose @ rec["T_rel_inv"].reshape(4, 4) if int(rec["ok"]) else pose


@pytest.mark.parametrize("select", ["all", "keep_strongest", "buckets"])
def test_lk_capacity_overflow_inside_a_batch(pkg, oracle, tc, small_seq, select):
    """A frame with more corners than max_keypoints between clean frames of one svo_track_batch launch: the emit kernel's
    capacity guard keeps its list out of the next image's (the lists are max_keypoints apart), and the keep-strongest and
    bucket kernels leave it alone.  The two pairs that use it fail with SVO_FAIL_CAPACITY (6) and report the count FOUND;
    the pairs on either side are what a fresh context gives for them.

    The pose: finalize_chain_kernel multiplies T_rel_inv into the running pose for pairs that are ok and passes the pose
    on unchanged for the others, so pairs 1 and 2 repeat pair 0's pose bit for bit and pair 3's is pair 0's times its own
    T_rel_inv -- to 1e-12: four products of entries below ~10 in float64, whatever the contraction of multiply and add."""
    seq, frames = small_seq
    h, w = frames[0][0].shape
    P1, P2 = seq.proj()
    dense = rand_image(h, w, 3, blocks=False)
    n_clean = [len(oracle.fast(f[0], 20, True)) for f in frames]
    n_dense = len(oracle.fast(dense, 20, True))
    cap = (max(n_clean) + n_dense) // 2
    assert 64 <= max(n_clean) < cap < n_dense                       # a condition on the inputs
    kw = dict(P1=P1, P2=P2, max_keypoints=cap, max_batch=4)
    keep, grid = 500, (32, 32, 2)
    if select == "keep_strongest":
        assert keep < min(n_clean)
        kw["fast_keep_strongest"] = keep

    def context():
        c = pkg.Context(w, h, device=0, **kw)
        if select == "buckets":
            c.set_fast_buckets(*grid)
        return c

    def batch(c, fs):
        L = tc.from_numpy(np.stack([f[0] for f in fs])).cuda()
        R = tc.from_numpy(np.stack([f[1] for f in fs])).cuda()
        return c.track_batch(L, R)

    c = context()
    res = batch(c, [frames[0], frames[1], (dense, dense), frames[2], frames[3]])
    tracks = [c.batch_tracks(p) for p in (0, 3)]
    c.close()
    c = context()
    head = batch(c, [frames[0], frames[1]])
    head_tracks = c.batch_tracks(0)
    c.close()
    c = context()
    tail = batch(c, [frames[2], frames[3]])
    tail_tracks = c.batch_tracks(0)
    c.close()

    # what a clean frame reports: every corner, the `keep` strongest, or what its cells keep (the fresh contexts' counts;
    # test_gpu_keep_strongest.py and test_gpu_buckets.py hold those to the oracle)
    if select == "all":
        assert (int(head[0]["n_prev_kps"]), int(head[0]["n_cur_kps"])) == (n_clean[0], n_clean[1])
        assert (int(tail[0]["n_prev_kps"]), int(tail[0]["n_cur_kps"])) == (n_clean[2], n_clean[3])
    elif select == "keep_strongest":
        assert [int(r[k]) for r in (head[0], tail[0]) for k in ("n_prev_kps", "n_cur_kps")] == [keep] * 4
    else:
        assert all(30 <= int(r[k]) < min(n_clean) for r in (head[0], tail[0]) for k in ("n_prev_kps", "n_cur_kps"))
    assert int(head[0]["ok"]) == 1 and int(tail[0]["ok"]) == 1      # the clean pairs track: their records are not trivial

    for p in (1, 2):
        assert int(res[p]["fail_stage"]) == 6 and int(res[p]["ok"]) == 0, p
    # the overflowing side reports the count found, untouched by the selection; the other side its own
    assert (int(res[1]["n_prev_kps"]), int(res[1]["n_cur_kps"])) == (int(head[0]["n_cur_kps"]), n_dense)
    assert (int(res[2]["n_prev_kps"]), int(res[2]["n_cur_kps"])) == (n_dense, int(tail[0]["n_prev_kps"]))
    assert res[0].tobytes() == head[0].tobytes()
    for got, want in zip(tracks[0], head_tracks):
        assert got.tobytes() == want.tobytes()
    for name in pkg.STEP_DTYPE.names:
        if name != "pose":
            assert res[3][name].tobytes() == tail[0][name].tobytes(), name
    for got, want in zip(tracks[1], tail_tracks):
        assert got.tobytes() == want.tobytes()
    pose0 = res[0]["pose"].reshape(4, 4)
    assert np.abs(pose0 - _chain_step(np.eye(4), res[0])).max() < 1e-12
    assert res[1]["pose"].tobytes() == res[0]["pose"].tobytes() and res[2]["pose"].tobytes() == res[0]["pose"].tobytes()
    assert np.abs(res[3]["pose"].reshape(4, 4) - _chain_step(pose0, res[3])).max() < 1e-12
    assert np.abs(tail[0]["pose"].reshape(4, 4) - _chain_step(np.eye(4), tail[0])).max() < 1e-12
