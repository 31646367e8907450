"""FAST corner buckets (-m gpu): svo_set_fast_buckets / svo_bucket_corners against tests/_bucket_ref.py.

LK mode tracks every cv::FAST corner (src/tracking.cpp:94-113); the additive option keeps the per_cell strongest corners of
every cell of a pixel grid ON THE DEVICE (ties: raster order first, survivors in raster order), so an LK user trades corners
for throughput without losing coverage of the image.  (a) the stage entry on lists no rendered image produces, byte for
byte; (b)-(f) the fused entry points against the CPU oracle fed the reference's kept list; (g) the host runner; (h) KITTI
size."""
import os
import subprocess

import numpy as np
import pytest

from _bucket_ref import bucket, bucket_cells
from test_gpu_ingest import _render
from test_gpu_keep_strongest import _strongest
from test_gpu_parity_fullsize import TIGHT, _K, relfro
from test_host_api import _write_pgm, _write_yaml, host_built   # noqa: F401  (host_built: the fixture that builds host/)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tc():
    import torch
    assert torch.cuda.is_available()
    return torch


# ---- a. the stage kernel on adversarial lists -----------------------------------------------------------------------------
def _list(pixels, resp, width):
    """the raster-ordered cv::FAST records of distinct pixel indices y * width + x"""
    order = np.argsort(pixels, kind="stable")
    pixels, resp = np.asarray(pixels)[order], np.asarray(resp)[order]
    kp = np.zeros(len(pixels), dtype=[("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"),
                                      ("octave", "<i4"), ("class_id", "<i4")])
    kp["x"], kp["y"], kp["response"] = pixels % width, pixels // width, resp
    kp["size"], kp["angle"], kp["class_id"] = 7.0, -1.0, -1
    return kp


def _random_list(seed, w, h, n, lo=1, hi=255, x0=0, y0=0, rw=None, rh=None):
    """n distinct pixels of the rw x rh window at (x0, y0) of a w x h image, responses uniform in lo..hi"""
    rng = np.random.default_rng(seed)
    rw, rh = rw or w, rh or h
    p = rng.choice(rw * rh, size=n, replace=False)
    return _list((y0 + p // rw) * w + x0 + p % rw, rng.integers(lo, hi + 1, n), w)


# name: (list, width, height, cell_w, cell_h, per_cell)
STAGE_CASES = {
    "empty": lambda: (_random_list(1, 64, 48, 0), 64, 48, 16, 16, 2),
    "one": lambda: (_random_list(2, 64, 48, 1), 64, 48, 16, 16, 1),
    "fewer_than_per_cell": lambda: (_random_list(3, 64, 48, 5), 64, 48, 16, 16, 8),
    "exact_cells": lambda: (_random_list(4, 64, 48, 1500), 64, 48, 16, 16, 3),
    "partial_edge_cells": lambda: (_random_list(5, 64, 48, 1500), 64, 48, 40, 24, 3),
    "pixel_cells_16384": lambda: (_random_list(6, 128, 128, 9000), 128, 128, 1, 1, 1),           # nothing is dropped
    "uniform_responses": lambda: (_random_list(7, 200, 120, 5000), 200, 120, 23, 17, 4),
    "few_distinct_responses": lambda: (_random_list(8, 200, 120, 5000, 20, 23), 200, 120, 23, 17, 4),
    "all_equal": lambda: (_random_list(9, 64, 48, 2000, 77, 77), 64, 48, 16, 16, 5),               # pure raster tie-breaking
    "one_cell_3001": lambda: (_random_list(10, 512, 512, 3001, 1, 255, 128, 192, 64, 64), 512, 512, 64, 64, 7),
    "one_cell_3001_ties": lambda: (_random_list(11, 512, 512, 3001, 9, 10, 128, 192, 64, 64), 512, 512, 64, 64, 7),
    "whole_image_65536": lambda: (_random_list(12, 512, 512, 65536), 512, 512, 512, 512, 2000),
    "per_cell_above_every_population": lambda: (_random_list(13, 64, 48, 1500), 64, 48, 16, 16, 100000),
    # the per-cell words move from LDS to device memory above 3072 cells: the last grid in LDS, the first beyond it, a large one
    "cells_3072": lambda: (_random_list(14, 128, 96, 9000, 1, 6), 128, 96, 2, 2, 1),
    "cells_3120": lambda: (_random_list(15, 130, 96, 9000, 1, 6), 130, 96, 2, 2, 1),
    "cells_8192_two_per_cell": lambda: (_random_list(16, 256, 128, 26000, 1, 3), 256, 128, 2, 2, 2),
}


@pytest.fixture(scope="module")
def stage_ctx(pkg):
    c = pkg.Context(64, 64, device=0)              # the stage entry is independent of the context's frame size
    yield c
    c.close()


@pytest.mark.parametrize("name", list(STAGE_CASES))
def test_stage_equals_reference_host_lists(stage_ctx, name):
    kps, w, h, cw, ch, k = STAGE_CASES[name]()
    want = bucket(kps, w, h, cw, ch, k)
    got = stage_ctx.bucket_corners(kps, w, h, cw, ch, k)
    assert len(got) == len(want) and got.tobytes() == want.tobytes()
    if name in ("pixel_cells_16384", "per_cell_above_every_population", "fewer_than_per_cell"):
        assert len(want) == len(kps)
    elif len(kps) > 1:
        assert len(want) < len(kps)
    if name == "whole_image_65536":
        assert len(want) == 2000 and want.tobytes() == _strongest(kps, 2000).tobytes()
    if name.startswith("one_cell_3001"):
        assert len(want) == 7 and len(np.unique(bucket_cells(kps, w, cw, ch))) == 1


@pytest.mark.parametrize("name", ["one_cell_3001", "whole_image_65536", "cells_8192_two_per_cell"])
def test_stage_equals_reference_device_lists(pkg, stage_ctx, tc, name):
    kps, w, h, cw, ch, k = STAGE_CASES[name]()
    want = bucket(kps, w, h, cw, ch, k)
    d = tc.from_numpy(np.frombuffer(kps.tobytes(), np.uint8).copy()).cuda()
    out, m = stage_ctx.bucket_corners(d, w, h, cw, ch, k)
    tc.cuda.synchronize()
    m = int(m.cpu()[0])
    got = np.frombuffer(out.cpu().numpy().tobytes(), dtype=pkg.KP_DTYPE)[:m]
    assert m == len(want) and got.tobytes() == want.tobytes()


def test_stage_argument_errors(pkg, stage_ctx):
    kps = _random_list(20, 129, 128, 300)
    with pytest.raises(pkg.SvoError):
        stage_ctx.bucket_corners(kps, 129, 128, 1, 1, 1)              # 16 512 cells
    assert len(stage_ctx.bucket_corners(kps, 129, 128, 129, 1, 1)) == len(np.unique(kps["y"]))
    with pytest.raises(pkg.SvoError):
        stage_ctx.bucket_corners(kps, 129, 128, 16, 16, 2, cap=len(kps) - 1)      # n > cap
    for bad in [(0, 16, 2), (16, 0, 2), (16, 16, 0)]:
        with pytest.raises(pkg.SvoError):
            stage_ctx.bucket_corners(kps, 129, 128, *bad)


# ---- b. the fused entry points against the CPU oracle --------------------------------------------------------------------
GRIDS = [(32, 32, 1), (32, 32, 2), (40, 24, 3), (16, 16, 1), (416, 128, 40)]
# what the CPU oracle keeps per frame for this seed, and the cells it cuts inside a run of equal responses
KEPT = {(32, 32, 1): (52, 52), (32, 32, 2): (103, 104), (40, 24, 3): (169, 184), (16, 16, 1): (191, 194), (416, 128, 40): (40, 40)}

TIE_CUTS = {(32, 32, 1): 6, (32, 32, 2): 15, (40, 24, 3): 14, (16, 16, 1): 14, (416, 128, 40): 2}     # over the three previous frames

_REF = {}


def _tie_cuts(kps, w, cw, ch, k):
    """cells that drop a corner whose response equals a kept one's"""
    cells, n = bucket_cells(kps, w, cw, ch), 0
    for c in np.unique(cells):
        r = np.sort(kps["response"][cells == c])[::-1]
        n += int(len(r) > k and r[k - 1] == r[k])
    return n


def _oracle_pairs(oracle, seq, frames, grid, keep=1 << 30):
    """Per pair: (step incl. tracks, kept corners of the previous frame, kept count of the current one, RANSAC record,
    T_rel_inv) -- the oracle's LK step on the reference's kept list, as test_gpu_keep_strongest._oracle_pairs."""
    key = (grid, keep)
    if key in _REF:
        return _REF[key]
    h, w = frames[0][0].shape
    P1, P2 = seq.proj()
    prm = oracle.make_params(P1, P2)
    sel_of = lambda img: _strongest(bucket(oracle.fast(img), w, h, *grid), keep)
    out, ties = [], 0
    for t in range(1, len(frames)):
        sel = sel_of(frames[t - 1][0])
        ties += _tie_cuts(oracle.fast(frames[t - 1][0]), w, *grid)
        res, _cur, _ = oracle.lk_track_step(prm, *frames[t - 1], *frames[t], sel, np.eye(4), want_tracks=True, threads=8)
        X = oracle.triangulate(P1, P2, res["tracks"][0], res["tracks"][1])
        pnp = oracle.pnp_ransac(X, res["tracks"][3], _K(P1))
        out.append((res, sel, len(sel_of(frames[t][0])), pnp))
    # not vacuous: every pair tracks, no frame falls under the 30-corner gate, and raster tie-breaking decides some cell
    assert all(r["ok"] for r, *_ in out)
    assert all(len(sel) >= 30 and n_cur >= 30 for _, sel, n_cur, _ in out)
    assert ties >= 1 and (keep < (1 << 30) or ties == TIE_CUTS[grid]), (grid, ties)
    _REF[key] = out
    return out


def _check(g, ref, tracks, pose):
    r, sel, n_cur, pnp = ref
    assert int(g["ok"]) == r["ok"] and int(g["fail_stage"]) == r["fail_stage"]
    assert int(g["n_prev_kps"]) == len(sel) and int(g["n_cur_kps"]) == n_cur                # the KEPT counts
    assert int(g["n_tracked"]) == r["n_tracked"] and int(g["n_inliers"]) == r["n_inliers"]
    assert int(g["ransac_iters"]) == pnp["ransac_iters"] and int(g["lm_iters"]) == pnp["lm_iters"]
    for got, want in zip(tracks[:4], r["tracks"]):
        assert got.tobytes() == want.tobytes()
    assert tracks[4].tobytes() == pnp["mask"].tobytes()
    assert relfro(g["pose"].reshape(4, 4), pose) <= TIGHT * 10


def _chain(ref, first, last):
    pose = np.eye(4)
    for r, *_ in ref[first:last + 1]:
        if r["ok"]:
            pose = pose @ r["T_rel_inv"]
    return pose


def _stacks(tc, frames):
    return (tc.stack([tc.from_numpy(f[0]) for f in frames]).cuda(), tc.stack([tc.from_numpy(f[1]) for f in frames]).cuda())


@pytest.mark.parametrize("grid", GRIDS)
def test_fused_parity_small_seq(pkg, oracle, tc, small_seq, grid):
    seq, frames = small_seq
    h, w = frames[0][0].shape
    P1, P2 = seq.proj()
    ref = _oracle_pairs(oracle, seq, frames, grid)
    n_pairs = len(ref)
    for _, sel, n_cur, _ in ref:
        assert KEPT[grid][0] <= len(sel) <= KEPT[grid][1], (grid, len(sel))
    kept = [bucket(oracle.fast(f[0]), w, h, *grid) for f in frames]
    # svo_track_batch
    c = pkg.Context(w, h, device=0, P1=P1, P2=P2, max_batch=n_pairs)
    c.set_fast_buckets(*grid)
    assert c.fast_buckets() == grid
    res = c.track_batch(*_stacks(tc, frames))
    for p in range(n_pairs):
        _check(res[p], ref[p], c.batch_tracks(p), _chain(ref, 0, p))
    c.close()
    # svo_add_frame on a fresh context
    c = pkg.Context(w, h, device=0, P1=P1, P2=P2)
    c.set_fast_buckets(*grid)
    for t, fr in enumerate(frames):
        rc, g = c.add_frame(*fr)
        assert c.frame_keypoints().tobytes() == kept[t].tobytes()      # the kept corners, raster order, responses intact
        if t:
            assert rc == 0
            _check(g, ref[t - 1], c.last_tracks(), _chain(ref, 0, t - 1))
        else:
            assert int(g["n_cur_kps"]) == len(kept[0])
    c.close()
    # svo_streams_step: stream 0 is the sequence, stream 1 the sequence shifted by one frame
    c = pkg.Context(w, h, device=0, P1=P1, P2=P2, max_batch=3)
    c.set_fast_buckets(*grid)
    c.streams_create(2)
    for s in range(len(frames) - 1):
        a, b = frames[s], frames[s + 1]
        recs = c.streams_step([0, 1], [a[0], b[0]], [a[1], b[1]])
        if s == 0:
            assert [int(r["n_cur_kps"]) for r in recs] == [len(kept[0]), len(kept[1])] and all(int(r["ok"]) == 1 for r in recs)
            continue
        _check(recs[0], ref[s - 1], c.streams_tracks(0), _chain(ref, 0, s - 1))
        _check(recs[1], ref[s], c.streams_tracks(1), _chain(ref, 1, s))
    c.close()


# ---- c. one cell covering the image is fast_keep_strongest ----------------------------------------------------------------
@pytest.mark.parametrize("k", [37, 150])
def test_one_cell_equals_keep_strongest(pkg, tc, small_seq, k):
    seq, frames = small_seq
    h, w = frames[0][0].shape
    P1, P2 = seq.proj()
    L, R = _stacks(tc, frames)
    a = pkg.Context(w, h, device=0, P1=P1, P2=P2, max_batch=len(frames) - 1)
    a.set_fast_buckets(w, h, k)
    b = pkg.Context(w, h, device=0, P1=P1, P2=P2, max_batch=len(frames) - 1, fast_keep_strongest=k)
    ra, rb = a.track_batch(L, R), b.track_batch(L, R)
    assert ra.tobytes() == rb.tobytes() and all(int(r["n_prev_kps"]) == k and int(r["ok"]) == 1 for r in ra)
    for p in range(len(frames) - 1):
        for x, y in zip(a.batch_tracks(p), b.batch_tracks(p)):
            assert x.tobytes() == y.tobytes() and len(x) > 0
    a.close()
    b.close()


# ---- d. buckets, then the global top-N on their survivors -----------------------------------------------------------------
def test_buckets_then_keep_strongest(pkg, oracle, tc, small_seq):
    seq, frames = small_seq
    h, w = frames[0][0].shape
    P1, P2 = seq.proj()
    ref = _oracle_pairs(oracle, seq, frames, (16, 16, 1), keep=100)
    assert all(len(sel) == 100 for _, sel, _, _ in ref)                 # 191-194 bucket survivors: the top-N cuts again
    c = pkg.Context(w, h, device=0, P1=P1, P2=P2, max_batch=len(ref), fast_keep_strongest=100)
    c.set_fast_buckets(16, 16, 1)
    res = c.track_batch(*_stacks(tc, frames))
    for p in range(len(ref)):
        _check(res[p], ref[p], c.batch_tracks(p), _chain(ref, 0, p))
    c.close()
    c = pkg.Context(w, h, device=0, P1=P1, P2=P2, fast_keep_strongest=100)
    c.set_fast_buckets(16, 16, 1)
    c.add_frame(*frames[0])
    assert c.frame_keypoints().tobytes() == ref[0][1].tobytes()
    c.close()


# ---- e. the setter's rules -----------------------------------------------------------------------------------------------
def test_setter_rules(pkg, oracle, tc, small_seq):
    seq, frames = small_seq
    h, w = frames[0][0].shape
    P1, P2 = seq.proj()
    raw = [oracle.fast(f[0]) for f in frames]
    kept = [bucket(k, w, h, 32, 32, 1) for k in raw]
    c = pkg.Context(w, h, device=0, P1=P1, P2=P2)
    assert c.fast_buckets() == (0, 0, 0)
    _, g = c.add_frame(*frames[0])
    assert int(g["n_cur_kps"]) == len(raw[0])
    c.set_fast_buckets(32, 32, 1)                                      # between two svo_add_frame calls
    _, g = c.add_frame(*frames[1])
    assert int(g["n_prev_kps"]) == len(raw[0]) and int(g["n_cur_kps"]) == len(kept[1])      # the stored frame keeps its corners
    assert c.frame_keypoints().tobytes() == kept[1].tobytes()
    _, g = c.add_frame(*frames[2])
    assert int(g["n_prev_kps"]) == len(kept[1]) and int(g["n_cur_kps"]) == len(kept[2])
    c.set_fast_buckets(7, -3, 0)                                       # off: the sizes are ignored
    assert c.fast_buckets() == (0, 0, 0)
    _, g = c.add_frame(*frames[3])
    assert int(g["n_prev_kps"]) == len(kept[2]) and int(g["n_cur_kps"]) == len(raw[3])
    c.close()
    # per_cell = 0 gives back the records of a context that never called the setter
    L, R = _stacks(tc, frames)
    a = pkg.Context(w, h, device=0, P1=P1, P2=P2, max_batch=len(frames) - 1)
    a.set_fast_buckets(32, 32, 1)
    cut = a.track_batch(L, R)
    a.set_fast_buckets(32, 32, 0)
    b = pkg.Context(w, h, device=0, P1=P1, P2=P2, max_batch=len(frames) - 1)
    ra, rb = a.track_batch(L, R), b.track_batch(L, R)
    assert ra.tobytes() == rb.tobytes() and cut.tobytes() != rb.tobytes()
    for bad in [(0, 32, 1), (32, 0, 1), (32, 32, -1), (1, 1, 1), (3, 1, 1)]:          # 416 x 128 / 3 x 1: 139 x 128 = 17 792 cells
        with pytest.raises(pkg.SvoError):
            b.set_fast_buckets(*bad)
    b.set_fast_buckets(4, 1, 1)                                        # 104 x 128 = 13 312 cells: per-cell words in device memory
    assert b.fast_buckets() == (4, 1, 1)
    got = b.track_batch(L, R)
    assert [int(r["n_prev_kps"]) for r in got] == [len(bucket(k, w, h, 4, 1, 1)) for k in raw[:-1]]
    a.close()
    b.close()
    o = pkg.Context(w, h, device=0, P1=P1, P2=P2, track_mode=pkg.MODE_ORB)
    with pytest.raises(pkg.SvoError):
        o.set_fast_buckets(32, 32, 1)                                  # ORB mode has its quadtree
    o.set_fast_buckets(32, 32, 0)
    o.close()


# ---- f. behind the ingest stage -------------------------------------------------------------------------------------------
def test_ingest_add_frame_with_buckets(pkg, synth, tc):
    seq, frames = _render(synth, tc, 832, 256, 4)
    P1, P2 = (pkg.scale_projection(P, 0.5, 0.5, "nearest").reshape(12) for P in seq.proj())
    a = pkg.Context(416, 128, device=0, P1=P1, P2=P2)
    a.ingest_create(832, 256, "nearest", 0.5, 0.5)
    b = pkg.Context(416, 128, device=0, P1=P1, P2=P2)
    plain = pkg.Context(416, 128, device=0, P1=P1, P2=P2)
    for c in (a, b):
        c.set_fast_buckets(32, 32, 2)
    for t, fr in enumerate(frames):
        small = tuple(b.resize(x, 416, 128, "nearest", 0.5, 0.5) for x in fr)
        rca, ga = a.ingest_add_frame(*fr)
        rcb, gb = b.add_frame(*small)
        _, gp = plain.add_frame(*small)
        assert rca == rcb == 0 and ga.tobytes() == gb.tobytes()
        assert 30 <= int(ga["n_cur_kps"]) < int(gp["n_cur_kps"]) and (t == 0 or int(ga["n_tracked"]) > 0)
        assert a.frame_keypoints().tobytes() == b.frame_keypoints().tobytes()
        for x, y in zip(a.last_tracks(), b.last_tracks()):
            assert x.tobytes() == y.tobytes()
    for c in (a, b, plain):
        c.close()


# ---- g. the host runner: the three YAML keys --------------------------------------------------------------------------------
def test_runner_bucket_keys(host_built, pkg, small_seq, tmp_path):
    seq, frames = small_seq
    h, w = frames[0][0].shape
    for cam in (0, 1):
        os.makedirs(tmp_path / f"image_{cam}")
        for t, fr in enumerate(frames):
            _write_pgm(tmp_path / f"image_{cam}" / f"{t:06d}.pgm", fr[cam])
    P1, P2 = seq.proj()
    ref = {}
    for on in (False, True):
        c = pkg.Context(w, h, device=0, P1=P1, P2=P2)
        if on:
            c.set_fast_buckets(32, 32, 2)
        ref[on] = []
        for fr in frames:
            c.add_frame(*fr)
            ref[on].append(c.get_pose()[:3])
        c.close()
    assert np.abs(np.array(ref[True]) - np.array(ref[False])).max() > 1e-9            # the option changes what is tracked
    keys = "fast_bucket_width: 32\nfast_bucket_height: 32\nfast_bucket_keep: 2\n"
    for name, extra in [("loop", ""), ("batch", "batch_size: 2\ndecode_threads: 2\n")]:
        y = tmp_path / f"{name}.yaml"
        _write_yaml(y, str(tmp_path), fx=seq.fx, fy=seq.fy, cx=seq.cx, cy=seq.cy)
        with open(y, "a", encoding="utf-8") as f:
            f.write(keys + extra)
        r = subprocess.run([os.path.join(host_built, "run_kitti_stereo"), str(y), str(tmp_path / f"{name}.txt")], capture_output=True)
        assert r.returncode == 0, r.stderr.decode()
        poses = np.loadtxt(tmp_path / f"{name}.txt").reshape(-1, 3, 4)
        assert poses.shape[0] == len(frames) and np.abs(poses - np.array(ref[True])).max() < 1e-6


# ---- h. KITTI size ----------------------------------------------------------------------------------------------------------
def test_kitti_size_properties(pkg, synth, tc):
    seq, frames = _render(synth, tc, 1241, 376, 2, 20200710)
    P1, P2 = seq.proj()
    c = pkg.Context(1241, 376, device=0, P1=P1, P2=P2)
    raw = c.fast_detect(frames[1][0])
    c.set_fast_buckets(50, 50, 4)
    c.add_frame(*frames[0])
    rc, g = c.add_frame(*frames[1])
    kp = c.frame_keypoints()
    c.close()
    assert rc == 0 and int(g["ok"]) == 1 and int(g["n_cur_kps"]) == len(kp)
    key = kp["y"].astype(np.int64) * 1241 + kp["x"].astype(np.int64)
    assert np.all(np.diff(key) > 0)                                                       # raster order
    pop = np.bincount(bucket_cells(kp, 1241, 50, 50), minlength=25 * 8)
    assert len(pop) == 25 * 8 and pop.max() == 4 and len(kp) < len(raw)
    assert kp.tobytes() == bucket(raw, 1241, 376, 50, 50, 4).tobytes()
