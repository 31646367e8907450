"""Shi-Tomasi corners (-m gpu): svo_min_eigen_map / svo_gftt_detect / svo_set_lk_detector against tests/_gftt_ref.py.

(a) the eigenvalue map bit for bit; (b) the detector byte for byte -- records, strengths, count -- over the parameter space
and the sizes its sort and its grid change path at; (c) the fused entry points against the CPU oracle fed the reference's
list; (d) the < 30 gate on the reference's counts; (e) the setter's rules; (f) behind the ingest stage; (g) the host runner;
(h) KITTI size."""
import os
import subprocess

import numpy as np
import pytest

import _gftt_ref as G
import _natural
import conftest
from test_gpu_buckets import _chain, _check, _stacks
from test_gpu_ingest import _render
from test_gpu_parity_fullsize import _K
from test_host_api import _write_pgm, _write_yaml, host_built   # noqa: F401  (host_built: the fixture that builds host/)

pytestmark = pytest.mark.gpu

SIZES = [(8, 8), (33, 17), (67, 35), (161, 97), (416, 128)]           # (w, h): below a tile, odd, partial edge tiles
CONTENT = ["noise", "flat", "checker", "natural"]


@pytest.fixture(scope="module")
def tc():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(64, 64, device=0, max_keypoints=16384)            # the stage entries are independent of the context's frame size
    yield c
    c.close()


_IMG, _EIG = {}, {}


def _image(content, w, h):
    key = (content, w, h)
    if key not in _IMG:
        if content == "noise":
            img = conftest.rand_image(h, w, 3 * w + h, blocks=(w > 40))
        elif content == "flat":
            img = np.full((h, w), 93, np.uint8)
        elif content == "checker":                                    # 0 / 255 squares of 4: extreme gradients and mass ties
            yy, xx = np.mgrid[0:h, 0:w]
            img = ((((yy // 4) + (xx // 4)) & 1) * 255).astype(np.uint8)
        else:                                                         # a crop of the 1/f texture (natural-image statistics)
            tex = _natural.pink_noise(512, seed=5)
            img = np.clip(tex[40:40 + h, 60:60 + w] * 255.0 + 0.5, 0, 255).astype(np.uint8)
        _IMG[key] = np.ascontiguousarray(img)
    return _IMG[key]


def _eig(content, w, h):
    key = (content, w, h)
    if key not in _EIG:
        _EIG[key] = G.min_eigen_map(_image(content, w, h))
    return _EIG[key]


def _padded(img, extra=13):
    """the same image as a view of a wider buffer (pitch > width), the padding poisoned"""
    h, w = img.shape
    buf = np.full((h, w + extra), 0xA5, np.uint8)
    buf[:, :w] = img
    return buf[:, :w]


def _same_list(got, want, what=""):
    (gk, gs), (wk, ws) = got, want
    assert len(gk) == len(wk), (what, len(gk), len(wk))
    assert gk.tobytes() == wk.tobytes(), what
    assert gs.dtype == np.float32 and gs.tobytes() == ws.tobytes(), what


# ---- a. the eigenvalue map ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("content", CONTENT)
@pytest.mark.parametrize("w,h", SIZES)
def test_min_eigen_map_equals_reference(ctx, tc, w, h, content):
    img, want = _image(content, w, h), _eig(content, w, h)
    got = ctx.min_eigen_map(_padded(img))
    assert got.dtype == np.float32 and got.shape == (h, w) and got.tobytes() == want.tobytes()
    d = tc.from_numpy(_padded(img, 29).base.copy()).cuda()[:, :w]      # device input, pitch w + 29
    assert d.stride(0) == w + 29
    got_d = ctx.min_eigen_map(d)
    tc.cuda.synchronize()
    assert got_d.cpu().numpy().tobytes() == want.tobytes()
    if content == "flat":
        assert np.all(want == 0)
    else:
        assert want.max() > 0


# ---- b. the detector ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("content", CONTENT)
@pytest.mark.parametrize("w,h", SIZES)
def test_detect_equals_reference(pkg, ctx, tc, w, h, content):
    img, eig = _image(content, w, h), _eig(content, w, h)
    n_cand = len(G.candidates(eig, 0.01))
    if n_cand > 16384:
        pytest.fail("the case needs a larger cap")
    for maxc, q, md in [(0, 0.01, 0.0), (0, 0.01, 8.0), (500, 0.01, 20.0), (0, 1e-6, 2.5) if w * h < 20000 else (0, 0.05, 2.5)]:
        want = G.gftt(img, maxc, q, md, eig=eig)
        _same_list(ctx.gftt_detect(_padded(img), maxc, q, md), want, (maxc, q, md))
    # device input and outputs
    want = G.gftt(img, 0, 0.01, 8.0, eig=eig)
    d = tc.from_numpy(_padded(img, 29).base.copy()).cuda()[:, :w]
    out, strength, n = ctx.gftt_detect(d, 0, 0.01, 8.0)
    tc.cuda.synchronize()
    n = int(n.cpu()[0])
    got = np.frombuffer(out.cpu().numpy().tobytes(), dtype=pkg.KP_DTYPE)[:n]
    _same_list((got, strength.cpu().numpy()[:n]), want, "device")
    if content == "flat":
        assert n == 0
    elif (w, h) != (8, 8):
        assert n > 0


@pytest.fixture(scope="module")
def base_case():
    img = _image("noise", 161, 97)
    return img, _eig("noise", 161, 97)


@pytest.mark.parametrize("md", [0.0, 1.0, 1.5, 2.5, 8.0, 20.0, 200.0])
def test_detect_min_distance(ctx, base_case, md):
    img, eig = base_case
    want = G.gftt(img, 0, 0.01, md, eig=eig)
    _same_list(ctx.gftt_detect(img, 0, 0.01, md), want)
    assert len(want[0]) >= 1 and (md < 190 or len(want[0]) == 1)      # 200 > the image diagonal (188): one corner
    if md >= 1:
        x, y = want[0]["x"].astype(np.int64), want[0]["y"].astype(np.int64)
        d2 = (x[:, None] - x[None]) ** 2 + (y[:, None] - y[None]) ** 2 + np.eye(len(x), dtype=np.int64) * 10 ** 9
        assert d2.min() >= md * md


def test_detect_max_corners(ctx, base_case):
    img, eig = base_case
    full = G.gftt(img, 0, 0.01, 8.0, eig=eig)
    n = len(full[0])
    assert n > 3
    for maxc in (0, 1, n, n - 1, n + 1, -5):
        want = G.gftt(img, maxc, 0.01, 8.0, eig=eig)
        assert len(want[0]) == (n if maxc <= 0 else min(n, maxc))
        _same_list(ctx.gftt_detect(img, maxc, 0.01, 8.0), want, maxc)
    for maxc in (1, 7):                                               # and without spacing
        _same_list(ctx.gftt_detect(img, maxc, 0.01, 0.0), G.gftt(img, maxc, 0.01, 0.0, eig=eig), maxc)


@pytest.mark.parametrize("q", [1e-6, 0.01, 1.0])
def test_detect_quality_level(ctx, base_case, q):
    img, eig = base_case
    want = G.gftt(img, 0, q, 3.0, eig=eig)
    _same_list(ctx.gftt_detect(img, 0, q, 3.0), want)
    assert (len(want[0]) == 0) == (q == 1.0)                          # eig > thr is strict: nothing passes at 1.0


def _blobs(n, w=512, h=264):
    """n isolated bright blobs of different size and brightness on black: exactly n candidates at quality 0.2"""
    img = np.zeros((h, w), np.uint8)
    rng = np.random.default_rng(n)
    per_row = (w - 8) // 12
    assert n <= per_row * ((h - 8) // 12)
    for k in range(n):
        x, y = 6 + 12 * (k % per_row), 6 + 12 * (k // per_row)
        img[y:y + 3, x:x + 3] = 200 + int(rng.integers(0, 56))          # (a 3 x 3 blob has ONE peak; 2 x 2 would tie four ways)
    return img


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1024, 1025])
def test_detect_candidate_counts_around_the_sort_sizes(pkg, n):
    w, h = (512, 264) if n <= 65 else (640, 480)
    img = _blobs(n, w, h)
    eig = G.min_eigen_map(img)
    assert len(G.candidates(eig, 0.2)) == n
    c = pkg.Context(64, 64, device=0, max_keypoints=8192)
    try:
        for md in (0.0, 5.0, 13.0):
            want = G.gftt(img, 0, 0.2, md, eig=eig)
            _same_list(c.gftt_detect(img, 0, 0.2, md), want, md)
            assert md > 12 or len(want[0]) == n
    finally:
        c.close()


def test_detect_sort_in_device_memory(pkg):
    """more candidates than the LDS sort holds (4096 keys): every local maximum of a noise image"""
    big = conftest.rand_image(240, 400, 77, blocks=False)
    eig = G.min_eigen_map(big)
    assert 4096 < len(G.candidates(eig, 1e-6)) <= 8192
    c = pkg.Context(64, 64, device=0, max_keypoints=8192)
    try:
        for md in (0.0, 4.0):                                         # 4: 100 x 60 cells, in device memory too
            _same_list(c.gftt_detect(big, 0, 1e-6, md), G.gftt(big, 0, 1e-6, md, eig=eig), md)
    finally:
        c.close()


def test_detect_tie_order_on_the_checkerboard(ctx):
    img, eig = _image("checker", 161, 97), _eig("checker", 161, 97)
    idx = G.candidates(eig, 0.01)
    val = eig.reshape(-1)[idx]
    assert (np.diff(val) == 0).sum() >= 20                            # mass ties: the order is the raster rule's
    for md in (0.0, 3.0):
        _same_list(ctx.gftt_detect(img, 0, 0.01, md), G.gftt(img, 0, 0.01, md, eig=eig), md)


def test_detect_grids(pkg, ctx):
    # partial edge cells: 161 x 97 with cells of 20 (8.05 x 4.85 cells) is in test_detect_min_distance; a grid above what LDS
    # holds (1536 cells): cells of 2 at 161 x 97 = 81 x 49 = 3969 cells, and the last grid inside it, 96 x 32 / 2 = 768
    img, eig = _image("noise", 161, 97), _eig("noise", 161, 97)
    for md, cells in [(2.0, 3969), (1.0, 15617), (3.0, 54 * 33)]:
        cell = G.cv_round(md)
        assert ((161 + cell - 1) // cell) * ((97 + cell - 1) // cell) == cells and cells > 1536
        _same_list(ctx.gftt_detect(img, 0, 1e-6, md), G.gftt(img, 0, 1e-6, md, eig=eig), md)
    small = _image("noise", 67, 35)
    _same_list(ctx.gftt_detect(small, 0, 1e-6, 2.0), G.gftt(small, 0, 1e-6, 2.0), "34 x 18 cells")
    with pytest.raises(pkg.SvoError):
        ctx.gftt_detect(_image("noise", 416, 128), 0, 0.01, 1.0)      # 53 248 cells


def test_detect_argument_errors(pkg, ctx, base_case):
    img, eig = base_case
    n_cand = len(G.candidates(eig, 0.01))
    kept = len(G.gftt(img, 5, 0.01, 8.0, eig=eig)[0])
    assert kept == 5 < n_cand
    with pytest.raises(pkg.SvoError):
        ctx.gftt_detect(img, 5, 0.01, 8.0, cap=n_cand - 1)            # CANDIDATES above cap, whatever would be kept
    _same_list(ctx.gftt_detect(img, 5, 0.01, 8.0, cap=n_cand), G.gftt(img, 5, 0.01, 8.0, eig=eig))
    for q, md in [(0.0, 8.0), (-1.0, 8.0), (float("inf"), 8.0), (float("nan"), 8.0), (0.01, -1.0), (0.01, float("inf")),
                  (0.01, float("nan"))]:
        with pytest.raises(pkg.SvoError):
            ctx.gftt_detect(img, 5, q, md)


# ---- c. the fused entry points against the CPU oracle ---------------------------------------------------------------------
GF = (100, 0.01, 8.0)
_SEQ = {}


def _seq(synth, w, h, n):
    if (w, h, n) not in _SEQ:
        seq = synth.StereoSequence(width=w, height=h, n_frames=n, seed=11)
        _SEQ[(w, h, n)] = (seq, [tuple(x.numpy() for x in seq.render(t)) for t in range(n)])
    return _SEQ[(w, h, n)]


@pytest.fixture(scope="module")
def fused_ref(oracle, synth):
    """Per pair of the 5-frame 416 x 128 sequence: (oracle step on the reference's list, that list, the reference's count of
    the current frame, RANSAC record) -- the layout test_gpu_buckets._check reads."""
    seq, frames = _seq(synth, 416, 128, 5)
    P1, P2 = seq.proj()
    prm = oracle.make_params(P1, P2)
    kept = [G.gftt(f[0], *GF)[0] for f in frames]
    assert all(len(k) == 100 for k in kept) and all(1500 < G.n_candidates(f[0]) < 4096 for f in frames)
    out = []
    for t in range(1, len(frames)):
        res, _cur, _ = oracle.lk_track_step(prm, *frames[t - 1], *frames[t], kept[t - 1], np.eye(4), want_tracks=True, threads=8)
        X = oracle.triangulate(P1, P2, res["tracks"][0], res["tracks"][1])
        pnp = oracle.pnp_ransac(X, res["tracks"][3], _K(P1))
        out.append((res, kept[t - 1], len(kept[t]), pnp))
    assert all(r["ok"] for r, *_ in out)                               # (the oracle's own FAST count passes its gate here)
    return seq, frames, kept, out


def test_fused_parity(pkg, tc, fused_ref):
    seq, frames, kept, ref = fused_ref
    h, w = frames[0][0].shape
    P1, P2 = seq.proj()
    n_pairs = len(ref)
    # svo_track_batch
    c = pkg.Context(w, h, device=0, P1=P1, P2=P2, max_batch=n_pairs)
    c.set_lk_detector("gftt", *GF)
    assert c.lk_detector() == ("gftt",) + GF
    res = c.track_batch(*_stacks(tc, frames))
    for p in range(n_pairs):
        _check(res[p], ref[p], c.batch_tracks(p), _chain(ref, 0, p))
    c.close()
    # svo_add_frame on a fresh context
    c = pkg.Context(w, h, device=0, P1=P1, P2=P2)
    c.set_lk_detector("gftt", *GF)
    for t, fr in enumerate(frames):
        rc, g = c.add_frame(*fr)
        assert c.frame_keypoints().tobytes() == kept[t].tobytes()      # the reference's list, selection order
        if t:
            assert rc == 0
            _check(g, ref[t - 1], c.last_tracks(), _chain(ref, 0, t - 1))
        else:
            assert int(g["n_cur_kps"]) == len(kept[0])
    c.close()
    # svo_streams_step: stream 0 is the sequence, stream 1 the sequence shifted by one frame
    c = pkg.Context(w, h, device=0, P1=P1, P2=P2, max_batch=3)
    c.set_lk_detector("gftt", *GF)
    c.streams_create(2)
    for s in range(len(frames) - 1):
        a, b = frames[s], frames[s + 1]
        recs = c.streams_step([0, 1], [a[0], b[0]], [a[1], b[1]])
        if s == 0:
            assert [int(r["n_cur_kps"]) for r in recs] == [100, 100] and all(int(r["ok"]) == 1 for r in recs)
            continue
        _check(recs[0], ref[s - 1], c.streams_tracks(0), _chain(ref, 0, s - 1))
        _check(recs[1], ref[s], c.streams_tracks(1), _chain(ref, 1, s))
    c.close()


def test_fused_parity_uploaded_async_carry_frame(pkg, fused_ref):
    seq, frames, kept, ref = fused_ref
    h, w = frames[0][0].shape
    P1, P2 = seq.proj()
    c = pkg.Context(w, h, device=0, P1=P1, P2=P2, max_batch=3)
    c.set_lk_detector("gftt", *GF)
    host = [c.host_frames(3) for _ in range(2)]
    got = []
    for k, (t0, n, slot) in enumerate([(0, 3, 0), (3, 2, 1)]):        # frames 0-2, then 3-4 behind the carried frame 2
        for e in (0, 1):
            host[e][:n, :, :w] = np.stack([frames[t][e] for t in range(t0, t0 + n)])
        c.upload_frames(k & 1, host[0][:n], host[1][:n], first_slot=slot)
        c.wait_upload(k & 1)
        c.track_uploaded_async(k & 1, slot + n, continue_chain=k > 0, carry_frame=k > 0)
        n_pairs = slot + n - 1
        recs = c.collect_results(n_pairs)
        for p in range(n_pairs):
            _check(recs[p], ref[len(got) + p], c.batch_tracks(p), _chain(ref, 0, len(got) + p))
        got.extend(recs)
    assert len(got) == 4
    c.close()


# ---- d. the < 30 gate on the reference's counts ---------------------------------------------------------------------------
def test_gate_follows_the_kept_count(pkg, oracle, synth):
    seq, frames = _seq(synth, 160, 96, 6)
    P1, P2 = seq.proj()
    prm = oracle.make_params(P1, P2)
    kept = [G.gftt(f[0], 500, 0.01, 20.0)[0] for f in frames]          # the reference's own literals
    n = [len(k) for k in kept]
    fails = [n[t] < 30 for t in range(1, len(frames))]
    assert any(fails) and not all(fails), n                             # the sequence crosses the gate, both ways
    c = pkg.Context(160, 96, device=0, P1=P1, P2=P2)
    c.set_lk_detector("gftt", 500, 0.01, 20.0)
    pose = np.eye(4)
    for t, fr in enumerate(frames):
        rc, g = c.add_frame(*fr)
        assert int(g["n_cur_kps"]) == n[t] and c.frame_keypoints().tobytes() == kept[t].tobytes()
        if t == 0:
            continue
        assert int(g["n_prev_kps"]) == n[t - 1]
        if fails[t - 1]:
            assert rc == 1 and int(g["ok"]) == 0 and int(g["fail_stage"]) == 1 and int(g["n_tracked"]) == 0      # SVO_FAIL_FEW_KEYPOINTS
        else:
            res, _cur, _ = oracle.lk_track_step(prm, *frames[t - 1], *fr, kept[t - 1], np.eye(4), want_tracks=True, threads=8)
            X = oracle.triangulate(P1, P2, res["tracks"][0], res["tracks"][1])
            pnp = oracle.pnp_ransac(X, res["tracks"][3], _K(P1))
            if res["ok"]:
                pose = pose @ res["T_rel_inv"]
            assert rc == (0 if res["ok"] else res["fail_stage"])
            _check(g, (res, kept[t - 1], n[t], pnp), c.last_tracks(), pose)
        assert np.allclose(c.get_pose(), pose, rtol=0, atol=1e-9)       # the chain skips the failed steps
    c.close()


# ---- e. the setter's rules ------------------------------------------------------------------------------------------------
def test_setter_rules(pkg, oracle, fused_ref):
    seq, frames, kept, ref = fused_ref
    h, w = frames[0][0].shape
    P1, P2 = seq.proj()
    raw = [oracle.fast(f[0]) for f in frames]
    c = pkg.Context(w, h, device=0, P1=P1, P2=P2)
    assert c.lk_detector() == ("fast", 0, 0.0, 0.0)
    _, g = c.add_frame(*frames[0])
    assert int(g["n_cur_kps"]) == len(raw[0])
    c.set_lk_detector("gftt", *GF)                                      # between two svo_add_frame calls
    assert c.lk_detector() == ("gftt",) + GF
    _, g = c.add_frame(*frames[1])
    assert int(g["n_prev_kps"]) == len(raw[0]) and int(g["n_cur_kps"]) == 100      # the stored frame keeps its corners
    assert c.frame_keypoints().tobytes() == kept[1].tobytes()
    c.set_lk_detector("fast", -7, float("nan"), -1.0)                   # back: the other arguments are ignored
    assert c.lk_detector() == ("fast", 0, 0.0, 0.0)
    _, g = c.add_frame(*frames[2])
    assert int(g["n_prev_kps"]) == 100 and int(g["n_cur_kps"]) == len(raw[2])
    assert c.frame_keypoints().tobytes() == raw[2].tobytes()            # the plain cv::FAST records again
    # mutual exclusion with the buckets, in both orders; the refused setter changes nothing
    c.set_fast_buckets(32, 32, 2)
    with pytest.raises(pkg.SvoError):
        c.set_lk_detector("gftt", *GF)
    assert c.lk_detector()[0] == "fast" and c.fast_buckets() == (32, 32, 2)
    c.set_fast_buckets(32, 32, 0)
    c.set_lk_detector("gftt", 50, 0.02, 4.0)
    with pytest.raises(pkg.SvoError):
        c.set_fast_buckets(32, 32, 2)
    assert c.lk_detector() == ("gftt", 50, 0.02, 4.0) and c.fast_buckets() == (0, 0, 0)
    c.set_fast_buckets(32, 32, 0)                                       # "off" is always allowed
    for bad in [(100, 0.0, 8.0), (100, -0.01, 8.0), (100, float("inf"), 8.0), (100, float("nan"), 8.0), (100, 0.01, -1.0),
                (100, 0.01, float("inf")), (100, 0.01, float("nan")), (100, 0.01, 1.0), (100, 0.01, 1.4)]:      # cells of 1: 53 248
        with pytest.raises(pkg.SvoError):
            c.set_lk_detector("gftt", *bad)
        assert c.lk_detector() == ("gftt", 50, 0.02, 4.0)
    with pytest.raises(pkg.SvoError):
        c.set_lk_detector(2, *GF)                                       # an unknown detector
    c.set_lk_detector("gftt", 100, 0.01, 2.0)                           # 208 x 64 = 13 312 cells: the grid lives in device memory
    _, g = c.add_frame(*frames[3])
    assert c.frame_keypoints().tobytes() == G.gftt(frames[3][0], 100, 0.01, 2.0)[0].tobytes()
    c.close()
    k = pkg.Context(w, h, device=0, P1=P1, P2=P2, fast_keep_strongest=100)
    with pytest.raises(pkg.SvoError):
        k.set_lk_detector("gftt", *GF)
    k.set_lk_detector("fast")
    k.close()
    o = pkg.Context(w, h, device=0, P1=P1, P2=P2, track_mode=pkg.MODE_ORB)
    with pytest.raises(pkg.SvoError):
        o.set_lk_detector("gftt", *GF)
    o.close()


def test_more_candidates_than_max_keypoints_is_a_capacity_failure(pkg, fused_ref):
    seq, frames, kept, ref = fused_ref
    h, w = frames[0][0].shape
    P1, P2 = seq.proj()
    c = pkg.Context(w, h, device=0, P1=P1, P2=P2, max_keypoints=1024)   # ~1 950 candidates per frame
    c.set_lk_detector("gftt", *GF)
    c.add_frame(*frames[0])
    rc, g = c.add_frame(*frames[1])
    assert rc == 6 and int(g["fail_stage"]) == 6 and int(g["n_cur_kps"]) == G.n_candidates(frames[1][0])       # SVO_FAIL_CAPACITY
    c.close()


# ---- f. behind the ingest stage -------------------------------------------------------------------------------------------
def test_ingest_add_frame_with_gftt(pkg, synth, tc):
    seq, frames = _render(synth, tc, 832, 256, 4)
    P1, P2 = (pkg.scale_projection(P, 0.5, 0.5, "nearest").reshape(12) for P in seq.proj())
    a = pkg.Context(416, 128, device=0, P1=P1, P2=P2)
    a.ingest_create(832, 256, "nearest", 0.5, 0.5)
    b = pkg.Context(416, 128, device=0, P1=P1, P2=P2)
    for c in (a, b):
        c.set_lk_detector("gftt", *GF)
    for t, fr in enumerate(frames):
        small = tuple(b.resize(x, 416, 128, "nearest", 0.5, 0.5) for x in fr)
        rca, ga = a.ingest_add_frame(*fr)
        rcb, gb = b.add_frame(*small)
        assert rca == rcb == 0 and ga.tobytes() == gb.tobytes()
        assert int(ga["n_cur_kps"]) == 100 and (t == 0 or int(ga["n_tracked"]) > 0)
        assert a.frame_keypoints().tobytes() == b.frame_keypoints().tobytes() == G.gftt(small[0], *GF)[0].tobytes()
        for x, y in zip(a.last_tracks(), b.last_tracks()):
            assert x.tobytes() == y.tobytes()
    for c in (a, b):
        c.close()


# ---- g. the host runner: the YAML keys --------------------------------------------------------------------------------------
def test_runner_gftt_keys(host_built, pkg, fused_ref, tmp_path):
    seq, frames, kept, ref = fused_ref
    h, w = frames[0][0].shape
    for cam in (0, 1):
        os.makedirs(tmp_path / f"image_{cam}")
        for t, fr in enumerate(frames):
            _write_pgm(tmp_path / f"image_{cam}" / f"{t:06d}.pgm", fr[cam])
    want = [np.eye(4)[:3]] + [_chain(ref, 0, p)[:3] for p in range(len(ref))]
    keys = "lk_detector: gftt\nnum_features: 100\ngftt_quality_level: 0.01\ngftt_min_distance: 8\n"
    for name, extra in [("loop", ""), ("batch", "batch_size: 2\ndecode_threads: 2\n")]:
        y = tmp_path / f"{name}.yaml"
        _write_yaml(y, str(tmp_path), fx=seq.fx, fy=seq.fy, cx=seq.cx, cy=seq.cy)
        with open(y, "a", encoding="utf-8") as f:
            f.write(keys + extra)
        r = subprocess.run([os.path.join(host_built, "run_kitti_stereo"), str(y), str(tmp_path / f"{name}.txt")], capture_output=True)
        assert r.returncode == 0, r.stderr.decode()
        poses = np.loadtxt(tmp_path / f"{name}.txt").reshape(-1, 3, 4)
        assert poses.shape[0] == len(frames) and np.abs(poses - np.array(want)).max() < 1e-6


def test_runner_gftt_defaults(host_built, pkg, fused_ref, tmp_path):
    """`lk_detector: gftt` alone: the runner's defaults are the reference's literals (500, 0.01, 20)"""
    seq, frames, kept, ref = fused_ref
    h, w = frames[0][0].shape
    for cam in (0, 1):
        os.makedirs(tmp_path / f"image_{cam}")
        for t, fr in enumerate(frames):
            _write_pgm(tmp_path / f"image_{cam}" / f"{t:06d}.pgm", fr[cam])
    P1, P2 = seq.proj()
    c = pkg.Context(w, h, device=0, P1=P1, P2=P2)
    c.set_lk_detector("gftt", 500, 0.01, 20.0)
    want = []
    for t, fr in enumerate(frames):
        c.add_frame(*fr)
        assert c.frame_keypoints().tobytes() == G.gftt(fr[0], 500, 0.01, 20.0)[0].tobytes()
        want.append(c.get_pose()[:3])
    c.close()
    assert np.abs(np.array(want[-1]) - np.eye(4)[:3]).max() > 1e-3                      # it moved
    y = tmp_path / "d.yaml"
    _write_yaml(y, str(tmp_path), fx=seq.fx, fy=seq.fy, cx=seq.cx, cy=seq.cy)
    with open(y, "a", encoding="utf-8") as f:
        f.write("lk_detector: gftt\n")
    r = subprocess.run([os.path.join(host_built, "run_kitti_stereo"), str(y), str(tmp_path / "d.txt")], capture_output=True)
    assert r.returncode == 0, r.stderr.decode()
    poses = np.loadtxt(tmp_path / "d.txt").reshape(-1, 3, 4)
    assert poses.shape[0] == len(frames) and np.abs(poses - np.array(want)).max() < 1e-6


# ---- h. KITTI size ----------------------------------------------------------------------------------------------------------
def test_kitti_size_step(pkg, synth, tc):
    seq, frames = _render(synth, tc, 1241, 376, 3, 20200710)
    P1, P2 = seq.proj()
    L, R = _stacks(tc, frames)
    c = pkg.Context(1241, 376, device=0, P1=P1, P2=P2, max_batch=2, max_keypoints=16384)
    c.set_lk_detector("gftt", 500, 0.01, 20.0)
    res = c.track_batch(L, R)
    assert all(int(r["ok"]) == 1 and int(r["n_prev_kps"]) == 500 and int(r["n_cur_kps"]) == 500 for r in res)
    for t in (0, 1):
        kp, s = c.gftt_detect(frames[t][0], 500, 0.01, 20.0)
        want = G.gftt(frames[t][0], 500, 0.01, 20.0)
        _same_list((kp, s), want, t)
        assert len(kp) == 500 and np.all(np.diff(s) <= 0)
        x, y = kp["x"].astype(np.int64), kp["y"].astype(np.int64)
        d2 = (x[:, None] - x[None]) ** 2 + (y[:, None] - y[None]) ** 2 + np.eye(500, dtype=np.int64) * 10 ** 9
        assert d2.min() >= 400
        t1 = c.batch_tracks(t)[0]                                       # tracked corners are a subset of the kept list, in its order
        pos = {(float(a), float(b)): i for i, (a, b) in enumerate(zip(kp["x"], kp["y"]))}
        order = [pos[(float(a), float(b))] for a, b in t1]
        assert len(order) > 30 and order == sorted(order)
    c.close()
