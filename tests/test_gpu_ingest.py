"""cv::resize on the GPU (svo_resize) and the ingest stage (svo_ingest_*): full-size frames downscaled on the device before
tracking.

Yardsticks, none of which is the code under test:
  - tests/_resize_ref.py, the numpy restatement of the three cv::resize branches (itself held against the oracle's C
    restatement by tests/test_resize_ref.py): svo_resize equals it byte for byte;
  - a SECOND context without an ingest stage, fed _resize_ref frames and scale_projection matrices: every record and track
    read-back of an svo_ingest_X call equals, as bytes, what svo_X gives there (the contract of include/svo_abi.h);
  - the CPU oracle on _resize_ref frames, with the comparison of the existing parity tests.
Every contract case also asserts ok == 1 on every tracked step: two empty records compare equal and prove nothing."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import conftest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _resize_ref as RR   # noqa: E402
from test_gpu_parity_pose import TIGHT, _check_step, relfro   # noqa: E402

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = -1, -4
ORB_KW = dict(min_move2=0.05 ** 2, max_move2=100.0)


@pytest.fixture(scope="module")
def tc():
    import torch
    assert torch.cuda.is_available()
    return torch


def _same(g, a, what=""):
    for name in g.dtype.names:
        assert np.asarray(g[name]).tobytes() == np.asarray(a[name]).tobytes(), f"{what}: field {name} differs: {g[name]} != {a[name]}"
    assert g.tobytes() == a.tobytes(), what


def _same_tracks(ta, tb, what=""):
    assert len(ta) == len(tb) == 5
    for x, y in zip(ta, tb):
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), what


_RENDERED = {}


def _render(synth, tc, w, h, n, seed=11):
    """n frames (left, right) as numpy, rendered once per (size, n, seed) on the GPU."""
    key = (w, h, n, seed)
    if key not in _RENDERED:
        seq = synth.StereoSequence(width=w, height=h, n_frames=n, seed=seed, device=tc.device("cuda", 0))
        _RENDERED[key] = (seq, [tuple(x.cpu().numpy() for x in seq.render(t)) for t in range(n)])
    return _RENDERED[key]


# ---- e. svo_resize == _resize_ref ------------------------------------------------------------------------------------
#        (sw, sh, dw, dh, f): f > 0 factor form, f = 0 size form
RESIZE_CASES = [(1920, 1080, 960, 540, 0.5), (1280, 720, 768, 432, 0.6), (2208, 1242, 1104, 621, 0.5),
                (1241, 376, 620, 188, 0.5),      # odd width: the box branch with a spare source column
                (1241, 376, 620, 188, 0.0),      # the same sizes in size form: scale 2.0016, bilinear
                (832, 256, 499, 154, 0.0), (416, 128, 416, 128, 0.0)]


def _padded(tc, stack, pad, fill, device):
    """(n, h, w) numpy -> a view with rows `pad` bytes longer, numpy (host) or torch cuda; the padding holds `fill`."""
    n, h, w = stack.shape
    big = np.full((n, h, w + pad), fill, np.uint8)
    big[:, :, :w] = stack
    if device:
        t = tc.from_numpy(big).cuda()
        return t, t[:, :, :w]
    return big, big[:, :, :w]


@pytest.mark.parametrize("interp", ["nearest", "linear"])
@pytest.mark.parametrize("sw,sh,dw,dh,f", RESIZE_CASES)
def test_resize_equals_reference(pkg, synth, tc, sw, sh, dw, dh, f, interp):
    if f:
        assert RR.out_size(sw, sh, f, f) == (dw, dh)
    box = interp == "linear" and RR.is_box(sw, sh, dw, dh, f, f)
    assert box == (interp == "linear" and f == 0.5)
    _, fr = _render(synth, tc, sw, sh, 1)
    imgs = np.stack([conftest.rand_image(sh, sw, 1, blocks=False), conftest.rand_image(sh, sw, 2, blocks=True),
                     fr[0][0], fr[0][1], conftest.rand_image(sh, sw, 3, blocks=False)])
    ref = np.stack([RR.resize(im, dw, dh, interp, f, f) for im in imgs])
    c = pkg.Context(416, 128, device=0)                 # any context: the sizes of a resize are its own
    combos = 0
    for n in (1, 5):
        src_n, ref_n = (imgs[2:3], ref[2:3]) if n == 1 else (imgs, ref)
        for device in (False, True):
            for pad_s, pad_d in ((0, 0), (13, 7), (64, 16)):
                _, src = _padded(tc, src_n, pad_s, 0x5A, device)
                dst_full, dst = _padded(tc, np.zeros((n, dh, dw), np.uint8), pad_d, 0xA5, device)
                if pad_s == 0:
                    src = tc.from_numpy(src_n.copy()).cuda() if device else src_n.copy()
                got = c.resize(src, dw, dh, interp, f, f, out=dst)
                assert got is dst
                if device:
                    c.sync()
                    out_full = dst_full.cpu().numpy()
                else:
                    out_full = dst_full
                bad = int((out_full[:, :, :dw] != ref_n).sum())
                assert bad == 0, (n, device, pad_s, pad_d, bad)
                assert (out_full[:, :, dw:] == 0xA5).all(), "bytes beyond dw were written"
                combos += 1
    # a single 2-D image, result allocated by the binding
    assert np.array_equal(c.resize(imgs[1], dw, dh, interp, f, f), ref[1])
    assert np.array_equal(c.resize(tc.from_numpy(imgs[1]).cuda(), dw, dh, interp, f, f).cpu().numpy(), ref[1])
    assert combos == 12
    c.close()


def test_resize_steep_reduction_is_gathered_from_global_memory(pkg, tc):
    """8192 -> 40 columns: the source segment of a tile does not fit the LDS budget; the unstaged path gives the same bytes."""
    img = conftest.rand_image(600, 8192, 9, blocks=False)
    c = pkg.Context(416, 128, device=0)
    for interp in ("nearest", "linear"):
        assert np.array_equal(c.resize(img, 40, 30, interp), RR.resize(img, 40, 30, interp))
        assert np.array_equal(c.resize(tc.from_numpy(img).cuda(), 40, 30, interp).cpu().numpy(), RR.resize(img, 40, 30, interp))
    c.close()


# ---- f. argument errors ------------------------------------------------------------------------------------------------
def _plain_records(c, frames):
    return [c.add_frame(*f)[1] for f in frames]


def test_argument_errors_leave_the_context_alone(pkg, small_seq):
    seq, frames = small_seq                              # 416 x 128
    P1, P2 = seq.proj()
    fresh = pkg.Context(416, 128, device=0, P1=P1, P2=P2, max_batch=4)
    want = _plain_records(fresh, frames)
    fresh.close()
    assert all(int(r["ok"]) == 1 for r in want)
    c = pkg.Context(416, 128, device=0, P1=P1, P2=P2, max_batch=4)
    lib, h = c.lib, c.h
    big = np.zeros((256, 832), np.uint8)
    res = pkg.StepResult()
    ids = np.zeros(1, np.int32)
    p = ctypes.c_void_p(big.ctypes.data)
    # every svo_ingest_* call before svo_ingest_create: SVO_ERR_STATE
    assert lib.svo_ingest_info(h, None, None, None, None, None) == ERR_STATE
    assert lib.svo_ingest_add_frame(h, p, p, 832, 0, ctypes.byref(res)) == ERR_STATE
    assert lib.svo_ingest_track_batch(h, p, p, 832, 832 * 256, 2, None, None, 1) == ERR_STATE
    assert lib.svo_ingest_streams_step(h, ctypes.c_void_p(ids.ctypes.data), 1, p, p, 832, 0, 0, ctypes.byref(res), 0) == ERR_STATE
    assert lib.svo_ingest_upload_frames_at(h, 0, 0, p, p, 832, 832 * 256, 1) == ERR_STATE
    # refused creations: cvRound(sw * fx) != dw, upscale, the box branch with 2 dw > sw, sw > 8192, unknown interp, mixed forms
    for args in [(832, 256, 0, 0.6, 0.6), (835, 256, 0, 0.5, 0.5), (208, 64, 0, 0.0, 0.0), (208, 64, 1, 2.0, 2.0),
                 (831, 256, 1, 0.5, 0.5), (832, 255, 1, 0.5, 0.5), (8320, 256, 0, 0.0, 0.0), (832, 256, 2, 0.5, 0.5),
                 (832, 256, 0, 0.5, 0.0)]:
        assert lib.svo_ingest_create(h, args[0], args[1], args[2], args[3], args[4]) == ERR_ARG, args
        assert lib.svo_ingest_info(h, None, None, None, None, None) == ERR_STATE
    # ... and the same rules through svo_resize
    out = np.zeros((128, 416), np.uint8)
    po = ctypes.c_void_p(out.ctypes.data)
    assert lib.svo_resize(h, p, 832, 256, 832, 0, po, 416, 128, 416, 0, 1, 0, 0.6, 0.6, 0) == ERR_ARG
    assert lib.svo_resize(h, po, 416, 128, 416, 0, p, 832, 256, 832, 0, 1, 0, 0.0, 0.0, 0) == ERR_ARG       # upscale
    assert lib.svo_resize(h, p, 831, 256, 832, 0, po, 416, 128, 416, 0, 1, 1, 0.5, 0.5, 0) == ERR_ARG       # box, 2 dw > sw
    assert lib.svo_resize(h, p, 832, 256, 800, 0, po, 416, 128, 416, 0, 1, 0, 0.5, 0.5, 0) == ERR_ARG       # pitch < width
    assert (out == 0).all()
    got = _plain_records(c, frames)
    for t, (g, w) in enumerate(zip(got, want)):
        _same(g, w, f"after the refused calls, frame {t}")
    # a valid creation, then a second one: SVO_ERR_ARG, and the stage stays what it was
    c.reset()
    c.ingest_create(832, 256, "linear", 0.5, 0.5)
    assert c.ingest_info() == (832, 256, 1, 0.5, 0.5)
    assert lib.svo_ingest_create(h, 832, 256, 0, 0.5, 0.5) == ERR_ARG
    assert c.ingest_info() == (832, 256, 1, 0.5, 0.5)
    # svo_add_frame's own argument rules, against the source size
    assert lib.svo_ingest_add_frame(h, p, p, 800, 0, ctypes.byref(res)) == ERR_ARG
    assert lib.svo_ingest_add_frame(h, p, None, 832, 0, ctypes.byref(res)) == ERR_ARG
    assert lib.svo_ingest_track_batch(h, p, p, 832, 832 * 256, 6, None, None, 1) == ERR_ARG                  # n_frames - 1 > max_batch
    assert lib.svo_ingest_streams_step(h, ctypes.c_void_p(ids.ctypes.data), 1, p, p, 832, 0, 0, ctypes.byref(res), 0) == ERR_ARG   # no stream set
    got = _plain_records(c, frames)
    for t, (g, w) in enumerate(zip(got, want)):
        _same(g, w, f"with an ingest stage, frame {t}")
    c.close()


def test_refused_ingest_stream_ids_stage_nothing(pkg, synth, tc):
    """svo_ingest_streams_step with host frames and stream ids it must refuse (twice the same, out of range, more than
    (max_batch + 1) / 2) answers SVO_ERR_ARG before anything is staged: stream 3, one frame in, goes on exactly as a fresh
    context fed the same frames alone."""
    seq, frames = _render(synth, tc, 832, 256, 4)
    P1, P2 = (pkg.scale_projection(P, 0.5, 0.5, "linear").reshape(12) for P in seq.proj())

    def make():
        c = pkg.Context(416, 128, device=0, P1=P1, P2=P2, max_batch=4)                      # LK, exact sums: the defaults
        assert c.cfg.track_mode == pkg.MODE_LK and c.cfg.lk_accum == pkg.LK_ACCUM_EXACT
        c.ingest_create(832, 256, "linear", 0.5, 0.5)
        return c

    fresh = make()
    alone = [fresh.ingest_add_frame(*frames[t])[1] for t in range(3)]
    fresh.close()
    _all_ok(alone)
    c = make()
    c.streams_create(4)
    L, R = [f[0] for f in frames], [f[1] for f in frames]
    _same(c.ingest_streams_step([3], L[:1], R[:1])[0], alone[0], "stream 3, frame 0")
    for bad_ids in ([3, 3], [4], [-1], [0, 1, 2]):
        m = len(bad_ids)
        ids = np.asarray(bad_ids, np.int32)
        fl, fr = np.stack([L[1]] * m), np.stack([R[1]] * m)
        out = np.zeros(m, dtype=pkg.STEP_DTYPE)
        rc = c.lib.svo_ingest_streams_step(c.h, ctypes.c_void_p(ids.ctypes.data), m, ctypes.c_void_p(fl.ctypes.data),
                                           ctypes.c_void_p(fr.ctypes.data), 832, 832 * 256, pkg.MEM_HOST,
                                           ctypes.c_void_p(out.ctypes.data), pkg.MEM_HOST)
        assert rc == ERR_ARG, (bad_ids, rc)
        assert not out.tobytes().strip(b"\0"), bad_ids
    _same(c.ingest_streams_step([3], L[1:2], R[1:2])[0], alone[1], "stream 3, frame 1")
    got = c.ingest_streams_step([1, 3], [L[0], L[2]], [R[0], R[2]])
    _same(got[0], alone[0], "stream 1, frame 0")
    _same(got[1], alone[2], "stream 3, frame 2")
    c.close()


# ---- g. the contract: svo_ingest_X == svo_X on _resize_ref frames -----------------------------------------------------------
#        (dw, dh, interp, f) for 832 x 256 sources
GEOMS = [(416, 128, "nearest", 0.5), (416, 128, "linear", 0.5), (499, 154, "linear", 0.0)]
MODES = ["exact", "sse2", "orb"]


def _mode_kw(pkg, mode):
    if mode == "orb":
        return dict(track_mode=pkg.MODE_ORB, **ORB_KW)
    return dict(lk_accum=pkg.LK_ACCUM_SSE2) if mode == "sse2" else {}


def _pair(pkg, seq, sw, sh, dw, dh, interp, f, **kw):
    """(context with an ingest stage, context without one), same configuration, P1 / P2 of the working size."""
    ix, iy = (f, f) if f else (dw / sw, dh / sh)
    P1, P2 = (pkg.scale_projection(P, ix, iy, interp).reshape(12) for P in seq.proj())
    a = pkg.Context(dw, dh, device=0, P1=P1, P2=P2, **kw)
    a.ingest_create(sw, sh, interp, f, f)
    assert a.ingest_info() == (sw, sh, int(interp == "linear"), ix, iy)
    b = pkg.Context(dw, dh, device=0, P1=P1, P2=P2, **kw)
    return a, b


def _small(frames, dw, dh, interp, f):
    return [tuple(RR.resize(x, dw, dh, interp, f, f) for x in fr) for fr in frames]


def _all_ok(records, first_is_init=True):
    for t, r in enumerate(records):
        assert int(r["ok"]) == 1, (t, r)
        if not (first_is_init and t == 0):
            assert int(r["n_tracked"]) > 0 and int(r["n_inliers"]) > 0, (t, r)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dw,dh,interp,f", GEOMS)
def test_ingest_add_frame_contract(pkg, synth, tc, dw, dh, interp, f, mode):
    seq, frames = _render(synth, tc, 832, 256, 4)
    small = _small(frames, dw, dh, interp, f)
    a, b = _pair(pkg, seq, 832, 256, dw, dh, interp, f, **_mode_kw(pkg, mode))
    recs = []
    for t, (fr, sm) in enumerate(zip(frames, small)):
        src = fr if t % 2 == 0 else tuple(tc.from_numpy(x).cuda() for x in fr)          # host and device frames alternate
        rca, ga = a.ingest_add_frame(*src)
        rcb, gb = b.add_frame(*sm)
        assert rca == rcb
        _same(ga, gb, f"frame {t}")
        _same_tracks(a.last_tracks(), b.last_tracks(), f"tracks of frame {t}")
        for side in ((0, 1) if mode == "orb" else (0,)):
            ka, kb = a.frame_keypoints(side, with_descriptors=mode == "orb"), b.frame_keypoints(side, with_descriptors=mode == "orb")
            if mode == "orb":
                assert ka[0].tobytes() == kb[0].tobytes() and ka[1].tobytes() == kb[1].tobytes() and len(ka[0]) > 0
            else:
                assert ka.tobytes() == kb.tobytes() and len(ka) > 0
        assert np.array_equal(a.get_pose(), b.get_pose())
        recs.append(ga)
    _all_ok(recs)
    a.close()
    b.close()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dw,dh,interp,f", GEOMS)
def test_ingest_track_batch_contract(pkg, synth, tc, dw, dh, interp, f, mode):
    seq, frames = _render(synth, tc, 832, 256, 4)
    small = _small(frames, dw, dh, interp, f)
    a, b = _pair(pkg, seq, 832, 256, dw, dh, interp, f, max_batch=3, **_mode_kw(pkg, mode))
    stack = lambda fs, k: tc.stack([tc.from_numpy(x[k]) for x in fs]).cuda()
    # padded source rows, host results; then device-resident results
    Lp = tc.zeros((4, 256, 896), dtype=tc.uint8, device="cuda")
    Rp = tc.zeros((4, 256, 896), dtype=tc.uint8, device="cuda")
    Lp[:, :, :832] = stack(frames, 0)
    Rp[:, :, :832] = stack(frames, 1)
    ga = a.ingest_track_batch(Lp[:, :, :832], Rp[:, :, :832])
    gb = b.track_batch(stack(small, 0), stack(small, 1))
    assert len(ga) == len(gb) == 3
    for p in range(3):
        _same(ga[p], gb[p], f"pair {p}")
        _same_tracks(a.batch_tracks(p), b.batch_tracks(p), f"tracks of pair {p}")
    _all_ok(ga, first_is_init=False)
    pose0 = np.eye(4)
    pose0[:3, 3] = (1.0, -2.0, 3.0)
    da = tc.zeros(3 * pkg.STEP_DTYPE.itemsize, dtype=tc.uint8, device="cuda")
    db = tc.zeros_like(da)
    a.ingest_track_batch(stack(frames, 0), stack(frames, 1), pose0=pose0, results=da)
    b.track_batch(stack(small, 0), stack(small, 1), pose0=pose0, results=db)
    a.sync()
    b.sync()
    ha, hb = (np.frombuffer(x.cpu().numpy().tobytes(), dtype=pkg.STEP_DTYPE) for x in (da, db))
    for p in range(3):
        _same(ha[p], hb[p], f"device results, pair {p}")
    _all_ok(ha, first_is_init=False)
    assert not np.array_equal(ha[0]["pose"], ga[0]["pose"])
    a.close()
    b.close()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dw,dh,interp,f", GEOMS)
def test_ingest_streams_step_contract(pkg, synth, tc, dw, dh, interp, f, mode):
    """Three streams of a set of five; ids a shuffled strict subset; stream 4 joins one call late, so call 1 holds an init
    item beside tracked items; host and device frames alternate; the last call leaves its records on the device."""
    seqs = [_render(synth, tc, 832, 256, 4, seed) for seed in (11, 12, 13)]
    smalls = [_small(fr, dw, dh, interp, f) for _, fr in seqs]
    a, b = _pair(pkg, seqs[0][0], 832, 256, dw, dh, interp, f, max_batch=7, **_mode_kw(pkg, mode))
    a.streams_create(5)
    b.streams_create(5)
    ids = [3, 0, 4]                                       # stream index s -> stream id
    calls = [[(1, 0), (0, 0)], [(2, 0), (0, 1), (1, 1)], [(1, 2), (2, 1), (0, 2)], [(0, 3), (2, 2), (1, 3)]]
    tracked = 0
    for k, call in enumerate(calls):
        sid = [ids[s] for s, _ in call]
        big = [np.stack([seqs[s][1][t][e] for s, t in call]) for e in (0, 1)]
        sm = [np.stack([smalls[s][t][e] for s, t in call]) for e in (0, 1)]
        if k % 2:
            big = [tc.from_numpy(x).cuda() for x in big]
        if k == len(calls) - 1:
            da = tc.zeros(len(call) * pkg.STEP_DTYPE.itemsize, dtype=tc.uint8, device="cuda")
            db = tc.zeros_like(da)
            a.ingest_streams_step(sid, big[0], big[1], results=da)
            b.streams_step(sid, tc.from_numpy(sm[0]).cuda(), tc.from_numpy(sm[1]).cuda(), results=db)
            a.sync()
            b.sync()
            ga, gb = (np.frombuffer(x.cpu().numpy().tobytes(), dtype=pkg.STEP_DTYPE) for x in (da, db))
        else:
            ga = a.ingest_streams_step(sid, big[0], big[1])
            gb = b.streams_step(sid, sm[0], sm[1])
        for i, (s, t) in enumerate(call):
            _same(ga[i], gb[i], f"call {k} item {i} (stream {ids[s]} frame {t})")
            _same_tracks(a.streams_tracks(i), b.streams_tracks(i), f"tracks of call {k} item {i}")
            assert int(ga[i]["ok"]) == 1
            if t == 0:
                assert int(ga[i]["n_prev_kps"]) == 0 and int(ga[i]["n_cur_kps"]) > 0
            else:
                assert int(ga[i]["n_tracked"]) > 0 and int(ga[i]["n_inliers"]) > 0
                tracked += 1
    assert tracked == 8
    for sid in range(5):
        assert np.array_equal(a.streams_get_pose(sid), b.streams_get_pose(sid))
    a.close()
    b.close()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dw,dh,interp,f", GEOMS)
def test_ingest_upload_contract(pkg, synth, tc, dw, dh, interp, f, mode):
    """Three chunks of a 7-frame sequence through ingest_upload_frames + track_uploaded_async, the halo frame of chunks 2 and
    3 carried on the device (first_slot = 1), against upload_frames of _resize_ref frames on the sibling context."""
    seq, frames = _render(synth, tc, 832, 256, 7)
    small = _small(frames, dw, dh, interp, f)
    a, b = _pair(pkg, seq, 832, 256, dw, dh, interp, f, max_batch=3, **_mode_kw(pkg, mode))
    ha = [a.host_frames(3, source_size=True) for _ in range(2)]
    hb = [b.host_frames(3) for _ in range(2)]
    assert ha[0].shape == (3, 256, 832) and hb[0].shape == (3, dh, dw)
    chunks = [(0, 3, 0), (3, 2, 1), (5, 2, 1)]           # (first new frame, new frames, first_slot)
    got_a, got_b = [], []
    for k, (t0, n, slot) in enumerate(chunks):
        buf = k & 1
        for c, host, fr in ((a, ha, frames), (b, hb, small)):
            for e in (0, 1):
                host[e][:n] = np.stack([fr[t][e] for t in range(t0, t0 + n)])
        a.ingest_upload_frames(buf, ha[0][:n], ha[1][:n], first_slot=slot)
        b.upload_frames(buf, hb[0][:n], hb[1][:n], first_slot=slot)
        for c in (a, b):
            c.wait_upload(buf)                            # the pinned buffers are refilled for the next chunk
            c.track_uploaded_async(buf, slot + n, continue_chain=k > 0, carry_frame=k > 0)
        n_pairs = slot + n - 1
        got_a.extend(a.collect_results(n_pairs))
        got_b.extend(b.collect_results(n_pairs))
        for p in range(n_pairs):
            _same_tracks(a.batch_tracks(p), b.batch_tracks(p), f"chunk {k} pair {p}")
    assert len(got_a) == len(got_b) == 6
    for p, (x, y) in enumerate(zip(got_a, got_b)):
        _same(x, y, f"pair {p}")
    _all_ok(got_a, first_is_init=False)
    a.close()
    b.close()


def test_orb_from_1080p(pkg, synth, tc):
    """The configuration that cannot be created at source size: ORB mode refuses a 1920 x 1080 context (2108 cells), the
    ingest path reaches it through a 960 x 540 one."""
    with pytest.raises(pkg.SvoError):
        pkg.Context(1920, 1080, device=0, track_mode=pkg.MODE_ORB)
    seq, frames = _render(synth, tc, 1920, 1080, 3)
    for interp in ("nearest", "linear"):
        small = _small(frames, 960, 540, interp, 0.5)
        a, b = _pair(pkg, seq, 1920, 1080, 960, 540, interp, 0.5, track_mode=pkg.MODE_ORB, max_batch=3, **ORB_KW)
        recs = []
        for t, (fr, sm) in enumerate(zip(frames, small)):
            src = fr if t % 2 else tuple(tc.from_numpy(x).cuda() for x in fr)
            rca, ga = a.ingest_add_frame(*src)
            rcb, gb = b.add_frame(*sm)
            assert rca == rcb == 0
            _same(ga, gb, f"{interp} frame {t}")
            _same_tracks(a.last_tracks(), b.last_tracks(), f"{interp} tracks of frame {t}")
            recs.append(ga)
        _all_ok(recs)
        L, R = (tc.stack([tc.from_numpy(x[e]) for x in frames]).cuda() for e in (0, 1))
        Ls, Rs = (tc.stack([tc.from_numpy(x[e]) for x in small]).cuda() for e in (0, 1))
        ga, gb = a.ingest_track_batch(L, R), b.track_batch(Ls, Rs)
        for p in range(2):
            _same(ga[p], gb[p], f"{interp} batch pair {p}")
            _same(ga[p], recs[p + 1], f"{interp} batch pair {p} against the online step")
        a.close()
        b.close()


# ---- h. directly against the oracle ---------------------------------------------------------------------------------------
def test_ingest_add_frame_against_the_oracle(pkg, oracle, synth, tc):
    seq, frames = _render(synth, tc, 832, 256, 4)
    small = _small(frames, 416, 128, "nearest", 0.5)
    P1, P2 = (RR.scale_projection(P, 0.5, 0.5, "nearest").reshape(12) for P in seq.proj())
    prm = oracle.make_params(P1, P2)
    a = pkg.Context(416, 128, device=0, P1=P1, P2=P2)
    a.ingest_create(832, 256, "nearest", 0.5, 0.5)
    rc, g0 = a.ingest_add_frame(*frames[0])
    kps = oracle.fast(small[0][0])
    assert rc == 0 and g0["ok"] == 1 and g0["n_cur_kps"] == len(kps)
    pose = np.eye(4)
    for t in range(1, 4):
        res, kps, pose = oracle.lk_track_step(prm, *small[t - 1], *small[t], kps, pose, want_tracks=True)
        rc, g = a.ingest_add_frame(*frames[t])
        assert rc == 0 and res["ok"] == 1
        _check_step(g, res)                              # integers exactly, relative motion to 1e-9
        tr = a.last_tracks()
        for got, want in zip(tr[:4], res["tracks"]):
            assert got.tobytes() == want.tobytes(), t    # LK floats bit for bit
        assert relfro(a.get_pose(), pose) <= TIGHT
    a.close()


# ---- i. non-interference --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["exact", "orb"])
def test_plain_calls_on_a_context_with_an_ingest_stage(pkg, synth, tc, mode):
    seq, frames = _render(synth, tc, 832, 256, 4)
    small = _small(frames, 416, 128, "linear", 0.5)
    a, b = _pair(pkg, seq, 832, 256, 416, 128, "linear", 0.5, max_batch=7, **_mode_kw(pkg, mode))
    a.ingest_add_frame(*frames[0])                        # the stage has been used ...
    a.reset()
    for t, sm in enumerate(small):                        # ... and the plain calls give what they give without it
        (rca, ga), (rcb, gb) = a.add_frame(*sm), b.add_frame(*sm)
        assert rca == rcb
        _same(ga, gb, f"add_frame {t}")
    Ls, Rs = (tc.stack([tc.from_numpy(x[e]) for x in small]).cuda() for e in (0, 1))
    ga, gb = a.track_batch(Ls, Rs), b.track_batch(Ls, Rs)
    for p in range(3):
        _same(ga[p], gb[p], f"track_batch pair {p}")
    _all_ok(ga, first_is_init=False)
    # ingest and plain steps interleaved on different streams of one set: stream 0 fed source-size frames through the stage,
    # stream 1 working-size frames of another sequence directly; both keep the record sequence of the sibling context
    _, frames2 = _render(synth, tc, 832, 256, 4, 12)
    small2 = _small(frames2, 416, 128, "linear", 0.5)
    a.streams_create(2)
    b.streams_create(2)
    for t in range(4):
        ra = a.ingest_streams_step([0], [frames[t][0]], [frames[t][1]])
        rb = b.streams_step([0], [small[t][0]], [small[t][1]])
        _same(ra[0], rb[0], f"ingest stream, frame {t}")
        ra = a.streams_step([1], [small2[t][0]], [small2[t][1]])
        rb = b.streams_step([1], [small2[t][0]], [small2[t][1]])
        _same(ra[0], rb[0], f"plain stream, frame {t}")
        assert int(ra[0]["ok"]) == 1 and (t == 0 or int(ra[0]["n_inliers"]) > 0)
    for sid in (0, 1):
        assert np.array_equal(a.streams_get_pose(sid), b.streams_get_pose(sid))
    a.close()
    b.close()


# ---- j. the runner: image_scale against hand-downscaled files -----------------------------------------------------------------
from test_host_api import _write_pgm, _write_yaml, host_built   # noqa: E402,F401  (host_built: the fixture that builds host/)


def _dataset(d, frames):
    for cam in (0, 1):
        os.makedirs(d / f"image_{cam}")
    for t, fr in enumerate(frames):
        for cam in (0, 1):
            _write_pgm(d / f"image_{cam}" / f"{t:06d}.pgm", fr[cam])


@pytest.mark.parametrize("interp", ["nearest", "linear"])
def test_runner_image_scale(host_built, synth, tc, tmp_path, interp):
    """run_kitti_stereo on 832 x 256 files with image_scale: 0.5 writes the pose file it writes on the _resize_ref-downscaled
    416 x 128 files with the camera keys scaled by hand and no image_scale, byte for byte (0.5 is a power of two: the YAML
    route and svo_scale_projection give identical doubles): per-frame loop, batch_size 8, stream_depth 2 (LK and ORB), and
    three sequences under --interleave."""
    exe = os.path.join(host_built, "run_kitti_stereo")
    f = 0.5
    o = 0.5 * (f - 1) if interp == "linear" else 0.0
    specs = [(11, 12), (12, 7), (13, 9)]                  # (seed, frames)
    big_y, small_y = [], []
    for k, (seed, n) in enumerate(specs):
        seq, frames = _render(synth, tc, 832, 256, n, seed)
        _dataset(tmp_path / f"big{k}", frames)
        _dataset(tmp_path / f"small{k}", _small(frames, 416, 128, interp, f))
        big_y.append((tmp_path / f"big{k}", dict(fx=seq.fx, fy=seq.fy, cx=seq.cx, cy=seq.cy)))
        small_y.append((tmp_path / f"small{k}", dict(fx=seq.fx * f, fy=seq.fy * f, cx=seq.cx * f + o, cy=seq.cy * f + o)))

    def yaml(name, k, small, mode, extra):
        d, cam = (small_y if small else big_y)[k]
        y = tmp_path / name
        _write_yaml(y, str(d), mode=mode, **cam)
        with open(y, "a", encoding="utf-8") as fh:
            fh.write(extra + ("" if small else f"image_scale: {f}\nimage_interp: {interp}\n"))
        return str(y)

    def run(args):
        r = subprocess.run([exe] + args, capture_output=True, timeout=600)
        assert r.returncode == 0, r.stderr.decode()[-3000:]

    cases = [("LK_stereof2f_pnp", ""), ("LK_stereof2f_pnp", "batch_size: 8\n"), ("LK_stereof2f_pnp", "stream_depth: 2\n"),
             ("ORB_stereof2f_pnp", ""), ("ORB_stereof2f_pnp", "batch_size: 8\n")]
    for i, (mode, extra) in enumerate(cases):
        got, want = str(tmp_path / f"got{i}.txt"), str(tmp_path / f"want{i}.txt")
        run([yaml(f"big_{i}.yaml", 0, False, mode, extra), got])
        run([yaml(f"small_{i}.yaml", 0, True, mode, extra), want])
        a, b = open(got, "rb").read(), open(want, "rb").read()
        assert a == b and len(a.splitlines()) == specs[0][1], (mode, extra)
        poses = np.loadtxt(got).reshape(-1, 3, 4)
        assert np.abs(poses[-1][:, 3]).max() > 1.0        # the camera has moved: the steps were tracked, not skipped
    for mode in ("LK_stereof2f_pnp", "ORB_stereof2f_pnp"):
        for small in (False, True):
            out = tmp_path / f"out_{mode}_{int(small)}"
            os.makedirs(out)
            ys = [yaml(f"il{k}_{mode}_{int(small)}.yaml", k, small, mode, "") for k in range(3)]
            run(ys + ["--poses-dir", str(out), "--interleave"])
        for k, (_, n) in enumerate(specs):
            a = open(tmp_path / f"out_{mode}_0" / f"il{k}_{mode}_0.yaml.poses.txt", "rb").read()
            b = open(tmp_path / f"out_{mode}_1" / f"il{k}_{mode}_1.yaml.poses.txt", "rb").read()
            assert a == b and len(a.splitlines()) == n, (mode, k)
