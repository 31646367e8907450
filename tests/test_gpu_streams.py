"""Stream sets (svo_streams_*): many independent live stereo streams advanced through ONE launch set per call.

Every record is held against two yardsticks, neither of which is the code under test:
  - the CPU oracle run on each sequence ALONE, with the tolerances of the existing parity tests (_check_step, pose <= TIGHT);
  - the library's own svo_add_frame on a fresh one-stream context per sequence, BYTE FOR BYTE on the whole record
    (T_rel_inv, pose, rvec, tvec, R and every integer field)."""
import os
import subprocess

import numpy as np
import pytest

from test_gpu_parity_orb import _check_orb_step, _oracle_orb_sequence
from test_gpu_parity_pose import TIGHT, _check_step, _oracle_sequence, relfro


@pytest.fixture(scope="module")
def tc():
    import torch
    return torch


LK_SPECS = [(11, 4), (12, 6), (13, 3), (14, 7), (15, 5)]          # (seed, n_frames), 416x128: 20 pairs
LK_IDS = [6, 0, 3, 7, 2]                                          # 5 of 8 streams, not in order
ORB_SPECS = [(5, 4), (6, 3), (7, 5)]                              # 832x256: 9 pairs
ORB_KW = dict(min_move2=0.05 ** 2, max_move2=10.0 ** 2)


def _render(synth, w, h, n, seed):
    seq = synth.StereoSequence(width=w, height=h, n_frames=n, seed=seed)
    return seq, [tuple(x.numpy() for x in seq.render(t)) for t in range(n)]


def _alone(pkg, seq, frames, **kw):
    """The records svo_add_frame gives for these frames on a fresh context of its own (record 0: the init record)."""
    h, w = frames[0][0].shape
    P1s, P2s = seq.proj()
    c = pkg.Context(w, h, device=0, P1=P1s, P2=P2s, **kw)
    out = [c.add_frame(*f)[1] for f in frames]
    c.close()
    return out


def _same(g, a, what=""):
    for name in g.dtype.names:
        assert np.asarray(g[name]).tobytes() == np.asarray(a[name]).tobytes(), f"{what}: field {name} differs: {g[name]} != {a[name]}"
    assert g.tobytes() == a.tobytes(), what


def _schedule(lengths, seed, late, late_from, pattern):
    """Which streams (indices into `lengths`) each call advances: call c takes pattern[c % len] of the streams that still
    have a frame, in a seeded random order; stream `late` joins at call `late_from`."""
    rng = np.random.default_rng(seed)
    nxt = [0] * len(lengths)
    calls = []
    while any(nxt[s] < lengths[s] for s in range(len(lengths))):
        c = len(calls)
        avail = [s for s in range(len(lengths)) if nxt[s] < lengths[s] and (s != late or c >= late_from)]
        pick = [int(s) for s in rng.permutation(avail)[:min(pattern[c % len(pattern)], len(avail))]]
        calls.append([(s, nxt[s]) for s in pick])
        for s in pick:
            nxt[s] += 1
    return calls


def _check_schedule(calls, n_streams, want_m):
    ms = {len(c) for c in calls}
    assert ms >= set(want_m), ms                                                    # (a) m varies over the whole range
    orders = [[s for s, _ in c] for c in calls if len(c) >= 2]
    assert any(sorted(o) != o for o in orders)                                      # (b) ids not in a fixed order
    sat_out = False
    for s in range(n_streams):
        played = [any(x == s for x, _ in c) for c in calls]
        first, last = played.index(True), len(played) - 1 - played[::-1].index(True)
        sat_out |= any(not played[k] and not played[k + 1] for k in range(first, last))
    assert sat_out                                                                  # (c) a live stream sits out two calls running
    assert any({t for _, t in c} >= {0} and any(t > 0 for _, t in c) for c in calls[1:])   # (d) init and track records share a call


def _run_schedule(pkg, tc, c, calls, ids, frames):
    """Plays the schedule on context c; returns {(stream index, frame index): record}.  Host and device frames alternate."""
    got = {}
    for k, call in enumerate(calls):
        Ls = np.stack([frames[s][t][0] for s, t in call])
        Rs = np.stack([frames[s][t][1] for s, t in call])
        if k % 2:
            Ls, Rs = tc.from_numpy(Ls).cuda(), tc.from_numpy(Rs).cuda()
        res = c.streams_step([ids[s] for s, _ in call], Ls, Rs)
        assert len(res) == len(call)
        for (s, t), r in zip(call, res):
            got[(s, t)] = r.copy()
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("accum", ["exact", "sse2"])
def test_interleaved_streams_parity_lk(pkg, oracle, synth, tc, accum):
    specs = LK_SPECS if accum == "exact" else [LK_SPECS[0], LK_SPECS[2]]
    ids = LK_IDS[:len(specs)]
    kw = {} if accum == "exact" else dict(lk_accum=pkg.LK_ACCUM_SSE2)
    seqs = [_render(synth, 416, 128, n, s) for s, n in specs]
    old = oracle.set_lk_accum(oracle.LK_ACCUM_FLOAT_SSE) if accum == "sse2" else None
    try:
        refs = [_oracle_sequence(oracle, seq, fr) for seq, fr in seqs]
    finally:
        if old is not None:
            oracle.set_lk_accum(old)
    alone = [_alone(pkg, seq, fr, **kw) for seq, fr in seqs]
    lengths = [n for _, n in specs]
    if accum == "exact":
        calls = _schedule(lengths, seed=2024, late=2, late_from=3, pattern=[1, 3, 2, 5, 4])
        _check_schedule(calls, len(specs), [1, 2, 3, 4, 5])
    else:
        calls = _schedule(lengths, seed=7, late=1, late_from=2, pattern=[1, 2])
    P1s, P2s = seqs[0][0].proj()
    c = pkg.Context(416, 128, device=0, P1=P1s, P2=P2s, max_batch=9, **kw)
    assert c.streams_count() == 0
    c.streams_create(8)
    assert c.streams_count() == 8
    got = _run_schedule(pkg, tc, c, calls, ids, [fr for _, fr in seqs])
    tracked = 0
    for s, (seq, fr) in enumerate(seqs):
        for t in range(len(fr)):
            g = got[(s, t)]
            _same(g, alone[s][t], f"stream {ids[s]} frame {t}")
            if t == 0:
                assert g["ok"] == 1 and g["n_prev_kps"] == 0 and g["n_cur_kps"] == len(oracle.fast(fr[0][0]))
                assert np.array_equal(g["pose"].reshape(4, 4), np.eye(4)) and np.array_equal(g["T_rel_inv"].reshape(4, 4), np.eye(4))
                continue
            r, pose = refs[s][t - 1]
            assert r["ok"] == 1
            _check_step(g, r)
            assert relfro(g["pose"].reshape(4, 4), pose) <= TIGHT
            tracked += 1
        assert np.array_equal(c.streams_get_pose(ids[s]), got[(s, len(fr) - 1)]["pose"].reshape(4, 4))
    assert tracked == sum(lengths) - len(lengths) and (accum != "exact" or tracked == 20)       # no case skipped
    for sid in set(range(8)) - set(ids):                                                         # untouched streams stay at identity
        assert np.array_equal(c.streams_get_pose(sid), np.eye(4))
    c.close()


@pytest.mark.gpu
def test_interleaved_streams_parity_orb(pkg, oracle, synth, tc):
    seqs = [_render(synth, 832, 256, n, s) for s, n in ORB_SPECS]
    kw = dict(track_mode=pkg.MODE_ORB, **ORB_KW)
    refs = [_oracle_orb_sequence(oracle, seq, fr) for seq, fr in seqs]
    alone = [_alone(pkg, seq, fr, **kw) for seq, fr in seqs]
    lengths = [n for _, n in ORB_SPECS]
    ids = [2, 0, 3]
    calls = _schedule(lengths, seed=100, late=1, late_from=2, pattern=[1, 3, 2])
    _check_schedule(calls, 3, [1, 2, 3])
    P1s, P2s = seqs[0][0].proj()
    c = pkg.Context(832, 256, device=0, P1=P1s, P2=P2s, max_batch=5, **kw)
    c.streams_create(4)
    got = _run_schedule(pkg, tc, c, calls, ids, [fr for _, fr in seqs])
    tracked = 0
    for s, (seq, fr) in enumerate(seqs):
        ref, feats = refs[s]
        for t in range(len(fr)):
            g = got[(s, t)]
            _same(g, alone[s][t], f"stream {ids[s]} frame {t}")
            if t == 0:
                assert g["ok"] == 1 and g["n_prev_kps"] == 0 and g["n_cur_kps"] == len(feats[0][0][0])
                continue
            r, pose = ref[t - 1]
            assert r["ok"] == 1
            _check_orb_step(g, r)
            assert relfro(g["pose"].reshape(4, 4), pose) <= TIGHT
            tracked += 1
        assert np.array_equal(c.streams_get_pose(ids[s]), got[(s, len(fr) - 1)]["pose"].reshape(4, 4))
    assert tracked == 9                                                                          # no case skipped
    c.close()


@pytest.mark.gpu
def test_failures_stay_in_their_stream(pkg, oracle, synth, tc):
    (seqA, fA), (seqB, fB) = _render(synth, 416, 128, 4, 11), _render(synth, 416, 128, 3, 12)
    flat = np.full((128, 416), 90, np.uint8)
    framesB = [fB[0], (flat, flat), fB[2]]
    P1s, P2s = seqA.proj()
    prm = oracle.make_params(P1s, P2s)
    aloneA = _alone(pkg, seqA, fA)
    c = pkg.Context(416, 128, device=0, P1=P1s, P2=P2s, max_batch=3)
    c.streams_create(2)
    A, B = 1, 0
    recs = [c.streams_step([A, B], [fA[t][0], framesB[t][0]], [fA[t][1], framesB[t][1]]) for t in range(3)]
    for t in range(3):
        _same(recs[t][0], aloneA[t], f"stream A frame {t}")
    kps = oracle.fast(fB[0][0])
    r1, kps2, pose = oracle.lk_track_step(prm, *framesB[0], *framesB[1], kps, np.eye(4))
    r2, _, pose = oracle.lk_track_step(prm, *framesB[1], *framesB[2], kps2, pose)
    assert r1["fail_stage"] == 1 and r2["fail_stage"] == 2
    _check_step(recs[1][1], r1)
    _check_step(recs[2][1], r2)
    assert recs[1][1]["ok"] == 0 and recs[2][1]["ok"] == 0
    for t in range(3):
        assert np.array_equal(recs[t][1]["pose"].reshape(4, 4), np.eye(4))
    assert np.array_equal(c.streams_get_pose(B), np.eye(4)) and np.array_equal(pose, np.eye(4))
    assert np.array_equal(c.streams_get_pose(A), aloneA[2]["pose"].reshape(4, 4))
    c.close()


@pytest.mark.gpu
def test_reset_and_seed(pkg, synth, tc):
    seqs = [_render(synth, 416, 128, 4, s) for s in (11, 12, 14)]
    alone = [_alone(pkg, seq, fr) for seq, fr in seqs]
    P1s, P2s = seqs[0][0].proj()
    c = pkg.Context(416, 128, device=0, P1=P1s, P2=P2s, max_batch=5)
    c.streams_create(3)
    ids = [2, 0, 1]

    def step(t):
        return c.streams_step(ids, [seqs[k][1][t][0] for k in range(3)], [seqs[k][1][t][1] for k in range(3)])
    for t in range(2):
        res = step(t)
        for k in range(3):
            _same(res[k], alone[k][t])
    c.streams_reset(ids[1])
    assert np.array_equal(c.streams_get_pose(ids[1]), np.eye(4))
    res = step(2)
    _same(res[0], alone[0][2])
    _same(res[2], alone[2][2])
    g = res[1]                                             # the reset stream: an init record on frame 2, pose = identity
    assert g["ok"] == 1 and g["fail_stage"] == 0 and g["n_prev_kps"] == 0 and g["n_tracked"] == 0
    assert g["n_cur_kps"] == alone[1][2]["n_cur_kps"]
    assert np.array_equal(g["pose"].reshape(4, 4), np.eye(4)) and np.array_equal(g["T_rel_inv"].reshape(4, 4), np.eye(4))
    res = step(3)
    _same(res[0], alone[0][3])
    _same(res[2], alone[2][3])
    g = res[1]                                             # ... and it tracks frame 2 -> 3 from identity
    a = alone[1][3]
    for name in ("ok", "fail_stage", "n_prev_kps", "n_cur_kps", "n_tracked", "n_inliers", "rvec", "tvec", "R", "T_rel_inv"):
        assert np.asarray(g[name]).tobytes() == np.asarray(a[name]).tobytes(), name
    assert g["ok"] == 1 and np.array_equal(g["pose"], g["T_rel_inv"])
    # reset of every stream
    c.streams_reset()
    for sid in range(3):
        assert np.array_equal(c.streams_get_pose(sid), np.eye(4))
    assert all(r["n_prev_kps"] == 0 and r["ok"] == 1 for r in step(0))
    c.close()
    # streams_set_pose seeds a stream's chain as pose0 seeds track_batch
    seq, fr = seqs[0]
    th = 0.3
    pose0 = np.array([[np.cos(th), 0, np.sin(th), 1.5], [0, 1, 0, -0.25], [-np.sin(th), 0, np.cos(th), 7.0], [0, 0, 0, 1]])
    c = pkg.Context(416, 128, device=0, P1=P1s, P2=P2s, max_batch=3)
    L = tc.stack([tc.from_numpy(f[0]) for f in fr]).cuda()
    R = tc.stack([tc.from_numpy(f[1]) for f in fr]).cuda()
    want = c.track_batch(L, R, pose0=pose0)
    assert all(want["ok"] == 1)
    c.streams_create(2)
    c.streams_set_pose(1, pose0)
    assert np.array_equal(c.streams_get_pose(1), pose0)
    g0 = c.streams_step([1], [fr[0][0]], [fr[0][1]])[0]
    assert np.array_equal(g0["pose"].reshape(4, 4), pose0)
    for t in range(1, 4):
        g = c.streams_step([1], L[t:t + 1], R[t:t + 1])[0]
        _same(g, want[t - 1], f"seeded chain, pair {t - 1}")
    assert np.array_equal(c.streams_get_pose(1), want[2]["pose"].reshape(4, 4))
    assert np.array_equal(c.streams_get_pose(0), np.eye(4))
    c.close()


@pytest.mark.gpu
def test_stream_set_coexists_with_the_other_entry_points(pkg, synth, tc):
    seqs = [_render(synth, 416, 128, 3, s) for s in (11, 12)]
    alone = [_alone(pkg, seq, fr) for seq, fr in seqs]
    sequ, fu = _render(synth, 416, 128, 4, 15)                       # unrelated frames for the non-stream calls
    P1s, P2s = seqs[0][0].proj()
    Lu = tc.stack([tc.from_numpy(f[0]) for f in fu]).cuda()
    Ru = tc.stack([tc.from_numpy(f[1]) for f in fu]).cuda()

    def others(c):
        c.reset()
        a0 = c.add_frame(*fu[0])[1]
        a1 = c.add_frame(*fu[1])[1]
        b = c.track_batch(Lu, Ru)
        return a0.tobytes() + a1.tobytes() + b.tobytes(), b
    plain = pkg.Context(416, 128, device=0, P1=P1s, P2=P2s, max_batch=5)
    want, b = others(plain)
    plain.close()
    assert all(b["ok"] == 1)
    c = pkg.Context(416, 128, device=0, P1=P1s, P2=P2s, max_batch=5)
    c.streams_create(3)
    ids = [2, 0]

    def step(t):
        return c.streams_step(ids, [seqs[k][1][t][0] for k in range(2)], [seqs[k][1][t][1] for k in range(2)])
    res = step(0)
    got, _ = others(c)
    assert got == want
    res = step(1)
    for k in range(2):
        _same(res[k], alone[k][1])
    tr = c.streams_tracks(0)
    assert len(tr[0]) == res[0]["n_tracked"] and int(tr[4].sum()) == res[0]["n_inliers"]
    got, _ = others(c)
    assert got == want
    res = step(2)
    for k in range(2):
        _same(res[k], alone[k][2])
    c.close()


@pytest.mark.gpu
def test_stream_step_arguments(pkg, synth, tc):
    seq, fr = _render(synth, 416, 128, 3, 11)
    alone = _alone(pkg, seq, fr)
    P1s, P2s = seq.proj()
    c = pkg.Context(416, 128, device=0, P1=P1s, P2=P2s, max_batch=4)          # m <= (4 + 1) / 2 = 2
    L, R = [f[0] for f in fr], [f[1] for f in fr]
    with pytest.raises(pkg.SvoError):
        c.streams_step([0], L[:1], R[:1])                                      # no stream set yet
    with pytest.raises(pkg.SvoError):
        c.streams_create(0)
    c.streams_create(4)
    with pytest.raises(pkg.SvoError):
        c.streams_create(4)                                                    # once per context
    _same(c.streams_step([3], L[:1], R[:1])[0], alone[0])
    for bad_ids in ([3, 3], [4], [-1], [0, 1, 2]):                             # duplicate, out of range (twice), over the cap
        with pytest.raises(pkg.SvoError):
            c.streams_step(bad_ids, [L[1]] * len(bad_ids), [R[1]] * len(bad_ids))
    with pytest.raises(pkg.SvoError):
        c.streams_step([], None, None)                                         # m = 0
    for bad in (4, -2):
        with pytest.raises(pkg.SvoError):
            c.streams_get_pose(bad)
        with pytest.raises(pkg.SvoError):
            c.streams_reset(bad)
    # none of the refused calls advanced stream 3
    _same(c.streams_step([3], L[1:2], R[1:2])[0], alone[1])
    _same(c.streams_step([1, 3], [L[0], L[2]], [R[0], R[2]])[1], alone[2])
    c.close()


@pytest.mark.gpu
def test_wide_step_64_streams_fullsize(pkg, oracle, synth, tc):
    """One full-size step set: m = 64 streams at 1241x376 on a context with max_batch = 127 (init call, track call); beyond one
    table entry per wave in the gather / scatter and one workgroup in the per-stream finalize."""
    W, H, M = 1241, 376, 64
    seqs = [_render(synth, W, H, 2, s) for s in (3, 4)]
    odd = {5: 1, 17: 1, 40: 1, 63: 1}                                         # items fed the other sequence
    alone = [_alone(pkg, seq, fr) for seq, fr in seqs]
    P1s, P2s = seqs[0][0].proj()
    c = pkg.Context(W, H, device=0, P1=P1s, P2=P2s, max_batch=127)
    c.streams_create(M)
    ids = [(37 * i + 11) % M for i in range(M)]                               # a permutation of 0..63
    assert sorted(ids) == list(range(M))
    recs = []
    for t in range(2):
        Ls = tc.stack([tc.from_numpy(seqs[odd.get(i, 0)][1][t][0]) for i in range(M)]).cuda()
        Rs = tc.stack([tc.from_numpy(seqs[odd.get(i, 0)][1][t][1]) for i in range(M)]).cuda()
        recs.append(c.streams_step(ids, Ls, Rs))
    for i in range(M):
        k = odd.get(i, 0)
        _same(recs[0][i], alone[k][0], f"item {i} init")
        _same(recs[1][i], alone[k][1], f"item {i} track")
        assert np.array_equal(c.streams_get_pose(ids[i]), alone[k][1]["pose"].reshape(4, 4))
    for k, i in ((0, 0), (1, 17)):
        r, pose = _oracle_sequence(oracle, *seqs[k])[0]
        assert r["ok"] == 1
        _check_step(recs[1][i], r)
        assert relfro(recs[1][i]["pose"].reshape(4, 4), pose) <= TIGHT
    c.close()


# ---- the runner: run_kitti_stereo a.yaml b.yaml c.yaml --poses-dir out --interleave ------------------------------------
def _host():
    import test_host_api as H
    return H


@pytest.fixture(scope="module")
def host_exe(pkg):
    H = _host()
    pkg.build_library()
    subprocess.check_call(["make", "-C", H.HOST], stdout=subprocess.DEVNULL)
    return os.path.join(H.HOST, "run_kitti_stereo")


def _write_sequence(H, synth, root, name, n, seed, **yaml_kw):
    seq = synth.StereoSequence(width=416, height=128, n_frames=n, seed=seed)
    d = root / name
    for cam in (0, 1):
        os.makedirs(d / f"image_{cam}")
    for t in range(n):
        L, R = (x.numpy() for x in seq.render(t))
        H._write_pgm(d / "image_0" / f"{t:06d}.pgm", L)
        H._write_pgm(d / "image_1" / f"{t:06d}.pgm", R)
    y = root / f"{name}.yaml"
    kw = dict(fx=seq.fx, fy=seq.fy, cx=seq.cx, cy=seq.cy)
    kw.update(yaml_kw)
    H._write_yaml(y, str(d), **kw)
    return str(y)


@pytest.mark.gpu
def test_runner_interleaves_sequences_of_different_lengths(host_exe, synth, tmp_path):
    H = _host()
    specs = [("s0", 6, 21), ("s1", 4, 22), ("s2", 9, 23)]
    yamls = [_write_sequence(H, synth, tmp_path, name, n, seed) for name, n, seed in specs]
    single = []
    for y in yamls:
        r = subprocess.run([host_exe, y, y + ".single.txt"], capture_output=True, timeout=300)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        single.append(open(y + ".single.txt", "rb").read())
    os.makedirs(tmp_path / "out")
    r = subprocess.run([host_exe] + yamls + ["--poses-dir", str(tmp_path / "out"), "--interleave"], capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    for (name, n, _), want in zip(specs, single):
        got = open(tmp_path / "out" / f"{name}.yaml.poses.txt", "rb").read()
        assert len(want.splitlines()) == n and got == want, name


def test_runner_refuses_streams_with_different_cameras(host_exe, synth, tmp_path):
    """No GPU needed: the runner compares the YAMLs and exits before it creates a context."""
    H = _host()
    yamls = [_write_sequence(H, synth, tmp_path, name, 2, seed) for name, seed in (("a", 21), ("b", 22))]
    other = _write_sequence(H, synth, tmp_path, "d", 2, 24, fx=700.0)
    os.makedirs(tmp_path / "out")
    r = subprocess.run([host_exe] + yamls + [other, "--poses-dir", str(tmp_path / "out"), "--interleave"], capture_output=True,
                       timeout=120)
    err = r.stderr.decode()
    assert r.returncode != 0 and "camera_l.fx" in err, err[-2000:]
    assert not os.listdir(tmp_path / "out")                                   # refused before anything was written


@pytest.mark.gpu
def test_stream_step_timing_names_the_copies(pkg, synth, tc):
    seq, fr = _render(synth, 416, 128, 2, 11)
    P1s, P2s = seq.proj()
    c = pkg.Context(416, 128, device=0, P1=P1s, P2=P2s, max_batch=3)
    c.streams_create(2)
    c.enable_timing(True)
    for t in range(2):
        c.streams_step([1, 0], [fr[t][0]] * 2, [fr[t][1]] * 2)
    names = [n for n, _ in c.get_timing()]
    for want in ("stream_gather", "pyramid", "fast", "stream_scatter", "lk", "compact", "triangulate", "pnp", "finalize"):
        assert want in names, names
    assert all(ms >= 0 for _, ms in c.get_timing()) and "start" not in names
    c.close()
