"""HIP vs the CPU oracle on natural image content (-m gpu), at 1241x376.

Every other parity test runs on the renderer's hashed value noise or on random blocks.  Here the corridor is walled with
two photographs that ship with installed packages (sklearn's china.jpg, matplotlib's grace_hopper.jpg; loaded at run
time, nothing committed) and with a procedural 1/f texture, under four photometric variants (tests/_natural.py):
`day` (identity), `overexposed` (gain 1.8: large saturated areas), `night` (gain 0.23: max <= 60, contrast near FAST's
threshold) and `lr_mismatch` (right camera gain 1.1, offset +8: the stereo half of the circular LK chain runs without
brightness constancy).  That content reaches the minimum-FAST-threshold retry of the ORB cells, ORB levels short of
their quota, LK windows rejected on minEig, and long LK iteration counts on smooth gradients.

Bars are the existing ones: FAST keypoints, pyramid bytes, LK points and status in all four lk_accum orders, ORB
pyramids / candidates / keypoints / descriptors / matches, tracks, 3-D points, RANSAC records and masks byte-equal;
pose within 1e-4 relative Frobenius with the observed 1e-9 asserted as well.  Guards assert on the oracle's side that
the content did reach those paths, so that a renderer change cannot quietly turn these tests back into value noise."""
import numpy as np
import pytest

import _natural
from _natural import TEXTURES, VARIANTS
from test_gpu_parity_lk_sse2 import accum_oracle
from test_gpu_parity_sequence import _check_batch, _check_online, _check_orb_sequence, _oracle_lk_sequence

pytestmark = pytest.mark.gpu
W, H = 1241, 376
BIG = 1 << 15                       # keypoint capacity: FAST(20) finds up to ~16 000 corners on the 1/f texture


@pytest.fixture(scope="module")
def tc():
    import torch
    assert torch.cuda.is_available()
    return torch


_CACHE = {}


def _frames(synth, tc, name, variant, n):
    """(seq, [(L, R) uint8 numpy]) rendered on the GPU, with the variant's evidence asserted on what was rendered."""
    key = (name, variant, n)
    if key not in _CACHE:
        seq = _natural.sequence(synth, name, variant, width=W, height=H, n_frames=n, device=tc.device("cuda", 0))
        frames = [tuple(x.cpu().numpy() for x in seq.render(t)) for t in range(n)]
        if variant == "overexposed":
            assert min(_natural.saturated_fraction(L) for L, _ in frames) >= 0.05
        if variant == "night":
            assert max(max(L.max(), R.max()) for L, R in frames) <= 60
        _CACHE[key] = (seq, frames)
    return _CACHE[key]


ORDERS = [("exact", 0, 0), ("sse2", 1, 2), ("simd128", 2, 4), ("sse2_legacy", 3, 3)]     # (name, svo lk_accum, oracle mode)


# ---- stages ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", TEXTURES)
def test_fast_natural(pkg, oracle, synth, tc, name, variant):
    _, frames = _frames(synth, tc, name, variant, 2)
    c = pkg.Context(W, H, device=0, max_keypoints=W * H)
    for img in frames[0]:
        for thr in (20, 7):
            for nms in (True, False):
                ref = oracle.fast(img, thr, nms, cap=W * H)
                assert c.fast_detect(img, thr, nms, cap=W * H).tobytes() == ref.tobytes(), (thr, nms)
        assert c.fast_detect(tc.from_numpy(img).cuda(), 7, True, cap=W * H).tobytes() == oracle.fast(img, 7, True).tobytes()
    c.close()


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", TEXTURES)
def test_pyramid_natural(pkg, oracle, synth, tc, name, variant):
    _, frames = _frames(synth, tc, name, variant, 2)
    c = pkg.Context(W, H, device=0)
    for s, img in enumerate(frames[0]):
        c.build_pyramid(s, img)
        ref = oracle.PyramidHandle(img)
        assert c.num_levels == ref.nlevels
        for lv in range(ref.nlevels):
            assert np.array_equal(c.read_pyramid_level(s, lv), ref.level(lv)), (s, lv)
    c.close()


def _lk_points(oracle, img, n_rand, seed):
    """The oracle's FAST(20) corners plus random points over the whole frame and 3 px beyond it (windows hanging over
    the edge), a quarter of them at integer positions."""
    kp = oracle.fast(img)
    rng = np.random.default_rng(seed)
    rnd = np.stack([rng.uniform(-3, W + 3, n_rand), rng.uniform(-3, H + 3, n_rand)], 1)
    rnd[: n_rand // 4] = np.round(rnd[: n_rand // 4])
    return np.concatenate([np.stack([kp["x"], kp["y"]], 1), rnd]).astype(np.float32)


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", TEXTURES)
def test_lk_single_call_all_orders_natural(pkg, oracle, synth, tc, name, variant):
    """One cv::calcOpticalFlowPyrLK call, frame t -> t+1 (left) and L -> R, in all four accumulation orders against
    the oracle in the same mode: points and status bytes."""
    _, frames = _frames(synth, tc, name, variant, 2)
    (L0, R0), (L1, _) = frames
    pts = _lk_points(oracle, L0, 2000, 17)
    pyr = [oracle.PyramidHandle(im) for im in (L0, L1, R0)]
    outs = {}
    for oname, svo_mode, o_mode in ORDERS:
        c = pkg.Context(W, H, device=0, max_keypoints=BIG, lk_accum=svo_mode)
        for s, im in enumerate((L0, L1, R0)):
            c.build_pyramid(s, im)
        for dst in (1, 2):
            got, st = c.lk_track(0, dst, pts)
            with accum_oracle(oracle, o_mode):
                want, wst = oracle.lk_track(pyr[0], pyr[dst], pts)
            assert st.tobytes() == wst.tobytes(), (oname, dst)
            assert got.tobytes() == want.tobytes(), (oname, dst)
            outs[oname, dst] = (want, wst)
        c.close()
    # the float orders do change bits on this content (else the comparison proves little) -- except at night: with
    # intensities <= 60 the LK sums stay small and the four orders were observed to agree bit for bit
    if variant != "night" and outs["exact", 1][1].sum() >= 1000:
        assert any(outs[o, d][0].tobytes() != outs["exact", d][0].tobytes() for o, _, _ in ORDERS[1:] for d in (1, 2))


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", TEXTURES)
def test_orb_extract_and_match_natural(pkg, oracle, synth, tc, name, variant):
    """ORBextractor on both views: pyramid levels, cell-FAST candidates, keypoints, descriptors; then match_hamming
    L -> R."""
    _, frames = _frames(synth, tc, name, variant, 2)
    _, _, quota, _ = oracle.orb_setup()
    c = pkg.Context(W, H, device=0, track_mode=pkg.MODE_ORB, max_keypoints=16384)      # ORB mode's largest capacity
    feats, short = [], False
    for img in frames[0]:
        kps, desc, per = c.orb_extract(img)
        rk, rd, rper = oracle.orb_extract(img)
        for lv in range(8):
            assert np.array_equal(c.orb_read_level(lv), oracle.orb_pyramid_level(img, lv)), lv
            assert c.orb_read_candidates(lv, cap=1 << 16).tobytes() == oracle.orb_candidates(img, lv).tobytes(), lv
        assert per.tolist() == rper.tolist()
        assert kps.tobytes() == rk.tobytes() and desc.tobytes() == rd.tobytes()
        short |= bool((rper < quota).any())
        feats.append((rk, rd))
    (kL, dL), (kR, dR) = feats
    assert len(kL) > 0 and len(kR) > 0
    idx, dist = c.match_hamming(dL, dR)
    ridx, rdist = oracle.match_hamming(dL, dR)
    assert np.array_equal(idx, ridx) and np.array_equal(dist, rdist)
    c.close()
    if variant == "night" and name in _natural.NATURAL:
        assert short          # at least one level falls short of its quota: sparse quadtree nodes


def test_night_rejects_more_lk_windows_than_day(pkg, oracle, synth, tc):
    """The same points tracked on the same frames by day and at night: minEig rejects more windows at night (status 0),
    on the oracle's side and, byte for byte, on HIP's."""
    rate = {}
    for variant in ("day", "night"):
        _, frames = _frames(synth, tc, "pink", variant, 2)
        (L0, R0), (L1, _) = frames
        pts = _lk_points(oracle, _frames(synth, tc, "pink", "day", 2)[1][0][0], 4000, 23)
        c = pkg.Context(W, H, device=0, max_keypoints=BIG)
        c.build_pyramid(0, L0)
        c.build_pyramid(1, L1)
        got, st = c.lk_track(0, 1, pts)
        c.close()
        want, wst = oracle.lk_track(L0, L1, pts)
        assert st.tobytes() == wst.tobytes() and got.tobytes() == want.tobytes()
        rate[variant] = 1.0 - wst.mean()
    print(f"LK status-0 rate, same points: day {rate['day']:.3f}, night {rate['night']:.3f}")
    assert rate["night"] > rate["day"]


# ---- whole steps -----------------------------------------------------------------------------------------------------
def _lk_exact(pkg, oracle, tc, seq, frames, min_ok):
    ref = _oracle_lk_sequence(oracle, seq, frames)
    assert sum(r["ok"] for r, _, _, _ in ref) >= min_ok
    res, _ = _check_batch(pkg, tc, seq, frames, ref, max_keypoints=BIG)
    _check_online(pkg, seq, frames, ref, max_keypoints=BIG)
    return ref, res


def _lk_float(pkg, oracle, tc, seq, frames, oname, exact_ref):
    _, svo_mode, o_mode = next(o for o in ORDERS if o[0] == oname)
    with accum_oracle(oracle, o_mode):
        ref = _oracle_lk_sequence(oracle, seq, frames)
    _check_batch(pkg, tc, seq, frames, ref, max_keypoints=BIG, lk_accum=svo_mode)
    _check_online(pkg, seq, frames, ref, max_keypoints=BIG, lk_accum=svo_mode)
    return any(a[0]["tracks"].tobytes() != b[0]["tracks"].tobytes() for a, b in zip(ref, exact_ref))


def _orb(pkg, oracle, tc, seq, frames, min_ok):
    """_check_orb_sequence, and the RANSAC counts of the pairs (iterationsCount 500: below it the adaptive stop fired)."""
    _check_orb_sequence(pkg, oracle, tc, seq, frames, min_ok=min_ok, min_tracked=20)
    P1, P2 = seq.proj()
    c = pkg.Context(W, H, device=0, P1=P1, P2=P2, track_mode=pkg.MODE_ORB, min_move2=0.05 ** 2, max_move2=10.0 ** 2,
                    max_batch=len(frames) - 1)
    L = tc.stack([tc.from_numpy(f[0]) for f in frames]).cuda()
    R = tc.stack([tc.from_numpy(f[1]) for f in frames]).cuda()
    res = c.track_batch(L, R)
    c.close()
    return res


def _gt_errors(seq, res):
    """Per ok pair: (angle between estimated and true translation in degrees, |norm error| / true norm, rotation error
    in degrees), against the renderer's ground truth (tools/trajectory_check.py's comparison)."""
    out = []
    for p in range(len(res)):
        if not res["ok"][p]:
            continue
        Tg = seq.relative_gt(p + 1).numpy()
        t, tg = res["tvec"][p], Tg[:3, 3]
        ang = np.degrees(np.arccos(np.clip(t @ tg / (np.linalg.norm(t) * np.linalg.norm(tg)), -1.0, 1.0)))
        dR = res["R"][p].reshape(3, 3) @ Tg[:3, :3].T
        rot = np.degrees(np.arccos(np.clip((np.trace(dR) - 1.0) / 2.0, -1.0, 1.0)))
        out.append((ang, abs(np.linalg.norm(t) - np.linalg.norm(tg)) / np.linalg.norm(tg), rot))
    return np.array(out)


# bounds against ground truth: GT_BOUNDS[mode] = (translation direction deg, relative norm error, rotation deg)
GT_BOUNDS = {"lk": (1.3, 0.021, 0.035), "orb": (3.8, 0.045, 0.25)}


def test_china_day_whole_steps_and_ground_truth(pkg, oracle, synth, tc):
    """24 pairs, LK exact and ORB, batched and online; then each ok pair's relative motion against the renderer's ground
    truth, which is independent of both sides (a misreading shared by HIP and the oracle would pass parity, not this).
    Calibrated with tools/trajectory_check.py's comparison on the first 24 pairs (max over ok pairs; S0 = the default
    rendering of seeds 20200710 and 7):
      LK : S0 direction 0.64 deg, norm 1.04 %, rotation 0.017 deg;  china day 0.39 deg, 0.36 %, 0.017 deg
      ORB: S0 direction 1.90 deg, norm 1.75 %, rotation 0.120 deg;  china day 1.77 deg, 2.20 %, 0.098 deg
    Each bound in GT_BOUNDS is 2x the larger of the two (rounded up).  On the MI355X (frames rendered there) the HIP
    path measured LK 0.35 deg, 0.51 %, 0.018 deg and ORB 1.89 deg, 1.67 %, 0.161 deg.  No ORB pair stopped RANSAC
    early (ransac_iters 500 throughout: inlier ratios 12-33 %), so test_gpu_parity_pose.py's early-stop bands carry
    that case."""
    seq, frames = _frames(synth, tc, "china", "day", 25)
    _, lk = _lk_exact(pkg, oracle, tc, seq, frames, min_ok=23)
    orb = _orb(pkg, oracle, tc, seq, frames, min_ok=20)
    print(f"china day ORB ransac_iters: {sorted(int(i) for i in orb['ransac_iters'])}")
    for mode, res in (("lk", lk), ("orb", orb)):
        e = _gt_errors(seq, res)
        assert len(e) >= 20, mode
        print(f"china day {mode} vs ground truth: direction {e[:, 0].max():.4f} deg, norm {e[:, 1].max():.5f}, "
              f"rotation {e[:, 2].max():.5f} deg")
        for k in range(3):
            assert e[:, k].max() <= GT_BOUNDS[mode][k], (mode, k, e[:, k].max())


def test_grace_hopper_overexposed_whole_steps(pkg, oracle, synth, tc):
    seq, frames = _frames(synth, tc, "grace_hopper", "overexposed", 13)
    _lk_exact(pkg, oracle, tc, seq, frames, min_ok=11)
    orb = _orb(pkg, oracle, tc, seq, frames, min_ok=10)
    print(f"grace_hopper overexposed ORB ransac_iters: {sorted(int(i) for i in orb['ransac_iters'])}")


def test_night_whole_steps_and_sse2_legacy(pkg, oracle, synth, tc):
    """Pairs may fail at night; their fail stages must equal the oracle's (asserted by the record checks)."""
    seq, frames = _frames(synth, tc, "china", "night", 13)
    ref, _ = _lk_exact(pkg, oracle, tc, seq, frames, min_ok=0)
    print(f"night fail stages: {[r['fail_stage'] for r, _, _, _ in ref]}, tracked {[r['n_tracked'] for r, _, _, _ in ref]}")
    assert max(r["n_tracked"] for r, _, _, _ in ref) > 0          # LK did run on some pair
    _lk_float(pkg, oracle, tc, seq, frames[:9], "sse2_legacy", ref[:8])


def test_lr_mismatch_whole_steps_and_float_orders(pkg, oracle, synth, tc):
    seq, frames = _frames(synth, tc, "grace_hopper", "lr_mismatch", 13)
    ref, _ = _lk_exact(pkg, oracle, tc, seq, frames, min_ok=11)
    differs = [_lk_float(pkg, oracle, tc, seq, frames[:9], o, ref[:8]) for o in ("sse2", "simd128")]
    assert any(differs)          # a float order moves tracks against exact on this content (else it proves little)
    orb = _orb(pkg, oracle, tc, seq, frames, min_ok=10)
    print(f"grace_hopper lr_mismatch ORB ransac_iters: {sorted(int(i) for i in orb['ransac_iters'])}")
