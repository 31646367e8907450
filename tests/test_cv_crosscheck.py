"""Cross-check of the CPU oracle against a REAL OpenCV, wherever one can be imported ("if a later
environment offers real OpenCV ... add an optional cross-check harness -- probe, never assume").

This image has no cv2 (and no OpenCV headers), so here every test SKIPS with its reason printed; on a box with
`import cv2` they turn the oracle from "parity unpinned" into "pinned against OpenCV <version>": each test compares one
restated callee with the real one on the golden stereo quadruple, at the call-site arguments of the reference --
  cv::FAST(img, kps, 20, true)                                    /root/reference/src/tracking.cpp:101
  cv::calcOpticalFlowPyrLK(.., Size(21,21), 3, (COUNT+EPS,30,0.01), 0, 0.001)   src/tracking.cpp:593-618
  cv::triangulatePoints + convertPointsFromHomogeneous            src/tracking.cpp:292-294
  cv::solvePnPRansac(.., 500, 0.5, 0.99, inliers, ITERATIVE)      src/tracking.cpp:485
  cv::resize(INTER_LINEAR), cv::GaussianBlur(7x7, 2, 2, REFLECT_101), cv::FAST per cell   src/ORBextractor.cpp:763, 1035, 1074-1081
  cv::BFMatcher(NORM_HAMMING).match                               src/tracking.cpp:539-544
-- and, where the oracle has version forks (oracle/geom.c orc_set_opencv_compat; the LK accumulation orders), says WHICH
fork this OpenCV is and fails when none of them reproduces it."""
import os

import numpy as np
import pytest

cv2 = pytest.importorskip("cv2", reason="no OpenCV in this environment (python3 -c 'import cv2' fails): the oracle stays "
                                        "PARITY UNPINNED here; run this file where cv2 exists")

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "stereo_quad_160x96.npz"))


@pytest.fixture()
def compat(oracle):
    touched = []

    def set_(knob, value):
        touched.append(knob)
        oracle.set_opencv_compat(knob, value)
    yield set_
    for k in touched:
        oracle.set_opencv_compat(k, 0)


def _pts():
    return np.stack([G["fast_kp"]["x"], G["fast_kp"]["y"]], 1).astype(np.float32)


def test_report_the_opencv_build():
    print("cross-checking against OpenCV", cv2.__version__)
    info = cv2.getBuildInformation()
    for key in ("CPU/HW features", "Baseline", "Dispatched"):
        for line in info.splitlines():
            if key in line:
                print(line.strip())


def test_fast_9_16_nonmax(oracle):
    det = cv2.FastFeatureDetector_create(threshold=20, nonmaxSuppression=True, type=cv2.FAST_FEATURE_DETECTOR_TYPE_9_16)
    for name in ("L0", "R0", "L1", "R1"):
        kps = det.detect(G[name], None)
        got = np.array([(k.pt[0], k.pt[1], k.response) for k in kps], np.float32).reshape(-1, 3)
        mine = oracle.fast(G[name])
        want = np.stack([mine["x"], mine["y"], mine["response"]], 1)
        assert got.shape == want.shape and np.array_equal(got, want), name      # positions, order and scores


def test_pyr_down(oracle):
    for name in ("L0", "R1"):
        assert np.array_equal(cv2.pyrDown(G[name]), oracle.pyr_down(G[name])), name


def test_calc_optical_flow_pyr_lk_names_its_accumulation_order(oracle):
    """Status bytes must agree in every order; the coordinates bit for bit in (at least) ONE of the restated orders --
    that order is what `lk_accum` should be set to when bit-identity with THIS OpenCV build is wanted."""
    pts = _pts()
    crit = (cv2.TERM_CRITERIA_COUNT | cv2.TERM_CRITERIA_EPS, 30, 0.01)
    names = {0: "exact int64 (canonical C0)", 1: "float, raster order", 2: "round-4 hybrid (lk_accum: sse2)",
             3: "legacy CV_SSE2 block", 4: "CV_SIMD128 block"}
    report = {}
    for a, b in (("L0", "R0"), ("R0", "R1"), ("L0", "L1")):
        nxt, st, _err = cv2.calcOpticalFlowPyrLK(G[a], G[b], pts.reshape(-1, 1, 2), None, winSize=(21, 21), maxLevel=3,
                                                 criteria=crit, flags=0, minEigThreshold=1e-3)
        nxt, st = nxt.reshape(-1, 2), st.reshape(-1)
        for mode in names:
            old = oracle.set_lk_accum(mode)
            try:
                mine, mst = oracle.lk_track(G[a], G[b], pts)
            finally:
                oracle.set_lk_accum(old)
            ok = mst == st
            same = (mine[st == 1] == nxt[st == 1]).all(axis=1).mean() if (st == 1).any() else 1.0
            report.setdefault(mode, []).append((float(ok.mean()), float(same)))
            assert ok.mean() > 0.99, (a, b, names[mode], "status bytes")          # last-bit sums can flip a borderline point
            assert np.abs(mine[(st == 1) & (mst == 1)] - nxt[(st == 1) & (mst == 1)]).max() < 5e-3, (a, b, names[mode])
    for mode, rows in report.items():
        print(f"  {names[mode]:34s} status equal {min(r[0] for r in rows):.4f}  coordinates bit-identical {min(r[1] for r in rows):.4f}")
    best = max(report, key=lambda m: min(r[1] for r in report[m]))
    print("OpenCV", cv2.__version__, "accumulates like:", names[best])
    assert min(r[1] for r in report[best]) == 1.0 and min(r[0] for r in report[best]) == 1.0, \
        "no restated accumulation order reproduces this OpenCV bit for bit: " + str(report)


def test_triangulate_points_names_its_system(oracle, compat):
    x1, x2 = G["tracks"][0], G["tracks"][1]
    P1, P2 = G["P1"].reshape(3, 4), G["P2"].reshape(3, 4)
    X4 = cv2.triangulatePoints(P1, P2, np.ascontiguousarray(x1.T), np.ascontiguousarray(x2.T))     # 4 x N, float32
    X3 = cv2.convertPointsFromHomogeneous(np.ascontiguousarray(X4.T)).reshape(-1, 3)
    hits = {}
    for v, name in ((0, "4 x 4 system (canonical)"), (1, "6 x 4 system (<= 3.3)")):
        compat(oracle.COMPAT_TRIANGULATE, v)
        mine, mine4 = oracle.triangulate(G["P1"], G["P2"], x1, x2, want4=True)
        # a singular vector's sign is the SVD's business: compare the de-homogenised points
        hits[name] = (float((mine == X3).all(axis=1).mean()), float(np.abs(mine - X3).max() / np.abs(X3).max()))
        print(f"  {name}: bit-identical points {hits[name][0]:.4f}, max relative difference {hits[name][1]:.2e}")
    assert max(h[0] for h in hits.values()) == 1.0, hits


def test_solve_pnp_ransac_names_its_refit(oracle, compat):
    x1, x2 = G["tracks"][0], G["tracks"][1]
    X = oracle.triangulate(G["P1"], G["P2"], x1, x2)
    K = G["P1"].reshape(3, 4)[:, :3].copy()
    rvec, tvec = np.zeros((3, 1)), np.zeros((3, 1))
    ok, rvec, tvec, inl = cv2.solvePnPRansac(X.reshape(-1, 1, 3), G["tracks"][3].reshape(-1, 1, 2), K, None, rvec, tvec, True,
                                             500, 0.5, 0.99, None, cv2.SOLVEPNP_ITERATIVE)
    mask = np.zeros(len(X), np.uint8)
    if inl is not None:
        mask[np.asarray(inl).reshape(-1)] = 1
    report = {}
    for v, name in ((0, "LM from the best hypothesis (canonical)"), (1, "no refit (<= 3.2)"), (2, "LM from the last hypothesis (3.4)"),
                    (3, "LM from the zero guess")):
        compat(oracle.COMPAT_PNP_REFIT, v)
        r = oracle.pnp_ransac(X, G["tracks"][3], K)
        assert r["mask"].tobytes() == mask.tobytes(), "RANSAC inlier set (cv::RNG sequence, EPnP, threshold)"
        report[name] = max(float(np.abs(r["rvec"] - rvec.reshape(3)).max()), float(np.abs(r["tvec"] - tvec.reshape(3)).max()))
        print(f"  {name}: max |pose difference| {report[name]:.3e}")
    assert min(report.values()) < 1e-9, report


def test_solve_pnp_ransac_with_four_points_is_p3p(oracle):
    """npoints == 4: cv::solvePnPRansac switches its minimal solver to P3P (one model from the four points, all of them inliers, the
    LM refit on them) -- reachable with num_features_tracking: 4, /root/reference/src/tracking.cpp:274, 485.  oracle/p3p.c restates
    p3p.cpp + polynom_solver.cpp."""
    x1, x2 = G["tracks"][0], G["tracks"][1]
    X = oracle.triangulate(G["P1"], G["P2"], x1, x2)
    K = G["P1"].reshape(3, 4)[:, :3].copy()
    checked = 0
    for start in range(0, len(X) - 4, max(1, (len(X) - 4) // 12)):
        Xs, xs = X[start:start + 4].copy(), G["tracks"][3][start:start + 4].copy()
        rvec, tvec = np.zeros((3, 1)), np.zeros((3, 1))
        ok, rvec, tvec, inl = cv2.solvePnPRansac(Xs.reshape(-1, 1, 3), xs.reshape(-1, 1, 2), K, None, rvec, tvec, True,
                                                 500, 0.5, 0.99, None, cv2.SOLVEPNP_ITERATIVE)
        r = oracle.pnp_ransac(Xs, xs, K)
        assert bool(ok) == bool(r["ok"]), start
        if ok:
            assert r["n_inliers"] == (0 if inl is None else len(inl))
            assert np.abs(r["rvec"] - rvec.reshape(3)).max() < 1e-8 and np.abs(r["tvec"] - tvec.reshape(3)).max() < 1e-8, start
            checked += 1
    assert checked > 0


def test_orb_callees(oracle):
    img = G["L0"]
    h, w = img.shape
    dw, dh = int(round(w / 1.2)), int(round(h / 1.2))
    assert np.array_equal(cv2.resize(img, (dw, dh), interpolation=cv2.INTER_LINEAR), oracle.resize_linear(img, dw, dh))
    assert np.array_equal(cv2.GaussianBlur(img, (7, 7), 2, 2, borderType=cv2.BORDER_REFLECT_101), oracle.gauss_blur7(img))
    kp, desc, _ = oracle.orb_extract(G["L0"], nlevels=3, nfeatures=300)
    kp2, desc2, _ = oracle.orb_extract(G["R0"], nlevels=3, nfeatures=300)
    m = cv2.BFMatcher(cv2.NORM_HAMMING).match(desc, desc2)
    idx, dist = oracle.match_hamming(desc, desc2)
    assert [x.trainIdx for x in m] == list(idx) and [x.distance for x in m] == list(dist)


def test_epnp_and_ransac_on_an_exactly_planar_set(oracle):
    """The restated EPnP returns NaN on five exactly coplanar points and solvePnPRansac then finds no model on a 257-point
    wall (tests/test_pnp_cases.py).  A real OpenCV has to be no better off: its EPnP is non-finite
    there, or reprojects the five points worse than the 0.5 px inlier threshold, and its RANSAC reports failure or no
    inliers."""
    import _pnp_cases as pc
    X, x, r, t = pc.make("wall", 5, pc.SEED, 0)
    ok, rvec, tvec = cv2.solvePnP(X.astype(np.float64).reshape(-1, 1, 3), x.astype(np.float64).reshape(-1, 1, 2), pc.K, None,
                                  flags=cv2.SOLVEPNP_EPNP)
    if ok and np.isfinite(rvec).all() and np.isfinite(tvec).all():
        proj, _ = cv2.projectPoints(X.astype(np.float64).reshape(-1, 1, 3), rvec, tvec, pc.K, None)
        assert np.linalg.norm(proj.reshape(-1, 2) - x, axis=1).max() > 0.5
    X, x, r, t = pc.make("wall", 257, pc.SEED, 80)
    assert oracle.pnp_ransac(X, x, pc.K)["ok"] == 0
    rvec, tvec = np.zeros((3, 1)), np.zeros((3, 1))
    ok, rvec, tvec, inl = cv2.solvePnPRansac(X.reshape(-1, 1, 3), x.reshape(-1, 1, 2), pc.K, None, rvec, tvec, True,
                                             500, 0.5, 0.99, None, cv2.SOLVEPNP_ITERATIVE)
    assert not ok or inl is None or len(inl) == 0
