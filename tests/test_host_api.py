"""Host-side C++ mirror of the reference's lzb_vio API (stereo-visual-odometry_amd/host/).

CPU: the YAML surface parses the reference's config/default.yaml layout and the PGM/PNG readers
decode what cv::imread(IMREAD_GRAYSCALE) would.  GPU (-m gpu): run_kitti_stereo <yaml> is a drop-in:
it walks a KITTI-layout dataset directory and its pose chain equals the C-ABI's online path."""
import os
import subprocess

import numpy as np
import pytest

import conftest

HOST = os.path.join(conftest.ROOT, "stereo-visual-odometry_amd", "host")

YAML = """%YAML:1.0
# data
dataset_path: {dataset}

# don't care，it doesn't effect others.(this param is diacard)
ros_data_IaE_dir: /
camera_l.fx: {fx}
camera_l.fy: {fy}
camera_l.cx: {cx}
camera_l.cy: {cy}
camera_r.fx: {fx2}
camera_r.fy: {fy2}
camera_r.cx: {cx2}
camera_r.cy: {cy2}
t_lr0: {tlr0}
t_lr1: {tlr1}
t_lr2: {tlr2}
R_lr0: {R0}
R_lr1: {R1}
R_lr2: {R2}
R_lr3: {R3}
R_lr4: {R4}
R_lr5: {R5}
R_lr6: {R6}
R_lr7: {R7}
R_lr8: {R8}
num_features: 500
num_features_init: 20
init_landmarks: 5
feature_match_error: 3
num_features_tracking: 5
num_features_tracking_bad: 10
num_features_needed_for_keyframe: 60
#you can choose LK_stereof2f_pnp, ORB_stereof2f_pnp
track_mode: {mode}
inlier_rate: 0.01
iterationsCount: 500
reprojectionError: 0.5
confidence: 0.99
display_scale: 1
display_x: 400
display_y: 200
minmove: 0.05
maxmove: 10
fMinThFAST: 7
fIniThFAST: 20
nLevels: 8
fScaleFactor: 1.2
nFeatures: 2000
"""


@pytest.fixture(scope="module")
def host_built(pkg):
    pkg.build_library()
    subprocess.check_call(["make", "-C", HOST], stdout=subprocess.DEVNULL)
    return HOST


_R_IDENTITY = ("1.0", "0.0", "0.0", "0.0", "1.0", "0.0", "0.0", "0.0", "1.0")


def _write_yaml(path, dataset, fx=718.856, fy=718.856, cx=607.193, cy=185.216, mode="LK_stereof2f_pnp", baseline=0.537,
                camera_r=None, t_lr=None, R_lr=None):
    """The reference's config layout.  camera_r = (fx, fy, cx, cy) of the right camera (default: the left one's),
    t_lr = its three t_lr* (default (-baseline, 0, 0)), R_lr = the nine R_lr*, row-major (default I); given values are
    written with repr(), so that the loader reads back the same doubles."""
    fx2, fy2, cx2, cy2 = (fx, fy, cx, cy) if camera_r is None else tuple(repr(float(v)) for v in camera_r)
    tl = (repr(-float(baseline)), "0.00", "0.00") if t_lr is None else tuple(repr(float(v)) for v in t_lr)
    Rl = _R_IDENTITY if R_lr is None else tuple(repr(float(v)) for v in np.asarray(R_lr, np.float64).reshape(9))
    with open(path, "w", encoding="utf-8") as f:
        f.write(YAML.format(dataset=dataset, fx=fx, fy=fy, cx=cx, cy=cy, mode=mode, fx2=fx2, fy2=fy2, cx2=cx2, cy2=cy2,
                            tlr0=tl[0], tlr1=tl[1], tlr2=tl[2], **{f"R{i}": Rl[i] for i in range(9)}))


def _write_pgm(path, img):
    with open(path, "wb") as f:
        f.write(b"P5\n# synthetic\n%d %d\n255\n" % (img.shape[1], img.shape[0]))
        f.write(np.ascontiguousarray(img).tobytes())


def _hash(img):
    s = 0
    for v in img.reshape(-1).tolist():
        s = (s * 31 + v) % (1 << 64)
    return s


def test_yaml_surface_and_image_readers(host_built, tmp_path):
    from PIL import Image
    rng = np.random.default_rng(3)
    gray = rng.integers(0, 256, (37, 53), dtype=np.uint8)
    rgb = rng.integers(0, 256, (21, 34, 3), dtype=np.uint8)
    Image.fromarray(gray).save(tmp_path / "g.png")
    Image.fromarray(rgb).save(tmp_path / "c.png")
    _write_pgm(tmp_path / "g.pgm", gray)
    (tmp_path / "bad.png").write_bytes(b"not a png at all")
    _write_yaml(tmp_path / "cfg.yaml", "/data/kitti/00", mode="ORB_stereof2f_pnp")
    out = subprocess.check_output([os.path.join(host_built, "host_selftest"), str(tmp_path / "cfg.yaml"),
                                   str(tmp_path / "g.png"), str(tmp_path / "g.pgm"), str(tmp_path / "c.png"),
                                   str(tmp_path / "bad.png")], stderr=subprocess.DEVNULL).decode()
    lines = dict(l.split("=", 1) if l.count("=") == 1 else (l.split(" ", 1)[0], l) for l in out.strip().split("\n"))
    assert lines["track_mode"] == "ORB_stereof2f_pnp" and lines["dataset_path"] == "/data/kitti/00"
    assert "fx=718.856000 cx=607.193000 cy=185.216000" in out
    assert "P2_03=%.9f" % (718.856 * -0.537) in out
    assert "feature_match_error=3.000 num_features_tracking=5 inlier_rate=0.0100" in out
    assert "iterationsCount=500 reprojectionError=0.500 confidence=0.990" in out
    assert "nFeatures=2000 fScaleFactor=1.20 nLevels=8 fIniThFAST=20 fMinThFAST=7" in out
    assert lines["missing"] == "0"
    assert f"image1 ok=1 rows=37 cols=53 hash={_hash(gray)}" in out
    assert f"image2 ok=1 rows=37 cols=53 hash={_hash(gray)}" in out
    g = ((rgb[..., 0].astype(np.int64) * 4899 + rgb[..., 1].astype(np.int64) * 9617 +
          rgb[..., 2].astype(np.int64) * 1868 + 8192) >> 14).astype(np.uint8)
    assert f"image3 ok=1 rows=21 cols=34 hash={_hash(g)}" in out
    assert "image4 ok=0" in out


def _selftest_P(out):
    """The 12 entries of projMatr1_ and projMatr2_ as host_selftest prints them (%.17g: the exact doubles)."""
    rows = dict(l.split("=", 1) for l in out.splitlines() if l.startswith(("P1=", "P2=")))
    return [np.array([float(v) for v in rows[k].split()]).reshape(3, 4) for k in ("P1", "P2")]


def test_general_rig_projection_matrices(host_built, tmp_path):
    """lzb_vio::Parameter on a rig with distinct camera_r.*, a non-symmetric R_lr0..8 and all three t_lr*: projMatr1_ =
    K1 [I|0] and projMatr2_ = K2 [R_rl | t_rl] (reference src/parameter.cpp, R_lr* row-major) against numpy.  Entries
    that are a single product (or a copy) must be exact, sums of two products within 1 ulp (the summation order)."""
    import _rigs
    fx, fy, cx, cy = 718.856, 0.85 * 718.856, 631.5, 171.25                       # R1's left camera
    cam_r = (_rigs.RIGS["R2"][k] for k in ("fx2", "fy2", "cx2", "cy2"))            # R2's right camera
    cam_r = tuple(cam_r)
    R, t = np.asarray(_rigs.RIGS["R3"]["R_rl"]), np.asarray(_rigs.R3_T)            # R3's rotation and translation
    assert not np.allclose(R, R.T) and np.all(t != 0)
    _write_yaml(tmp_path / "cfg.yaml", "/data/kitti/00", fx=repr(fx), fy=repr(fy), cx=repr(cx), cy=repr(cy),
                camera_r=cam_r, t_lr=t, R_lr=R)
    out = subprocess.check_output([os.path.join(host_built, "host_selftest"), str(tmp_path / "cfg.yaml")],
                                  stderr=subprocess.DEVNULL).decode()
    P1, P2 = _selftest_P(out)
    K1 = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]])
    K2 = np.array([[cam_r[0], 0, cam_r[2]], [0, cam_r[1], cam_r[3]], [0, 0, 1.0]])
    assert np.array_equal(P1, np.hstack([K1, np.zeros((3, 1))]))
    want = K2 @ np.hstack([R, t[:, None]])
    assert np.array_equal(P2[2], want[2])                                          # 1 * R[2, c], 1 * t[2]
    assert np.all(np.abs(P2 - want) <= np.spacing(np.abs(want))), P2 - want
    assert "P2_03=%.9f" % want[0, 3] in out
    # the default rig: P2 = K1 [I | (-0.537, 0, 0)] exactly, and the historical P2_03 line
    _write_yaml(tmp_path / "kitti.yaml", "/data/kitti/00")
    out = subprocess.check_output([os.path.join(host_built, "host_selftest"), str(tmp_path / "kitti.yaml")],
                                  stderr=subprocess.DEVNULL).decode()
    P1, P2 = _selftest_P(out)
    K = np.array([[718.856, 0, 607.193], [0, 718.856, 185.216], [0, 0, 1.0]])
    assert np.array_equal(P1, np.hstack([K, np.zeros((3, 1))]))
    assert np.array_equal(P2, np.hstack([K, [[718.856 * -0.537], [0], [0]]]))
    assert "P2_03=%.9f" % (718.856 * -0.537) in out


def test_png_reader_stream_shapes(host_built, tmp_path):
    """The PNG reader on the stream shapes deflate has: stored blocks (level 0), fixed and dynamic Huffman blocks, long
    matches (flat image), literals only (noise), every row filter (PIL picks them per row for the gradient / photo-like
    images), one and many IDAT chunks, widths that are not multiples of anything: same pixels as PIL."""
    from PIL import Image
    rng = np.random.default_rng(8)
    yy, xx = np.mgrid[0:173, 0:419]
    imgs = {
        "noise": rng.integers(0, 256, (173, 419), dtype=np.uint8),
        "flat": np.full((64, 1241), 93, np.uint8),
        "grad": ((xx * 3 + yy * 5) % 256).astype(np.uint8),
        "photo": np.clip(128 + 60 * np.sin(xx / 17.0) * np.cos(yy / 11.0) + rng.normal(0, 4, xx.shape), 0, 255).astype(np.uint8),
        "tiny": rng.integers(0, 256, (1, 1), dtype=np.uint8),
        "thin": rng.integers(0, 4, (300, 3), dtype=np.uint8) * 60,
    }
    files, want = [], []
    for name, im in imgs.items():
        for lvl in (0, 1, 6, 9):
            fn = tmp_path / f"{name}_{lvl}.png"
            Image.fromarray(im).save(fn, compress_level=lvl)
            files.append(str(fn)); want.append(im)
    big = np.clip(120 + 50 * np.sin(np.arange(376)[:, None] / 23.0) + rng.normal(0, 6, (376, 1241)), 0, 255).astype(np.uint8)
    Image.fromarray(big).save(tmp_path / "big.png", compress_level=3)           # several 64 KB IDAT chunks
    files.append(str(tmp_path / "big.png")); want.append(big)
    _write_yaml(tmp_path / "cfg.yaml", "/data/kitti/00")
    # the one-shot decoder (fast_inflate.h + four Paeth rows in flight) and the zlib path behind it: the same pixels
    for env in ({}, {"LZB_VIO_PNG_ZLIB": "1"}):
        out = subprocess.check_output([os.path.join(host_built, "host_selftest"), str(tmp_path / "cfg.yaml")] + files,
                                      stderr=subprocess.DEVNULL, env=dict(os.environ, **env)).decode()
        for i, im in enumerate(want):
            assert f"image{i + 1} ok=1 rows={im.shape[0]} cols={im.shape[1]} hash={_hash(im)}" in out, (files[i], env)


def test_fast_inflate_fuzz(tmp_path):
    """host/src/fast_inflate.h (the PNG reader's one-shot inflate, written from RFC 1950 / 1951) against zlib under ASan + UBSan:
    600 random streams of every level / strategy / window size round-trip exactly; bit flips, truncation and wrong sizes are
    never accepted with wrong bytes (the reader falls back to zlib on a refusal)."""
    host = os.path.join(conftest.ROOT, "stereo-visual-odometry_amd", "host")
    exe = tmp_path / "fuzz"
    subprocess.check_call(["g++", "-O2", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(host, "src"),
                           os.path.join(host, "tests_host", "fast_inflate_fuzz.cpp"), "-lz", "-o", str(exe)])
    r = subprocess.run([str(exe), "600"], capture_output=True, timeout=600)
    out = r.stdout.decode()
    assert r.returncode == 0, out[-2000:] + r.stderr.decode()[-2000:]
    assert "round trips ok 600 / 600" in out and "MISMATCH" not in out and "ACCEPTED" not in out, out[-2000:]


def _png_bytes(img, payload_edit=None, rows_in_stream=None):
    """A gray 8-bit PNG built by hand (filter 0, stored deflate blocks so that image bytes sit in the stream as they are),
    every chunk CRC correct; payload_edit(bytearray of the zlib stream) may damage it, rows_in_stream lies about the height."""
    import struct
    import zlib
    h, w = img.shape
    rows = img if rows_in_stream is None else np.vstack([img] * 2)[:rows_in_stream]
    raw = b"".join(b"\x00" + rows[y].tobytes() for y in range(rows.shape[0]))
    z = bytearray(zlib.compress(raw, 0))
    if payload_edit:
        payload_edit(z)

    def chunk(t, d):
        return struct.pack(">I", len(d)) + t + d + struct.pack(">I", zlib.crc32(t + d) & 0xFFFFFFFF)
    return b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 0, 0, 0, 0)) + chunk(b"IDAT", bytes(z)) + chunk(b"IEND", b"")


def test_png_reader_checks_the_stream_end(host_built, tmp_path):
    """A PNG whose deflate syntax is intact but whose bytes are not what was compressed (Adler-32 mismatch), one that
    carries more rows than its header says, and one cut short: all refused; the untouched file decodes."""
    rng = np.random.default_rng(12)
    img = rng.integers(0, 256, (40, 57), dtype=np.uint8)

    def flip(z):
        z[len(z) // 2] ^= 0x10               # a literal byte inside a stored block: still valid deflate, wrong checksum

    (tmp_path / "good.png").write_bytes(_png_bytes(img))
    (tmp_path / "flipped.png").write_bytes(_png_bytes(img, payload_edit=flip))
    (tmp_path / "extra_rows.png").write_bytes(_png_bytes(img, rows_in_stream=43))
    (tmp_path / "short.png").write_bytes(_png_bytes(img, rows_in_stream=31))
    _write_yaml(tmp_path / "cfg.yaml", "/data/kitti/00")
    out = subprocess.check_output([os.path.join(host_built, "host_selftest"), str(tmp_path / "cfg.yaml")] +
                                  [str(tmp_path / f) for f in ("good.png", "flipped.png", "extra_rows.png", "short.png")],
                                  stderr=subprocess.DEVNULL).decode()
    assert f"image1 ok=1 rows=40 cols=57 hash={_hash(img)}" in out
    assert "image2 ok=0" in out and "image3 ok=0" in out and "image4 ok=0" in out


@pytest.mark.parametrize("n,n_features,w,h,seed", [(3000, 500, 1209, 344, 1), (700, 2000, 600, 300, 2), (5000, 60, 200, 190, 3),
                                                    (40, 100, 90, 400, 4), (1, 10, 300, 100, 5)])
def test_distribute_octtree_host_matches_oracle(host_built, oracle, tmp_path, n, n_features, w, h, seed):
    """lzb_vio::ORBextractor::DistributeOctTree (protected in the reference, include/lzb_vio/ORBextractor.h:79-80; host
    code, no GPU) through a subclass, against the oracle's restatement of src/ORBextractor.cpp:487-715: dense sets that
    reach the "largest node first" phase, integer responses with many ties, a set smaller than N, a tall region
    (nIni = 0 -> nothing), a single key."""
    rng = np.random.default_rng(seed)
    xyr = np.stack([rng.integers(0, w, n), rng.integers(0, h, n), rng.integers(7, 60, n)], 1).astype(np.float32)
    with open(tmp_path / "k.txt", "w") as f:
        for x, y, r in xyr:
            f.write(f"{x:.1f} {y:.1f} {r:.1f}\n")
    out = subprocess.check_output([os.path.join(host_built, "host_selftest"), "--quadtree", str(tmp_path / "k.txt"),
                                   "16", str(16 + w), "16", str(16 + h), str(n_features)], stderr=subprocess.DEVNULL).decode().splitlines()
    assert out[0] == "pattern=512 first=8,-3 last=0,-11 umax0=15 umax15=3"          # src/ORBextractor.cpp:101, :356 (second point), umax table
    want = oracle.orb_distribute(xyr, 16, 16 + w, 16, 16 + h, n_features)
    got = [int(v) for v in out[1].split(":")[1].split()]
    assert got == want.tolist() and out[1].startswith(f"selected {len(want)}:")
    if n >= 700:
        assert len(want) >= min(n_features, 50)


def test_usage_error_returns_nonzero(host_built):
    r = subprocess.run([os.path.join(host_built, "run_kitti_stereo")], stderr=subprocess.DEVNULL)
    assert r.returncode == 2


@pytest.mark.gpu
def test_run_kitti_stereo_drop_in(host_built, pkg, small_seq, tmp_path):
    from PIL import Image
    seq, frames = small_seq
    h, w = frames[0][0].shape
    for cam in (0, 1):
        os.makedirs(tmp_path / f"image_{cam}")
    for t, (L, R) in enumerate(frames):
        Image.fromarray(L).save(tmp_path / "image_0" / f"{t:06d}.png")
        if t % 2:
            _write_pgm(tmp_path / "image_1" / f"{t:06d}.pgm", R)          # reader falls back to .pgm
        else:
            Image.fromarray(R).save(tmp_path / "image_1" / f"{t:06d}.png")
    _write_yaml(tmp_path / "cfg.yaml", str(tmp_path), fx=seq.fx, fy=seq.fy, cx=seq.cx, cy=seq.cy)
    r = subprocess.run([os.path.join(host_built, "run_kitti_stereo"), str(tmp_path / "cfg.yaml"),
                        str(tmp_path / "poses.txt")], capture_output=True)
    assert r.returncode == 0, r.stderr.decode()
    poses = np.loadtxt(tmp_path / "poses.txt").reshape(-1, 3, 4)
    assert poses.shape[0] == len(frames)
    # the same frames through the C-ABI's online path
    P1, P2 = seq.proj()
    c = pkg.Context(w, h, device=0, P1=P1, P2=P2)
    ref = []
    for L, R in frames:
        c.add_frame(L, R)
        ref.append(c.get_pose()[:3])
    c.close()
    assert np.allclose(poses[0], np.eye(4)[:3])
    assert np.abs(poses - np.array(ref)).max() < 1e-6
    gt = np.linalg.inv(seq.poses_wc()[0].numpy()) @ seq.poses_wc()[len(frames) - 1].numpy()
    assert np.abs(poses[-1][:, 3] - gt[:3, 3]).max() < 0.25
    # batched runner (additive YAML keys): chunks of 2 pairs with a one-frame halo, threaded decode
    for bs in (2, 8):
        with open(tmp_path / "cfg.yaml", encoding="utf-8") as f:
            txt = f.read()
        with open(tmp_path / f"batch{bs}.yaml", "w", encoding="utf-8") as f:
            f.write(txt + f"batch_size: {bs}\ndecode_threads: 3\n")
        r = subprocess.run([os.path.join(host_built, "run_kitti_stereo"), str(tmp_path / f"batch{bs}.yaml"),
                            str(tmp_path / f"poses_b{bs}.txt")], capture_output=True)
        assert r.returncode == 0, r.stderr.decode()
        poses_b = np.loadtxt(tmp_path / f"poses_b{bs}.txt").reshape(-1, 3, 4)
        assert poses_b.shape == poses.shape and np.abs(poses_b - poses).max() < 1e-7
    # the shipped default track_mode (ORB_stereof2f_pnp) through the same binary
    _write_yaml(tmp_path / "orb.yaml", str(tmp_path), fx=seq.fx, fy=seq.fy, cx=seq.cx, cy=seq.cy, mode="ORB_stereof2f_pnp")
    r = subprocess.run([os.path.join(host_built, "run_kitti_stereo"), str(tmp_path / "orb.yaml"),
                        str(tmp_path / "poses_orb.txt")], capture_output=True)
    assert r.returncode == 0, r.stderr.decode()
    poses_orb = np.loadtxt(tmp_path / "poses_orb.txt").reshape(-1, 3, 4)
    c = pkg.Context(w, h, device=0, P1=P1, P2=P2, track_mode=pkg.MODE_ORB, min_move2=0.05 ** 2, max_move2=10.0 ** 2)
    ref = []
    for L, R in frames:
        c.add_frame(L, R)
        ref.append(c.get_pose()[:3])
    c.close()
    assert np.abs(poses_orb - np.array(ref)).max() < 1e-6


@pytest.mark.gpu
def test_frame_carriers_and_track_dump(host_built, pkg, oracle, small_seq, tmp_path):
    """The reference's per-frame carriers (Frame::features_left_/right_, *_Descriptors_) filled from
    the GPU state, and the headless displayTracking replacement (tracks_file), in both modes."""
    seq, frames = small_seq
    h, w = frames[0][0].shape
    for cam in (0, 1):
        os.makedirs(tmp_path / f"image_{cam}")
    for t, (L, R) in enumerate(frames):
        _write_pgm(tmp_path / "image_0" / f"{t:06d}.pgm", L)
        _write_pgm(tmp_path / "image_1" / f"{t:06d}.pgm", R)
    P1, P2 = seq.proj()
    for mode in ("LK_stereof2f_pnp", "ORB_stereof2f_pnp"):
        _write_yaml(tmp_path / "c.yaml", str(tmp_path), fx=seq.fx, fy=seq.fy, cx=seq.cx, cy=seq.cy, mode=mode)
        with open(tmp_path / "c.yaml", "a", encoding="utf-8") as f:
            f.write(f"tracks_file: {tmp_path}/tracks_{mode}.txt\n")
        out = subprocess.run([os.path.join(host_built, "host_selftest"), "--track", str(tmp_path / "c.yaml"), str(len(frames))],
                             capture_output=True)
        assert out.returncode == 0, out.stderr.decode()
        rows = [dict(kv.split("=") for kv in line.split()) for line in out.stdout.decode().splitlines() if line.startswith("frame=")]
        assert len(rows) == len(frames)
        # the C-ABI read-back through the Python binding on the same frames
        kw = dict(P1=P1, P2=P2)
        if mode.startswith("ORB"):
            kw.update(track_mode=pkg.MODE_ORB, min_move2=0.05 ** 2, max_move2=10.0 ** 2)
        c = pkg.Context(w, h, device=0, **kw)
        for t, (L, R) in enumerate(frames):
            rc, rec = c.add_frame(L, R)
            r = rows[t]
            if mode.startswith("ORB"):
                kl, dl = c.frame_keypoints(0, with_descriptors=True)
                kr, dr = c.frame_keypoints(1, with_descriptors=True)
                okl, odl, _ = oracle.orb_extract(L)
                okr, odr, _ = oracle.orb_extract(R)
                assert kl.tobytes() == okl.tobytes() and dl.tobytes() == odl.tobytes()
                assert kr.tobytes() == okr.tobytes() and dr.tobytes() == odr.tobytes()
                assert int(r["featuresL"]) == len(kl) == int(r["descL"]) and int(r["featuresR"]) == len(kr) == int(r["descR"])
            else:
                kl = c.frame_keypoints(0)
                assert kl.tobytes() == oracle.fast(L).tobytes()
                assert int(r["featuresL"]) == len(kl) and int(r["featuresR"]) == 0
            s = float((kl["x"].astype(np.float64) + 2.0 * kl["y"] + kl["response"]).sum())
            assert abs(float(r["sumL"]) - s) < 1e-2
            tr = c.last_tracks()
            if t == 0:
                assert len(tr[0]) == 0 and int(r["tracks"]) == 0
            else:
                assert len(tr[0]) == int(rec["n_tracked"]) == int(r["tracks"]) == int(r["n_tracked"])
                assert int(tr[4].sum()) == int(rec["n_inliers"]) == int(r["inliers"]) == int(r["n_inliers"])
                if not mode.startswith("ORB"):
                    ref = c.circular_match  # the same tracks as the stage API on the ring slots is covered elsewhere
                    assert np.all(tr[0][:, 0] >= 0) and tr[1].shape == tr[0].shape == tr[3].shape
        c.close()
        # the track dump written by System::Step_ros
        lines = open(tmp_path / f"tracks_{mode}.txt").read().splitlines()
        F = [ln.split() for ln in lines if ln.startswith("F ")]
        T = [ln for ln in lines if ln.startswith("T ")]
        assert len(F) == len(frames) and sum(int(f[5]) for f in F[1:]) == len(T)
        assert sum(int(ln.split()[-1]) for ln in T) == sum(int(f[6]) for f in F[1:])


@pytest.mark.gpu
def test_orbextractor_class_matches_oracle(host_built, oracle, small_seq, tmp_path):
    """lzb_vio::ORBextractor (reference include/lzb_vio/ORBextractor.h:33-75): constructor tables,
    operator() on the left then the right image (src/tracking.cpp:508-509), getters, and the public
    mvImagePyramid, which afterwards holds the RIGHT image's pyramid --
    all compared byte for byte with the oracle through hashes printed by host_selftest --orb."""
    seq, frames = small_seq
    L, R = frames[0]
    h, w = L.shape
    _write_pgm(tmp_path / "l.pgm", L)
    _write_pgm(tmp_path / "r.pgm", R)
    _write_yaml(tmp_path / "c.yaml", str(tmp_path), mode="ORB_stereof2f_pnp")
    out = subprocess.run([os.path.join(host_built, "host_selftest"), "--orb", str(tmp_path / "c.yaml"), str(tmp_path / "l.pgm"),
                          str(tmp_path / "r.pgm")], capture_output=True)
    assert out.returncode == 0, out.stderr.decode()
    lines = out.stdout.decode().splitlines()

    def bhash(b):
        hh = 0
        for v in bytes(b):
            hh = (hh * 31 + v) & 0xFFFFFFFFFFFFFFFF
        return hh

    sc, inv, quota, umax = oracle.orb_setup(2000, 1.2, 8)
    head = lines[0].split()
    assert head[0] == "levels=8" and head[1] == "scale=1.200000"
    got_sc = np.array([float(v) for v in head[2:10]], np.float32)
    got_isig = np.array([float(v) for v in head[10:18]], np.float32)
    assert np.array_equal(got_sc, sc) and np.array_equal(got_isig, (np.float32(1) / (sc * sc)).astype(np.float32))
    assert [int(v) for v in head[19:27]] == quota.tolist()
    for i, img in ((1, L), (2, R)):
        kp, desc, _ = oracle.orb_extract(img)
        kv = dict(x.split("=") for x in lines[i].split()[1:])
        assert int(kv["n"]) == len(kp) == int(kv["rows"]) and int(kv["cols"]) == 32 and len(kp) > 50
        assert int(kv["kp_hash"]) == bhash(kp.tobytes()) and int(kv["desc_hash"]) == bhash(desc.tobytes())
    for l in range(8):
        lvl = oracle.orb_pyramid_level(R, l)                    # the RIGHT image's pyramid
        kv = dict(x.split("=") for x in lines[3 + l].split()[1:])
        assert (int(kv["rows"]), int(kv["cols"])) == lvl.shape and int(kv["hash"]) == bhash(lvl.tobytes())
    # the protected stages through a subclass (ComputePyramid + ComputeKeyPointsOctTree / ...Old on the LEFT image):
    # per-level counts of the oracle, level coordinates integral, scaled back == operator()'s keypoints bit for bit
    kpL, _, per = oracle.orb_extract(L)
    oct_ = lines[11].split()
    assert oct_[0] == "octree" and oct_[1] == "levels=8" and [int(v) for v in oct_[3:11]] == per.tolist()
    assert oct_[11] == f"total={len(kpL)}" and oct_[13] == str(len(kpL)) and oct_[14] == "same=1" and oct_[15] == f"pyramid0={w}x{h}"
    assert lines[12] == "empty n=0 rows=0"


def test_image_readers_survive_corrupted_files(host_built, tmp_path):
    """PNG / PGM readers (System::NextFrame_kitti replaces cv::imread with them) on truncated,
    bit-flipped and length-corrupted files, built with AddressSanitizer + UBSan: they may refuse a
    file, they must not crash, read out of bounds or overflow."""
    import random
    import struct
    from PIL import Image
    exe = str(tmp_path / "host_selftest_asan")
    srcs = [os.path.join(HOST, "tests_host", "host_selftest.cpp")] + \
           [os.path.join(HOST, "src", f) for f in sorted(os.listdir(os.path.join(HOST, "src"))) if f.endswith(".cpp")]
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++14", "-pthread", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                           "-I" + os.path.join(HOST, "include"), "-I" + os.path.join(conftest.ROOT, "include"), "-o", exe] + srcs +
                          ["-L" + os.path.dirname(HOST), "-lsvo_hip", "-lz", "-Wl,-rpath," + os.path.dirname(HOST)])
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, (40, 57), dtype=np.uint8)
    Image.fromarray(img).save(tmp_path / "ok.png")
    Image.fromarray(np.stack([img] * 3, 2)).save(tmp_path / "rgb.png")
    _write_pgm(tmp_path / "ok.pgm", img)
    random.seed(3)
    files = []
    for name in ("ok.png", "rgb.png", "ok.pgm"):
        data = open(tmp_path / name, "rb").read()
        for i in range(40):
            b = bytearray(data)
            if i % 4 == 0:
                b = b[:random.randrange(1, len(b))]
            elif i % 4 == 1:
                for _ in range(random.randrange(1, 6)):
                    b[random.randrange(len(b))] = random.randrange(256)
            elif i % 4 == 2:
                b = b + bytes(random.randrange(256) for _ in range(50))
            else:
                p = random.randrange(len(b))
                b[p:p + 4] = struct.pack(">I", random.choice([0, 0xFFFFFFFF, 0x7FFFFFFF, 65536]))
            fn = str(tmp_path / f"{name}.{i}.bin")
            open(fn, "wb").write(bytes(b))
            files.append(fn)
        if name.endswith(".png"):
            # deterministic: IHDR width (bytes 16-19) and height (20-23) overwritten with hostile values --
            # the reader must refuse them before allocating anything from the header
            for j, (off, val) in enumerate((o, v) for o in (16, 20) for v in (0x7FFFFFFF, 0xFFFFFFFF, 0x80000000, 65536, 16385, 0)):
                b = bytearray(data)
                b[off:off + 4] = struct.pack(">I", val)
                fn = str(tmp_path / f"{name}.ihdr{j}.bin")
                open(fn, "wb").write(bytes(b))
                files.append(fn)
    # PGM headers with absurd or overflowing dimensions
    for j, hdr in enumerate((b"P5\n99999999999999999999 4\n255\n", b"P5\n4 2147483647\n255\n", b"P5\n0 0\n255\n", b"P5\n70000 70000\n255\n")):
        fn = str(tmp_path / f"hdr{j}.pgm.bin")
        open(fn, "wb").write(hdr + b"\x00" * 64)
        files.append(fn)
    _write_yaml(tmp_path / "c.yaml", str(tmp_path))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    r = subprocess.run([exe, str(tmp_path / "c.yaml"), str(tmp_path / "ok.png")] + files, capture_output=True, env=env, timeout=300)
    err = r.stderr.decode()
    assert r.returncode == 0 and "AddressSanitizer" not in err and "runtime error" not in err, err[-3000:]
    assert f"image1 ok=1 rows=40 cols=57 hash={_hash(img)}" in r.stdout.decode()


@pytest.mark.gpu
def test_run_kitti_stereo_multi_sequence(host_built, synth, tmp_path):
    """`run_kitti_stereo a.yaml b.yaml c.yaml` (lzb_vio::RunSequences): three short sequences of
    different lengths, modes and runners dealt to the node's devices (one GPU here: two worker threads, two
    contexts on the card) -- every pose file equals the single-sequence run's byte for byte."""
    specs = [("s0", 9, 21, "LK_stereof2f_pnp", "batch_size: 4\n"), ("s1", 6, 22, "ORB_stereof2f_pnp", ""),
             ("s2", 13, 23, "LK_stereof2f_pnp", "batch_size: 5\ndecode_threads: 2\n")]
    yamls = []
    for name, n, seed, mode, extra in specs:
        seq = synth.StereoSequence(width=416, height=128, n_frames=n, seed=seed)
        d = tmp_path / name
        for cam in (0, 1):
            os.makedirs(d / f"image_{cam}")
        for t in range(n):
            L, R = (x.numpy() for x in seq.render(t))
            _write_pgm(d / "image_0" / f"{t:06d}.pgm", L)
            _write_pgm(d / "image_1" / f"{t:06d}.pgm", R)
        y = tmp_path / f"{name}.yaml"
        _write_yaml(y, str(d), fx=seq.fx, fy=seq.fy, cx=seq.cx, cy=seq.cy, mode=mode)
        with open(y, "a", encoding="utf-8") as f:
            f.write(extra)
        yamls.append(str(y))
    exe = os.path.join(host_built, "run_kitti_stereo")
    single = []
    for y in yamls:
        r = subprocess.run([exe, y, y + ".single.txt"], capture_output=True, timeout=300)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        single.append(open(y + ".single.txt", "rb").read())
    os.makedirs(tmp_path / "out")
    r = subprocess.run([exe] + yamls + ["--poses-dir", str(tmp_path / "out")], capture_output=True, timeout=600)
    err = r.stderr.decode()
    assert r.returncode == 0, err[-2000:]
    assert "worker 0 (device 0)" in err and "worker 1 (device 0)" in err        # one device: two workers share it
    # longest first: s2 (12 pairs) alone on worker 0, s0 (8) and s1 (5) on worker 1
    assert "worker 0 (device 0): sequences [2], 12 pairs" in err and "worker 1 (device 0): sequences [0,1], 13 pairs" in err
    for (name, n, _, _, _), want in zip(specs, single):
        got = open(tmp_path / "out" / f"{name}.yaml.poses.txt", "rb").read()
        assert got == want and len(got.splitlines()) == n
    # a sequence that cannot be read makes the run fail loudly (and the others still finish)
    bad = tmp_path / "bad.yaml"
    _write_yaml(bad, str(tmp_path / "nowhere"))
    r = subprocess.run([exe, yamls[0], str(bad), "--poses-dir", str(tmp_path / "out")], capture_output=True, timeout=300)
    assert r.returncode == 1 and "[FAILED]" in r.stderr.decode()
    assert open(tmp_path / "out" / "s0.yaml.poses.txt", "rb").read() == single[0]
    # a pose file that cannot be opened: that sequence is not run and counts as failed (exit code 1), not silently dropped
    r = subprocess.run([exe, yamls[0], yamls[1], "--poses-dir", str(tmp_path / "no_such_dir")], capture_output=True, timeout=300)
    assert r.returncode == 1 and r.stderr.decode().count("[FAILED]") == 2 and "is not run" in r.stderr.decode()


@pytest.mark.gpu
def test_run_kitti_stereo_split_pairs(host_built, synth, tmp_path):
    """`run_kitti_stereo cfg.yaml poses --split-pairs N` (lzb_vio::RunSplitPairs, SURVEY.md 8e granularity 2 / 8f rank 1):
    ONE sequence cut into N chunks of frame pairs with a one-frame halo, a context per chunk (here all on the one card),
    the relative motions chained once -- the pose file equals the single-context run's byte for byte, in both modes and
    for chunk counts that do and do not divide the pairs; the orderly-teardown exit (the default) and the fast one agree."""
    exe = os.path.join(host_built, "run_kitti_stereo")
    for name, n, seed, mode in (("lk", 14, 31, "LK_stereof2f_pnp"), ("orb", 9, 32, "ORB_stereof2f_pnp")):
        seq = synth.StereoSequence(width=416, height=128, n_frames=n, seed=seed)
        d = tmp_path / name
        for cam in (0, 1):
            os.makedirs(d / f"image_{cam}")
        for t in range(n):
            L, R = (x.numpy() for x in seq.render(t))
            _write_pgm(d / "image_0" / f"{t:06d}.pgm", L)
            _write_pgm(d / "image_1" / f"{t:06d}.pgm", R)
        y = tmp_path / f"{name}.yaml"
        _write_yaml(y, str(d), fx=seq.fx, fy=seq.fy, cx=seq.cx, cy=seq.cy, mode=mode)
        with open(y, "a", encoding="utf-8") as f:
            f.write("batch_size: 4\n")
        r = subprocess.run([exe, str(y), str(y) + ".single.txt"], capture_output=True, timeout=300)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        want = open(str(y) + ".single.txt", "rb").read()
        assert len(want.splitlines()) == n
        r = subprocess.run([exe, str(y), str(y) + ".fast.txt"], capture_output=True, timeout=300, env=dict(os.environ, LZB_VIO_FAST_EXIT="1"))
        assert r.returncode == 0 and open(str(y) + ".fast.txt", "rb").read() == want
        for parts in (2, 3, 5):
            out = str(y) + f".split{parts}.txt"
            r = subprocess.run([exe, str(y), out, "--split-pairs", str(parts)], capture_output=True, timeout=300)
            assert r.returncode == 0, r.stderr.decode()[-2000:]
            assert r.stderr.decode().count("chunk ") == parts
            assert open(out, "rb").read() == want, (name, parts)
    # more chunks than pairs: clamped; a sequence that cannot be read: exit code 1
    r = subprocess.run([exe, str(y), str(y) + ".many.txt", "--split-pairs", "64"], capture_output=True, timeout=300)
    assert r.returncode == 0 and open(str(y) + ".many.txt", "rb").read() == want
    # at most two chunk workers a device run at a time (here: one card), whatever the chunk count
    assert {int(l.split("worker ")[1].split(")")[0]) for l in r.stderr.decode().splitlines() if l.startswith("chunk ")} <= {0, 1}
    # the pose file named by the YAML (no path on the command line): the split run writes THAT file, the same bytes as the
    # single run; the probe and the chunk Systems neither truncate it nor leave it empty
    y2 = tmp_path / "orb_yaml_out.yaml"
    yaml_out = tmp_path / "yaml_named_poses.txt"
    with open(y2, "w", encoding="utf-8") as f:
        f.write(open(y, encoding="utf-8").read() + f"pose_file: {yaml_out}\n")
    r = subprocess.run([exe, str(y2)], capture_output=True, timeout=300)
    assert r.returncode == 0 and open(yaml_out, "rb").read() == want
    os.remove(yaml_out)
    r = subprocess.run([exe, str(y2), "--split-pairs", "3"], capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert open(yaml_out, "rb").read() == want
    bad = tmp_path / "bad.yaml"
    _write_yaml(bad, str(tmp_path / "nowhere"))
    r = subprocess.run([exe, str(bad), str(tmp_path / "bad.txt"), "--split-pairs", "2"], capture_output=True, timeout=300)
    assert r.returncode == 1
