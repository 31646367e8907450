"""The host mirror's additive YAML keys keyframe / keyframe_max_gap (svo_set_keyframe; min_tracks is the reference's own
num_features_needed_for_keyframe).  CPU: a bad value or a refused combination makes run_kitti_stereo exit 2 with the key named, good
values are reported as they take effect -- on the host, before a device is opened.  GPU (marked): one run on the short
synthetic sequence writes the poses the binding's chain reports."""
import os
import subprocess

import numpy as np
import pytest

import conftest
from test_host_api import _write_pgm, _write_yaml, host_built   # noqa: F401  (host_built: the fixture that builds host/)
from test_host_buckets import _yaml

KEYFRAME_LOG = "keyframe: 1 (num_features_needed_for_keyframe %d, keyframe_max_gap %d)"
ON = "track_carry: 1\nkeyframe: 1\n"


def _run(host_built, tmp_path, extra, mode="LK_stereof2f_pnp", args=()):
    exe = os.path.join(host_built, "run_kitti_stereo")
    y = _yaml(tmp_path, "c.yaml", extra, dataset=str(tmp_path), mode=mode)
    r = subprocess.run([exe, str(y), str(tmp_path / "poses.txt"), *args], capture_output=True, timeout=120)
    return r.returncode, r.stderr.decode()


@pytest.mark.parametrize("extra,says", [
    ("keyframe: 1\n", "keyframe: 1 without track_carry: 1"),
    ("track_carry: 0\nkeyframe: 1\n", "keyframe: 1 without track_carry: 1"),
    ("track_carry: 1\nkeyframe: 2\n", "keyframe: 2 is neither 0 nor 1"),
    ("track_carry: 1\nkeyframe: -1\n", "keyframe: -1"),
    (ON + "keyframe_max_gap: 1\n", "keyframe_max_gap: 1"),
    (ON + "keyframe_max_gap: -4\n", "keyframe_max_gap: -4"),
    ("keyframe_max_gap: 1\n", "keyframe_max_gap: 1"),                              # checked even while the mode is off
    (ON + "window_ba: 3\n", "keyframe: 1 with window_ba: 3"),
    (ON + "num_features_needed_for_keyframe: 3\n", "num_features_needed_for_keyframe: 3"),
    (ON + "batch_size: 8\n", "keyframe: 1 with batch_size > 1"),
    (ON + "stream_depth: 4\n", "keyframe: 1 with stream_depth > 0"),
])
def test_runner_refuses(host_built, tmp_path, extra, says):
    rc, err = _run(host_built, tmp_path, extra)
    assert rc == 2 and says in err, (rc, err)


def test_orb_mode_refuses(host_built, tmp_path):
    rc, err = _run(host_built, tmp_path, ON, mode="ORB_stereof2f_pnp")
    assert rc == 2 and "track_carry: 1 with track_mode ORB_stereof2f_pnp" in err, (rc, err)     # keyframe needs carry, carry needs LK


def test_split_pairs_and_interleave_refuse(host_built, tmp_path):
    rc, err = _run(host_built, tmp_path, ON, args=("--split-pairs", "2"))
    assert rc == 2 and "keyframe: 1 with --split-pairs" in err, (rc, err)
    rc, err = _run(host_built, tmp_path, "track_carry: 0\nkeyframe: 0\n", args=("--split-pairs", "2"))
    assert rc != 2 and "keyframe" not in err, (rc, err)
    exe = os.path.join(host_built, "run_kitti_stereo")
    d = tmp_path / "seq"
    for cam in (0, 1):
        os.makedirs(d / f"image_{cam}")
        _write_pgm(d / f"image_{cam}" / "000000.pgm", conftest.rand_image(64, 96, cam))
    os.makedirs(tmp_path / "out")

    def run(extra_a, extra_b):
        a = _yaml(tmp_path, "a.yaml", extra_a, dataset=str(d))
        b = _yaml(tmp_path, "b.yaml", extra_b, dataset=str(d))
        r = subprocess.run([exe, str(a), str(b), "--poses-dir", str(tmp_path / "out"), "--interleave"], capture_output=True, timeout=120)
        return r.returncode, r.stderr.decode()

    rc, err = run(ON, ON)
    assert rc == 2 and "keyframe: 1 with --interleave" in err, (rc, err)
    rc, err = run(ON, "track_carry: 1\nkeyframe: 0\n")
    assert rc == 2 and "'keyframe'" in err, (rc, err)
    rc, err = run(ON + "keyframe_max_gap: 1\n", ON + "keyframe_max_gap: 1\n")
    assert rc == 2 and "keyframe_max_gap: 1" in err and "--interleave" in err, (rc, err)


@pytest.mark.parametrize("extra,settings", [
    ("", None),                                                                    # absent: off, silently
    ("track_carry: 1\nkeyframe: 0\nkeyframe_max_gap: 5\n", None),
    ("keyframe: 0\nwindow_ba: 0\n", None),
    (ON, (60, 0)),                                                                 # the reference's key, no gap limit
    (ON + "keyframe_max_gap: 2\n", (60, 2)),
    (ON + "num_features_needed_for_keyframe: 45\nkeyframe_max_gap: 10\nbatch_size: 1\nstream_depth: 0\nwindow_ba: 0\n", (45, 10)),
])
def test_runner_parses_and_defaults_the_keys(host_built, tmp_path, extra, settings):
    """An empty dataset directory: the run gets past the key checks, reports the effective settings when the mode is on, and ends
    where it finds no frames -- not with the configuration's exit code."""
    rc, err = _run(host_built, tmp_path, extra)
    assert rc != 2, (rc, err)
    said = [ln for ln in err.splitlines() if "keyframe: " in ln]
    if settings is None:
        assert said == [], err
    else:
        assert len(said) >= 1 and all(ln.endswith(KEYFRAME_LOG % settings) for ln in said), err


@pytest.mark.gpu
def test_runner_pose_file_equals_the_bindings_chain(host_built, pkg, synth, tmp_path):
    n = 8
    seq = synth.StereoSequence(width=416, height=128, n_frames=n, seed=11)
    frames = [tuple(x.numpy() for x in seq.render(t)) for t in range(n)]
    P1, P2 = seq.proj()
    for cam in (0, 1):
        os.makedirs(tmp_path / f"image_{cam}")
        for t, fr in enumerate(frames):
            _write_pgm(tmp_path / f"image_{cam}" / f"{t:06d}.pgm", fr[cam])
    # the binding's chain under the settings the YAML below gives the runner
    c = pkg.Context(416, 128, device=0, P1=P1, P2=P2, max_batch=2)
    c.set_track_carry(True)
    c.set_keyframe(True, 60, 3)
    want, applied = [], 0
    for t, fr in enumerate(frames):
        rc, g = c.add_frame(*fr)
        assert rc == 0
        want.append(g["pose"].reshape(4, 4)[:3].copy())
        applied += t > 0 and c.keyframe_result()["status"] == pkg.KF_APPLIED
    c.close()
    assert applied >= 3
    outs = {}
    for on in (1, 0):
        y = tmp_path / f"kf{on}.yaml"
        _write_yaml(y, str(tmp_path), fx=seq.fx, fy=seq.fy, cx=seq.cx, cy=seq.cy)
        with open(y, "a", encoding="utf-8") as f:
            f.write(f"track_carry: 1\nkeyframe: {on}\nkeyframe_max_gap: 3\n")
        r = subprocess.run([os.path.join(host_built, "run_kitti_stereo"), str(y), str(tmp_path / f"kf{on}.txt")], capture_output=True)
        assert r.returncode == 0, r.stderr.decode()
        outs[on] = np.loadtxt(tmp_path / f"kf{on}.txt").reshape(-1, 3, 4)
    assert outs[1].shape[0] == n and np.abs(outs[1] - np.array(want)).max() < 1e-6
    assert np.abs(outs[1] - outs[0]).max() > 1e-4                    # ... and they are not the carry-only chain's
