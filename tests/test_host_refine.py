"""CPU tests of the host mirror's additive YAML keys pose_refine / pose_refine_rounds / pose_refine_iters / pose_refine_sigma /
pose_refine_min_inliers: a bad value makes run_kitti_stereo exit 2 with the key named -- on the host, before a device is opened,
so none of this needs a GPU -- and --interleave refuses YAMLs that differ in them.  Good values get past the checks: the run then
ends where it looks for frames (or for a device), never with a key's message.  The default is off: nothing is said."""
import os
import subprocess

import pytest

from test_host_api import _write_pgm, host_built   # noqa: F401  (host_built: the fixture that builds host/)
from test_host_buckets import _yaml
import conftest

REFINE_LOG = "pose_refine: reproj (pose_refine_rounds %d, pose_refine_iters %d, pose_refine_sigma %g, pose_refine_min_inliers %d)"


@pytest.mark.parametrize("mode", ["LK_stereof2f_pnp", "ORB_stereof2f_pnp"])
@pytest.mark.parametrize("extra,key", [
    ("pose_refine: g2o\n", "pose_refine"),
    ("pose_refine: Reproj\n", "pose_refine"),                                        # the values are case sensitive
    ("pose_refine: reproj\npose_refine_rounds: 0\n", "pose_refine_rounds"),
    ("pose_refine: reproj\npose_refine_rounds: 17\n", "pose_refine_rounds"),
    ("pose_refine: reproj\npose_refine_iters: 0\n", "pose_refine_iters"),
    ("pose_refine: reproj\npose_refine_iters: 101\n", "pose_refine_iters"),
    ("pose_refine: reproj\npose_refine_iters: many\n", "pose_refine_iters"),
    ("pose_refine: reproj\npose_refine_sigma: 0\n", "pose_refine_sigma"),
    ("pose_refine: reproj\npose_refine_sigma: -1.5\n", "pose_refine_sigma"),
    ("pose_refine: reproj\npose_refine_min_inliers: 0\n", "pose_refine_min_inliers"),
    ("pose_refine_sigma: -1\n", "pose_refine_sigma"),                                # checked even while the stage is off
])
def test_runner_refuses_a_bad_value(host_built, tmp_path, extra, key, mode):
    exe = os.path.join(host_built, "run_kitti_stereo")
    y = _yaml(tmp_path, "bad.yaml", extra, dataset=str(tmp_path), mode=mode)
    r = subprocess.run([exe, str(y), str(tmp_path / "poses.txt")], capture_output=True, timeout=120)
    assert r.returncode == 2 and key + ":" in r.stderr.decode(), (r.returncode, r.stderr.decode())


@pytest.mark.parametrize("extra,mode,settings", [
    ("", "LK_stereof2f_pnp", None),                                                  # absent: off
    ("pose_refine: none\n", "LK_stereof2f_pnp", None),
    ("pose_refine: none\npose_refine_rounds: 2\npose_refine_sigma: 0.5\n", "ORB_stereof2f_pnp", None),
    ("pose_refine: reproj\n", "LK_stereof2f_pnp", (4, 10, 1, 6)),                    # the defaults
    ("pose_refine: reproj\n", "ORB_stereof2f_pnp", (4, 10, 1, 6)),
    ("pose_refine: reproj\npose_refine_rounds: 2\npose_refine_iters: 25\n", "LK_stereof2f_pnp", (2, 25, 1, 6)),
    ("pose_refine: reproj\npose_refine_sigma: 0.75\npose_refine_min_inliers: 12\n", "LK_stereof2f_pnp", (4, 10, 0.75, 12)),
])
def test_runner_parses_and_defaults_the_keys(host_built, tmp_path, extra, mode, settings):
    """An empty dataset directory: the run gets past the key checks (never exit code 2, never a key's message), reports the
    effective settings when the stage is on, and ends where it finds no frames."""
    exe = os.path.join(host_built, "run_kitti_stereo")
    y = _yaml(tmp_path, "good.yaml", extra, dataset=str(tmp_path), mode=mode)
    r = subprocess.run([exe, str(y), str(tmp_path / "poses.txt")], capture_output=True, timeout=120)
    err = r.stderr.decode()
    assert r.returncode != 2, err
    said = [ln for ln in err.splitlines() if "pose_refine" in ln]
    if settings is None:
        assert said == [], err
    else:
        assert len(said) >= 1 and all(ln.endswith(REFINE_LOG % settings) for ln in said), err


def test_interleave_refuses_yamls_that_differ_in_the_keys(host_built, tmp_path):
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

    rc, err = run("pose_refine: reproj\n", "pose_refine: none\n")
    assert rc == 2 and "'pose_refine'" in err
    rc, err = run("pose_refine: reproj\n", "")
    assert rc == 2 and "'pose_refine'" in err
    rc, err = run("pose_refine: reproj\npose_refine_sigma: 1\n", "pose_refine: reproj\npose_refine_sigma: 2\n")
    assert rc == 2 and "'pose_refine_sigma'" in err
    rc, err = run("pose_refine: bundle\n", "pose_refine: bundle\n")                   # equal, but refused with the key named
    assert rc == 2 and "pose_refine:" in err and "--interleave" in err
