"""CPU tests of the host mirror's YAML value pose_refine: ba (the pose stage's bundle-adjustment mode): it is accepted in both
track modes with the other pose_refine_* keys, reported with the effective settings, and --interleave treats it as one more
value of the shared key.  As tests/test_host_refine.py: on the host, before a device is opened."""
import os
import subprocess

import pytest

from test_host_api import _write_pgm, host_built   # noqa: F401  (host_built: the fixture that builds host/)
from test_host_buckets import _yaml
import conftest

BA_LOG = "pose_refine: ba (pose_refine_rounds %d, pose_refine_iters %d, pose_refine_sigma %g, pose_refine_min_inliers %d)"


@pytest.mark.parametrize("extra,mode,settings", [
    ("pose_refine: ba\n", "LK_stereof2f_pnp", (4, 10, 1, 6)),
    ("pose_refine: ba\n", "ORB_stereof2f_pnp", (4, 10, 1, 6)),
    ("pose_refine: ba\npose_refine_rounds: 3\npose_refine_iters: 15\npose_refine_sigma: 0.5\npose_refine_min_inliers: 20\n",
     "LK_stereof2f_pnp", (3, 15, 0.5, 20)),
])
def test_runner_accepts_ba(host_built, tmp_path, extra, mode, settings):
    exe = os.path.join(host_built, "run_kitti_stereo")
    y = _yaml(tmp_path, "good.yaml", extra, dataset=str(tmp_path), mode=mode)
    r = subprocess.run([exe, str(y), str(tmp_path / "poses.txt")], capture_output=True, timeout=120)
    err = r.stderr.decode()
    assert r.returncode != 2, err
    said = [ln for ln in err.splitlines() if "pose_refine" in ln]
    assert len(said) >= 1 and all(ln.endswith(BA_LOG % settings) for ln in said), err


@pytest.mark.parametrize("extra,key", [("pose_refine: BA\n", "pose_refine"), ("pose_refine: ba\npose_refine_iters: 0\n", "pose_refine_iters")])
def test_runner_refuses_a_bad_value(host_built, tmp_path, extra, key):
    exe = os.path.join(host_built, "run_kitti_stereo")
    y = _yaml(tmp_path, "bad.yaml", extra, dataset=str(tmp_path))
    r = subprocess.run([exe, str(y), str(tmp_path / "poses.txt")], capture_output=True, timeout=120)
    assert r.returncode == 2 and key + ":" in r.stderr.decode(), (r.returncode, r.stderr.decode())


def test_interleave_refuses_yamls_that_differ_in_the_mode(host_built, tmp_path):
    exe = os.path.join(host_built, "run_kitti_stereo")
    d = tmp_path / "seq"
    for cam in (0, 1):
        os.makedirs(d / f"image_{cam}")
        _write_pgm(d / f"image_{cam}" / "000000.pgm", conftest.rand_image(64, 96, cam))
    os.makedirs(tmp_path / "out")
    a = _yaml(tmp_path, "a.yaml", "pose_refine: ba\n", dataset=str(d))
    b = _yaml(tmp_path, "b.yaml", "pose_refine: reproj\n", dataset=str(d))
    r = subprocess.run([exe, str(a), str(b), "--poses-dir", str(tmp_path / "out"), "--interleave"], capture_output=True, timeout=120)
    assert r.returncode == 2 and "'pose_refine'" in r.stderr.decode()
