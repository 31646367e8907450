"""CPU tests of the host mirror's additive YAML keys lk_detector / gftt_quality_level / gftt_min_distance (the corner count is
the existing num_features): an unknown detector, a bad value, or gftt together with ORB mode, the FAST buckets or
fast_keep_strongest makes run_kitti_stereo exit 2 with the key named, and --interleave refuses YAMLs that differ in them -- on
the host, before a device is opened, so none of this needs a GPU.  Good values get past these checks: the run then ends where it
looks for frames (or for a device), never with the key's message.  (The runner against the Python path: tests/test_gpu_gftt.py.)"""
import os
import subprocess

import pytest

from test_host_api import _write_pgm, _write_yaml, host_built   # noqa: F401  (host_built: the fixture that builds host/)
from test_host_buckets import _yaml
import conftest

KEYS = ("lk_detector", "gftt_quality_level", "gftt_min_distance")
BUCKETS = "fast_bucket_width: 32\nfast_bucket_height: 32\nfast_bucket_keep: 2\n"


@pytest.mark.parametrize("extra,mode,key", [
    ("lk_detector: harris\n", "LK_stereof2f_pnp", "lk_detector"),
    ("lk_detector: GFTT\n", "LK_stereof2f_pnp", "lk_detector"),                      # the values are case sensitive
    ("lk_detector: gftt\ngftt_quality_level: 0\n", "LK_stereof2f_pnp", "gftt_quality_level"),
    ("lk_detector: gftt\ngftt_quality_level: -0.01\n", "LK_stereof2f_pnp", "gftt_quality_level"),
    ("lk_detector: gftt\ngftt_quality_level: high\n", "LK_stereof2f_pnp", "gftt_quality_level"),
    ("lk_detector: gftt\ngftt_min_distance: -1\n", "LK_stereof2f_pnp", "gftt_min_distance"),
    ("gftt_min_distance: -1\n", "LK_stereof2f_pnp", "gftt_min_distance"),             # checked even while the detector is fast
    ("lk_detector: gftt\n", "ORB_stereof2f_pnp", "lk_detector"),
    ("lk_detector: gftt\n" + BUCKETS, "LK_stereof2f_pnp", "lk_detector"),
    ("lk_detector: gftt\nfast_keep_strongest: 500\n", "LK_stereof2f_pnp", "lk_detector"),
])
def test_runner_refuses_a_bad_combination(host_built, tmp_path, extra, mode, key):
    exe = os.path.join(host_built, "run_kitti_stereo")
    y = _yaml(tmp_path, "bad.yaml", extra, dataset=str(tmp_path), mode=mode)
    r = subprocess.run([exe, str(y), str(tmp_path / "poses.txt")], capture_output=True, timeout=120)
    assert r.returncode == 2 and key + ":" in r.stderr.decode(), (r.returncode, r.stderr.decode())


GFTT_LOG = "lk_detector: gftt (num_features %d, gftt_quality_level %g, gftt_min_distance %g)"


@pytest.mark.parametrize("extra,mode,settings", [
    ("", "LK_stereof2f_pnp", None),                                                  # absent: fast
    ("lk_detector: fast\n", "LK_stereof2f_pnp", None),
    ("lk_detector: fast\n" + BUCKETS, "LK_stereof2f_pnp", None),
    ("lk_detector: fast\ngftt_quality_level: 0.5\ngftt_min_distance: 3\n", "ORB_stereof2f_pnp", None),
    ("lk_detector: gftt\n", "LK_stereof2f_pnp", (500, 0.01, 20)),                    # the reference's literals are the defaults
    ("lk_detector: gftt\nnum_features: 321\n", "LK_stereof2f_pnp", (321, 0.01, 20)),
    ("lk_detector: gftt\ngftt_quality_level: 0.05\n", "LK_stereof2f_pnp", (500, 0.05, 20)),
    ("lk_detector: gftt\ngftt_min_distance: 7.5\n", "LK_stereof2f_pnp", (500, 0.01, 7.5)),
    ("lk_detector: gftt\ngftt_min_distance: 0\nfast_bucket_keep: 0\nfast_keep_strongest: 0\n", "LK_stereof2f_pnp", (500, 0.01, 0)),
])
def test_runner_parses_and_defaults_the_keys(host_built, tmp_path, extra, mode, settings):
    """An empty dataset directory: the run gets past the key checks (never exit code 2, never a key's message), reports the
    effective detector settings when the detector is gftt, and ends where it finds no frames."""
    exe = os.path.join(host_built, "run_kitti_stereo")
    y = _yaml(tmp_path, "good.yaml", extra, dataset=str(tmp_path), mode=mode)
    r = subprocess.run([exe, str(y), str(tmp_path / "poses.txt")], capture_output=True, timeout=120)
    err = r.stderr.decode()
    assert r.returncode != 2, err
    said = [ln for ln in err.splitlines() if "lk_detector:" in ln or "gftt_quality_level:" in ln or "gftt_min_distance:" in ln]
    if settings is None:
        assert said == [], err
    else:
        assert len(said) >= 1 and all(ln.endswith(GFTT_LOG % settings) for ln in said), err


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

    rc, err = run("lk_detector: gftt\n", "lk_detector: fast\n")
    assert rc == 2 and "'lk_detector'" in err
    rc, err = run("lk_detector: gftt\n", "")
    assert rc == 2 and "'lk_detector'" in err
    rc, err = run("lk_detector: gftt\ngftt_min_distance: 20\n", "lk_detector: gftt\ngftt_min_distance: 10\n")
    assert rc == 2 and "'gftt_min_distance'" in err
    rc, err = run("lk_detector: gftt\ngftt_quality_level: 0.01\n", "lk_detector: gftt\ngftt_quality_level: 0.02\n")
    assert rc == 2 and "'gftt_quality_level'" in err
    rc, err = run("lk_detector: corners\n", "lk_detector: corners\n")                 # equal, but refused with the key named
    assert rc == 2 and "lk_detector:" in err and "--interleave" in err
