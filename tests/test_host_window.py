"""CPU tests of the host mirror's additive YAML keys window_ba / window_ba_rounds / _iters / _sigma / _min_obs
(svo_set_window_ba): a bad value, or window_ba without track_carry: 1, makes run_kitti_stereo exit 2 with the key named; good
values are reported as they take effect -- all on the host, before a device is opened."""
import os
import subprocess

import pytest

from test_host_api import _write_pgm, _write_yaml, host_built   # noqa: F401  (host_built: the fixture that builds host/)
from test_host_buckets import _yaml

WINDOW_LOG = "window_ba: %d (window_ba_rounds %d, window_ba_iters %d, window_ba_sigma %g, window_ba_min_obs %d)"


def _run(host_built, tmp_path, extra, mode="LK_stereof2f_pnp"):
    exe = os.path.join(host_built, "run_kitti_stereo")
    y = _yaml(tmp_path, "c.yaml", extra, dataset=str(tmp_path), mode=mode)
    r = subprocess.run([exe, str(y), str(tmp_path / "poses.txt")], capture_output=True, timeout=120)
    return r.returncode, r.stderr.decode()


@pytest.mark.parametrize("extra,key", [
    ("window_ba: 3\n", "window_ba"),                                              # the refusal: no track_carry: 1
    ("track_carry: 0\nwindow_ba: 5\n", "window_ba"),
    ("track_carry: 1\nwindow_ba: 1\n", "window_ba"),
    ("track_carry: 1\nwindow_ba: 9\n", "window_ba"),
    ("track_carry: 1\nwindow_ba: -2\n", "window_ba"),
    ("track_carry: 1\nwindow_ba: 3\nwindow_ba_rounds: 0\n", "window_ba_rounds"),
    ("track_carry: 1\nwindow_ba: 3\nwindow_ba_iters: 101\n", "window_ba_iters"),
    ("track_carry: 1\nwindow_ba: 3\nwindow_ba_sigma: 0\n", "window_ba_sigma"),
    ("track_carry: 1\nwindow_ba: 3\nwindow_ba_min_obs: 0\n", "window_ba_min_obs"),
    ("window_ba_rounds: 17\n", "window_ba_rounds"),                               # checked even while the window is off
])
def test_runner_refuses(host_built, tmp_path, extra, key):
    rc, err = _run(host_built, tmp_path, extra)
    assert rc == 2 and key + ":" in err, (rc, err)


@pytest.mark.parametrize("extra,settings", [
    ("", None),                                                                   # absent: off, silently
    ("track_carry: 1\nwindow_ba: 0\nwindow_ba_rounds: 3\n", None),
    ("track_carry: 1\nwindow_ba: 5\n", (5, 4, 5, 1.0, 10)),                       # the defaults
    ("track_carry: 1\nwindow_ba: 8\nwindow_ba_rounds: 2\nwindow_ba_iters: 7\nwindow_ba_sigma: 0.5\nwindow_ba_min_obs: 20\n", (8, 2, 7, 0.5, 20)),
])
def test_runner_parses_and_defaults_the_keys(host_built, tmp_path, extra, settings):
    """An empty dataset directory: the run gets past the key checks, reports the effective settings when the window is on, and
    ends for want of images -- not with the configuration's exit code."""
    rc, err = _run(host_built, tmp_path, extra)
    assert rc != 2, (rc, err)
    if settings is None:
        assert "window_ba:" not in err
    else:
        assert WINDOW_LOG % settings in err, err
