"""CPU tests of the host mirror's additive YAML keys track_carry / track_carry_min_distance / track_carry_max_age
(svo_set_track_carry): a bad value or ORB mode makes run_kitti_stereo exit 2 with the key named; track_carry: 1 together with
batch_size > 1, stream_depth > 0 or --split-pairs is refused at start; the tracks_file header announces the id / age columns
only when carry is on -- all on the host, before a device is opened.  (The T rows against the twin: tests/test_gpu_carry.py.)"""
import os
import subprocess

import pytest

from test_host_api import _write_pgm, _write_yaml, host_built   # noqa: F401  (host_built: the fixture that builds host/)
from test_host_buckets import _yaml
import conftest

CARRY_LOG = "track_carry: 1 (track_carry_min_distance %g, track_carry_max_age %d)"
HEADER = "# F frame ok fail_stage n_cur_kps n_tracked n_inliers / T x1l y1l x1r y1r x2l y2l inlier"


def _run(host_built, tmp_path, extra, mode="LK_stereof2f_pnp", args=()):
    exe = os.path.join(host_built, "run_kitti_stereo")
    y = _yaml(tmp_path, "c.yaml", extra, dataset=str(tmp_path), mode=mode)
    r = subprocess.run([exe, str(y), str(tmp_path / "poses.txt"), *args], capture_output=True, timeout=120)
    return r.returncode, r.stderr.decode()


@pytest.mark.parametrize("extra,mode,key", [
    ("track_carry: 2\n", "LK_stereof2f_pnp", "track_carry"),
    ("track_carry: -1\n", "LK_stereof2f_pnp", "track_carry"),
    ("track_carry: 1\ntrack_carry_min_distance: 0.5\n", "LK_stereof2f_pnp", "track_carry_min_distance"),
    ("track_carry: 1\ntrack_carry_min_distance: 300\n", "LK_stereof2f_pnp", "track_carry_min_distance"),
    ("track_carry_min_distance: near\n", "LK_stereof2f_pnp", "track_carry_min_distance"),      # checked even while carry is off
    ("track_carry: 1\ntrack_carry_max_age: -3\n", "LK_stereof2f_pnp", "track_carry_max_age"),
    ("track_carry: 1\n", "ORB_stereof2f_pnp", "track_carry"),
    ("track_carry: 1\nbatch_size: 8\n", "LK_stereof2f_pnp", "track_carry"),
    ("track_carry: 1\nstream_depth: 4\n", "LK_stereof2f_pnp", "track_carry"),
])
def test_runner_refuses(host_built, tmp_path, extra, mode, key):
    rc, err = _run(host_built, tmp_path, extra, mode)
    assert rc == 2 and key + ":" in err, (rc, err)
    if "batch_size" in extra or "stream_depth" in extra:
        assert ("batch_size > 1" if "batch_size" in extra else "stream_depth > 0") in err


def test_split_pairs_refuses(host_built, tmp_path):
    rc, err = _run(host_built, tmp_path, "track_carry: 1\n", args=("--split-pairs", "2"))
    assert rc == 2 and "track_carry: 1 with --split-pairs" in err, (rc, err)
    rc, err = _run(host_built, tmp_path, "track_carry: 0\n", args=("--split-pairs", "2"))
    assert rc != 2 and "track_carry" not in err, (rc, err)


@pytest.mark.parametrize("extra,mode,settings", [
    ("", "LK_stereof2f_pnp", None),                                                  # absent: off, silently
    ("track_carry: 0\ntrack_carry_min_distance: 5\ntrack_carry_max_age: 2\n", "LK_stereof2f_pnp", None),
    ("track_carry: 0\nbatch_size: 8\n", "LK_stereof2f_pnp", None),
    ("track_carry: 0\n", "ORB_stereof2f_pnp", None),
    ("track_carry: 1\n", "LK_stereof2f_pnp", (3.0, 0)),                              # the defaults
    ("track_carry: 1\ntrack_carry_min_distance: 7.5\n", "LK_stereof2f_pnp", (7.5, 0)),
    ("track_carry: 1\ntrack_carry_max_age: 12\nbatch_size: 1\nstream_depth: 0\n", "LK_stereof2f_pnp", (3.0, 12)),
])
def test_runner_parses_and_defaults_the_keys(host_built, tmp_path, extra, mode, settings):
    """An empty dataset directory: the run gets past the key checks, reports the effective settings when carry is on, and ends
    where it finds no frames."""
    rc, err = _run(host_built, tmp_path, extra, mode)
    assert rc != 2, err
    said = [ln for ln in err.splitlines() if "track_carry" in ln]
    if settings is None:
        assert said == [], err
    else:
        assert len(said) >= 1 and all(ln.endswith(CARRY_LOG % settings) for ln in said), err


@pytest.mark.parametrize("on", [0, 1])
def test_tracks_file_header_names_the_columns(host_built, tmp_path, on):
    out = tmp_path / "tracks.txt"
    rc, err = _run(host_built, tmp_path, "track_carry: %d\ntracks_file: %s\n" % (on, out))
    assert rc != 2, err
    assert open(out).read().splitlines()[0] == HEADER + (" id age" if on else "")


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

    rc, err = run("track_carry: 1\n", "track_carry: 0\n")
    assert rc == 2 and "'track_carry'" in err
    rc, err = run("track_carry: 1\ntrack_carry_min_distance: 3\n", "track_carry: 1\ntrack_carry_min_distance: 4\n")
    assert rc == 2 and "'track_carry_min_distance'" in err
    rc, err = run("track_carry: 3\n", "track_carry: 3\n")                            # equal, but refused with the key named
    assert rc == 2 and "track_carry:" in err and "--interleave" in err
