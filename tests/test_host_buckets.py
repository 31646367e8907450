"""CPU tests of the host mirror's additive YAML keys fast_bucket_width / fast_bucket_height / fast_bucket_keep: a bad
combination (a keep value without sizes, a size < 1, ORB mode with keep > 0) makes run_kitti_stereo exit 2 with the key named,
and --interleave refuses YAMLs that differ in them -- on the host, before a device is opened, so none of this needs a GPU.
(The runner itself against the Python path: tests/test_gpu_buckets.py.)"""
import os
import subprocess

import pytest

from test_host_api import _write_pgm, _write_yaml, host_built   # noqa: F401  (host_built: the fixture that builds host/)
import conftest


def _yaml(tmp_path, name, extra, dataset="/data/none", **kw):
    y = tmp_path / name
    _write_yaml(y, dataset, **kw)
    with open(y, "a", encoding="utf-8") as f:
        f.write(extra)
    return y


@pytest.mark.parametrize("extra,mode,key", [
    ("fast_bucket_keep: 4\n", "LK_stereof2f_pnp", "fast_bucket_keep"),
    ("fast_bucket_keep: 4\nfast_bucket_width: 50\n", "LK_stereof2f_pnp", "fast_bucket_height"),
    ("fast_bucket_keep: 4\nfast_bucket_height: 50\n", "LK_stereof2f_pnp", "fast_bucket_width"),
    ("fast_bucket_keep: 4\nfast_bucket_width: 0\nfast_bucket_height: 50\n", "LK_stereof2f_pnp", "fast_bucket_width"),
    ("fast_bucket_keep: 4\nfast_bucket_width: 50\nfast_bucket_height: -3\n", "LK_stereof2f_pnp", "fast_bucket_height"),
    ("fast_bucket_keep: -1\nfast_bucket_width: 50\nfast_bucket_height: 50\n", "LK_stereof2f_pnp", "fast_bucket_keep"),
    ("fast_bucket_keep: 4\nfast_bucket_width: 50\nfast_bucket_height: 50\n", "ORB_stereof2f_pnp", "fast_bucket_keep"),
])
def test_runner_refuses_a_bad_combination(host_built, tmp_path, extra, mode, key):
    exe = os.path.join(host_built, "run_kitti_stereo")
    y = _yaml(tmp_path, "bad.yaml", extra, dataset=str(tmp_path), mode=mode)
    r = subprocess.run([exe, str(y), str(tmp_path / "poses.txt")], capture_output=True, timeout=120)
    assert r.returncode == 2 and key in r.stderr.decode(), (r.returncode, r.stderr.decode())


def test_interleave_refuses_yamls_that_differ_in_the_keys(host_built, tmp_path):
    exe = os.path.join(host_built, "run_kitti_stereo")
    d = tmp_path / "seq"
    for cam in (0, 1):
        os.makedirs(d / f"image_{cam}")
        _write_pgm(d / f"image_{cam}" / "000000.pgm", conftest.rand_image(64, 96, cam))
    os.makedirs(tmp_path / "out")
    size = "fast_bucket_width: 32\nfast_bucket_height: 32\n"

    def run(extra_a, extra_b):
        a = _yaml(tmp_path, "a.yaml", extra_a, dataset=str(d))
        b = _yaml(tmp_path, "b.yaml", extra_b, dataset=str(d))
        r = subprocess.run([exe, str(a), str(b), "--poses-dir", str(tmp_path / "out"), "--interleave"], capture_output=True, timeout=120)
        return r.returncode, r.stderr.decode()

    rc, err = run(size + "fast_bucket_keep: 2\n", size + "fast_bucket_keep: 3\n")
    assert rc == 2 and "'fast_bucket_keep'" in err
    rc, err = run(size + "fast_bucket_keep: 2\n", size)
    assert rc == 2 and "'fast_bucket_keep'" in err
    rc, err = run(size + "fast_bucket_keep: 2\n", "fast_bucket_width: 32\nfast_bucket_height: 16\nfast_bucket_keep: 2\n")
    assert rc == 2 and "'fast_bucket_height'" in err
    rc, err = run("fast_bucket_keep: 2\n", "fast_bucket_keep: 2\n")          # equal, but no sizes: refused with the key named
    assert rc == 2 and "fast_bucket_keep" in err and "--interleave" in err
