"""CPU tests of the host mirror's additive YAML keys image_scale / image_interp: they parse, a YAML without them reports no
ingest stage, and a value outside (0, 1] or a pair of --interleave YAMLs that differ in them is refused with the key named --
on the host, before a device is opened, so none of this needs a GPU.  (The runner itself, against hand-downscaled files:
tests/test_gpu_ingest.py.)"""
import os
import subprocess

import pytest

from test_host_api import _write_pgm, _write_yaml, host_built   # noqa: F401  (host_built: the fixture that builds host/)
import conftest


def _selftest(host_built, yaml):
    r = subprocess.run([os.path.join(host_built, "host_selftest"), str(yaml)], capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr.decode()
    return dict(l.split("=", 1) for l in r.stdout.decode().splitlines() if l.count("=") == 1), r.stderr.decode()


def _yaml(tmp_path, name, extra, dataset="/data/none"):
    y = tmp_path / name
    _write_yaml(y, dataset)
    with open(y, "a", encoding="utf-8") as f:
        f.write(extra)
    return y


def test_keys_parse_and_default_to_no_ingest_stage(host_built, tmp_path):
    kv, _ = _selftest(host_built, _yaml(tmp_path, "plain.yaml", ""))
    assert kv["image_scale_ok"] == "1" and float(kv["image_scale"]) == 1.0 and kv["image_interp"] == "nearest" and kv["ingest"] == "0"
    kv, _ = _selftest(host_built, _yaml(tmp_path, "one.yaml", "image_scale: 1\nimage_interp: linear\n"))
    assert kv["image_scale_ok"] == "1" and kv["ingest"] == "0" and kv["image_interp"] == "linear"
    kv, _ = _selftest(host_built, _yaml(tmp_path, "half.yaml", "image_scale: 0.5\n"))
    assert kv["ingest"] == "1" and float(kv["image_scale"]) == 0.5 and kv["image_interp"] == "nearest"
    kv, _ = _selftest(host_built, _yaml(tmp_path, "zed.yaml", "image_scale: 0.6\nimage_interp: linear\n"))
    assert kv["ingest"] == "1" and float(kv["image_scale"]) == 0.6 and kv["image_interp"] == "linear"
    kv, err = _selftest(host_built, _yaml(tmp_path, "word.yaml", "image_scale: 0.5\nimage_interp: cubic\n"))
    assert kv["ingest"] == "1" and kv["image_interp"] == "nearest" and "image_interp" in err and "cubic" in err
    for bad in ("0", "1.5", "-0.5"):
        kv, _ = _selftest(host_built, _yaml(tmp_path, "bad.yaml", f"image_scale: {bad}\n"))
        assert kv["image_scale_ok"] == "0" and kv["ingest"] == "0" and "image_scale" in kv["image_scale_error"]


@pytest.mark.parametrize("bad", ["0", "1.5"])
def test_runner_refuses_a_scale_outside_the_range(host_built, tmp_path, bad):
    exe = os.path.join(host_built, "run_kitti_stereo")
    y = _yaml(tmp_path, "bad.yaml", f"image_scale: {bad}\n", dataset=str(tmp_path))
    r = subprocess.run([exe, str(y), str(tmp_path / "poses.txt")], capture_output=True, timeout=120)
    assert r.returncode == 2 and "image_scale" in r.stderr.decode(), (r.returncode, r.stderr.decode())


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

    rc, err = run("image_scale: 0.5\n", "image_scale: 0.6\n")
    assert rc == 2 and "'image_scale'" in err
    rc, err = run("image_scale: 0.5\n", "")
    assert rc == 2 and "'image_scale'" in err
    rc, err = run("image_scale: 0.5\nimage_interp: linear\n", "image_scale: 0.5\nimage_interp: nearest\n")
    assert rc == 2 and "'image_interp'" in err
    rc, err = run("image_scale: 1.5\n", "image_scale: 1.5\n")
    assert rc == 2 and "image_scale" in err and "(0, 1]" in err
