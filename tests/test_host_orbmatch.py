"""CPU test of the host C++ layer's guided-matcher keys (orb_matcher, orb_match_th_stereo, orb_match_th_track, orb_match_ratio,
orb_match_radius, orb_max_disparity): they reach lzb_vio::Parameter and Tracking::ReadOrbMatcher, absent keys leave the
reference's brute-force matcher, and a bad value is refused on the host with a message that names the key."""
import os
import subprocess

import pytest

import test_host_api as H


@pytest.fixture(scope="module")
def host_built(pkg):
    pkg.build_library()
    subprocess.check_call(["make", "-C", H.HOST], stdout=subprocess.DEVNULL)
    return H.HOST


def _selftest(host_built, tmp_path, extra, mode="ORB_stereof2f_pnp"):
    H._write_yaml(tmp_path / "cfg.yaml", "/data/kitti/00", mode=mode)
    with open(tmp_path / "cfg.yaml", "a", encoding="utf-8") as f:
        f.write(extra)
    out = subprocess.check_output([os.path.join(host_built, "host_selftest"), str(tmp_path / "cfg.yaml")], stderr=subprocess.DEVNULL).decode()
    return dict(l.split("=", 1) for l in out.strip().split("\n") if l.startswith("orb_matcher"))


def test_absent_keys_leave_the_brute_matcher(host_built, tmp_path):
    d = _selftest(host_built, tmp_path, "")
    assert d["orb_matcher_param"] == "brute 75 100 0.90000000000000002 0 0"
    assert d["orb_matcher_ok"] == "1" and d["orb_matcher"] == d["orb_matcher_param"]


def test_keys_reach_parameter(host_built, tmp_path):
    d = _selftest(host_built, tmp_path, "orb_matcher: guided\norb_match_th_stereo: 60\norb_match_th_track: 90\norb_match_ratio: 0.75\n"
                                        "orb_match_radius: 64\norb_max_disparity: 200.5\n")
    assert d["orb_matcher_param"] == "guided 60 90 0.75 64 200.5"
    assert d["orb_matcher_ok"] == "1" and d["orb_matcher"] == d["orb_matcher_param"]


@pytest.mark.parametrize("extra,key", [("orb_matcher: fancy\n", "orb_matcher"), ("orb_matcher: guided\norb_match_th_stereo: 0\n", "orb_match_th_stereo"),
                                       ("orb_match_th_track: 257\n", "orb_match_th_track"), ("orb_match_ratio: 1.5\n", "orb_match_ratio"),
                                       ("orb_match_ratio: 0\n", "orb_match_ratio"), ("orb_match_radius: -1\n", "orb_match_radius"),
                                       ("orb_max_disparity: -3\n", "orb_max_disparity")])
def test_bad_values_are_refused(host_built, tmp_path, extra, key):
    d = _selftest(host_built, tmp_path, extra)
    assert d["orb_matcher_ok"] == "0" and d["orb_matcher"].startswith("brute 75 100 ")
    assert d["orb_matcher_error"].startswith(key + ":")


def test_guided_needs_orb_mode_and_the_runner_refuses(host_built, tmp_path):
    d = _selftest(host_built, tmp_path, "orb_matcher: guided\n", mode="LK_stereof2f_pnp")
    assert d["orb_matcher_ok"] == "0" and "track_mode" in d["orb_matcher_error"]
    # run_kitti_stereo refuses the configuration on the host, before a device is opened
    r = subprocess.run([os.path.join(host_built, "run_kitti_stereo"), str(tmp_path / "cfg.yaml"), str(tmp_path / "poses.txt")],
                       stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
    assert r.returncode != 0 and b"orb_matcher" in r.stderr
