"""bench.py --dump-outputs, --steps and --full.  CPU: the argument checks and the dump's layout and 64 MB bound on stand-in
records.  GPU (-m gpu): the timed path's last step is dumped, --steps is the number of timed steps, two runs with
the same arguments write the same arrays, and a plain run carries none of --full's extras but dumps what a self-checked
--full run dumps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import conftest


def _bench(*flags, timeout=600):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    return subprocess.run([sys.executable, os.path.join(conftest.ROOT, "bench.py")] + list(flags), capture_output=True,
                          timeout=timeout, env=env)


def _records(pkg, n):
    recs = np.zeros(n, dtype=pkg.STEP_DTYPE)
    rng = np.random.default_rng(3)
    recs["n_tracked"] = rng.integers(0, 2000, n)
    recs["pose"] = rng.standard_normal((n, 16))
    return recs


def test_steps_below_one_and_dump_with_scaling_table_are_refused():
    r = _bench("--steps", "0", timeout=120)
    assert r.returncode == 2 and "--steps must be >= 1" in r.stderr.decode()
    r = _bench("--gpus", "2", "--scaling-table", "--dump-outputs", "x", timeout=120)
    assert r.returncode == 2 and "--dump-outputs" in r.stderr.decode()
    r = _bench("--self-check-sabotage", timeout=120)
    assert r.returncode == 2 and "--self-check-sabotage needs --full" in r.stderr.decode()


def test_dump_writes_every_field_as_float64(pkg, tmp_path):
    import bench
    recs = _records(pkg, 10)
    info = bench.dump_outputs(str(tmp_path), recs)
    assert info["pairs"] == 10 and not info["sampled"]
    assert sorted(p[:-4] for p in os.listdir(tmp_path)) == sorted(["pair_index"] + list(pkg.STEP_DTYPE.names))
    for k in pkg.STEP_DTYPE.names:
        a = np.load(tmp_path / f"{k}.npy")
        assert a.dtype == np.float64 and a.shape == (10,) + pkg.STEP_DTYPE[k].shape, k
        assert np.array_equal(a, recs[k]), k
    assert np.array_equal(np.load(tmp_path / "pair_index.npy"), np.arange(10))


def test_dump_above_the_limit_is_a_fixed_sample(pkg, tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 64 << 10)
    recs = _records(pkg, 1000)
    a, b = tmp_path / "a", tmp_path / "b"
    ia, ib = bench.dump_outputs(str(a), recs), bench.dump_outputs(str(b), recs)
    assert ia["sampled"] and 0 < ia["pairs"] < 1000 and ia == dict(ib, dir=str(a))
    assert sum(os.path.getsize(p) for p in a.iterdir()) <= (64 << 10) + 1024 * len(os.listdir(a))     # + .npy headers
    idx = np.load(a / "pair_index.npy").astype(np.int64)
    assert np.array_equal(idx, np.load(b / "pair_index.npy")) and (np.diff(idx) > 0).all()
    assert np.array_equal(np.load(a / "pose.npy"), recs["pose"][idx])


@pytest.mark.gpu
def test_dump_outputs_of_the_timed_path_repeat_exactly(tmp_path):
    flags = ["--full", "--steps", "3", "--warmup", "1", "--batch", "12", "--chunks", "2", "--cpu-pairs", "0", "--e2e-frames", "0",
             "--no-legs", "--no-secondary"]
    outs = []
    for name in ("a", "b"):
        r = _bench(*flags, "--dump-outputs", str(tmp_path / name))
        assert r.returncode == 0, r.stderr.decode()[-3000:]
        outs.append(json.loads([ln for ln in r.stdout.decode().splitlines() if ln.startswith("{")][-1]))
    out = outs[0]
    assert out["steps"] == 3 and out["ms_per_step"] > 0 and out["self_check"]["ok"]
    assert out["dump_outputs"]["pairs"] == 12 and not out["dump_outputs"]["sampled"]
    ok = np.load(tmp_path / "a" / "ok.npy")
    assert ok.shape == (12,) and int(ok.sum()) == out["config"]["pairs_ok_last_step"]
    assert np.load(tmp_path / "a" / "pose.npy").shape == (12, 16)
    for f in sorted(os.listdir(tmp_path / "a")):
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)), f


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_what_a_full_run_dumps(tmp_path):
    common = ["--steps", "3", "--warmup", "1", "--batch", "12", "--chunks", "2"]
    r = _bench(*common, "--dump-outputs", str(tmp_path / "plain"))
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    plain = json.loads([ln for ln in r.stdout.decode().splitlines() if ln.startswith("{")][-1])
    r = _bench(*common, "--full", "--cpu-pairs", "0", "--e2e-frames", "0", "--no-legs", "--no-secondary",
               "--dump-outputs", str(tmp_path / "full"))
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    full = json.loads([ln for ln in r.stdout.decode().splitlines() if ln.startswith("{")][-1])
    assert full["self_check"]["ok"] and full["self_check"]["pairs"] == 12
    for k in ("metric", "unit", "higher_is_better", "dtype", "steps", "warmup"):
        assert plain[k] == full[k], k
    assert plain["value"] > 0 and plain["ms_per_step"] > 0 and plain["roofline"]["frac"] > 0
    assert plain["cpu_baseline"] is None
    for k in ("self_check", "m1", "online", "stream", "lk_accum_sse2", "orb", "hd", "value_x86_order", "e2e", "e2e_full"):
        assert k not in plain, k
    assert sorted(os.listdir(tmp_path / "plain")) == sorted(os.listdir(tmp_path / "full"))
    for f in sorted(os.listdir(tmp_path / "plain")):
        assert np.array_equal(np.load(tmp_path / "plain" / f), np.load(tmp_path / "full" / f)), f
