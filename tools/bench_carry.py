#!/usr/bin/env python3
"""Track carry: what svo_set_track_carry costs per step and what it does to the tracks and the trajectory (bench.py stays the
one-line contract; nothing here is a pass bar).

At 1241x376 on the rendered corridor tools/trajectory_check.py uses, LK mode with lk_accum exact, frames resident in HBM, M
lockstep streams of one context through svo_streams_step (the live product path), one process run on one box:

  off / on at M = 1, 16, 128        every cv::FAST corner per frame / carried tracks + the detections that do not crowd them
  on + buckets 50x50 / 4 at M = 128 the carried tracks topped up from a bucketed detector

Stream s of a step reads frame fold(k + s) of the sequence (fold bounces between its ends, so consecutive frames of a stream
are always neighbours).  Per row: ms per step over at least one second of steps that ends in a synchronise; the `carry` stage
mark of svo_get_timing from a second, short run; list length (n_prev_kps), n_tracked and n_inliers of the last step; mean and
90th-percentile age-at-t1 of its tracks (on rows); and, from a 301-frame run of ONE stream, the relative-pose errors and the
end-point drift against the renderer's ground truth as tools/trajectory_check.py computes them.

Usage: python tools/bench_carry.py [--out profiles/carry_bench.json] [--frames 301]
The document goes to stdout and to --out; --merge FILE copies every key of FILE this tool does not write itself (the plain
bench.py runs of the parent commit, this commit and the parent again are recorded there by hand)."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

W, H = 1241, 376
CELL, PER_CELL = 50, 4
MIN_SECONDS = 1.0


def fold(i, n):
    """0, 1, .., n-1, n-2, .., 1, 0, 1, ..: a walk whose consecutive steps are neighbouring frames"""
    p = i % (2 * n - 2)
    return p if p < n else 2 * n - 2 - p


def trajectory(seq, L, R, ctx, n):
    recs = [ctx.streams_step([0], L[t:t + 1], R[t:t + 1])[0] for t in range(n)]
    res = np.array(recs[1:])
    ages = ctx.streams_track_ids(0)[1] if ctx.track_carry()[0] else None
    gt_wc = seq.poses_wc().numpy()
    te, re_ = [], []
    for t in range(1, n):
        if not res["ok"][t - 1]:
            continue
        Tg = seq.relative_gt(t).numpy()
        te.append(np.linalg.norm(res["tvec"][t - 1] - Tg[:3, 3]))
        dR = res["R"][t - 1].reshape(3, 3) @ Tg[:3, :3].T
        re_.append(np.degrees(np.arccos(np.clip((np.trace(dR) - 1) / 2, -1, 1))))
    est_end = res["pose"][-1].reshape(4, 4)
    gt_end = np.linalg.inv(gt_wc[0]) @ gt_wc[n - 1]
    path = float(np.sum(np.linalg.norm(np.diff(gt_wc[:n, :3, 3], axis=0), axis=1)))
    drift = float(np.linalg.norm(est_end[:3, 3] - gt_end[:3, 3]))
    out = {"frames": n, "pairs_ok": int(res["ok"].sum()), "pairs": n - 1,
           "rel_translation_err_m": {"mean": float(np.mean(te)), "max": float(np.max(te))},
           "rel_rotation_err_deg": {"mean": float(np.mean(re_)), "max": float(np.max(re_))},
           "path_length_m": path, "end_point_drift_m": drift, "drift_percent_of_path": 100 * drift / path,
           "mean_list_length": float(res["n_prev_kps"].mean()), "mean_n_tracked": float(res["n_tracked"].mean()),
           "mean_n_inliers": float(res["n_inliers"].mean())}
    if ages is not None:
        out["last_pair_track_age"] = {"mean": float(ages.mean()), "p90": float(np.percentile(ages, 90)), "max": int(ages.max())}
    return out


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "carry_bench.json"))
    ap.add_argument("--frames", type=int, default=301)
    ap.add_argument("--merge", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: the hot path has no CPU fallback")
    pkg = entry.load_package()
    synth = importlib.import_module(entry.PKG_NAME + ".synth")
    dev = torch.device("cuda", 0)
    n = args.frames
    seq = synth.StereoSequence(width=W, height=H, n_frames=n, seed=20200710, device=dev)
    L = torch.zeros((n, H, W), dtype=torch.uint8, device=dev)
    R = torch.zeros((n, H, W), dtype=torch.uint8, device=dev)
    for f in range(n):
        L[f], R[f] = seq.render(f)
    P1, P2 = seq.proj()
    stream = torch.cuda.current_stream()
    traj = {}

    def make_ctx(m, carry, buckets):
        c = pkg.Context(W, H, device=0, max_batch=max(2 * m - 1, 1), P1=P1, P2=P2)
        if buckets:
            c.set_fast_buckets(CELL, CELL, PER_CELL)
        if carry:
            c.set_track_carry(True, 3.0, 0)
        c.streams_create(m)
        return c

    def measure(m, carry, buckets=False):
        name = ("on" if carry else "off") + (f"_buckets_{CELL}x{CELL}_{PER_CELL}" if buckets else "")
        ctx = make_ctx(m, carry, buckets)
        ctx.set_stream(stream.cuda_stream)
        ids = np.arange(m, dtype=np.int32)
        bufs = [torch.zeros((m, pkg.STEP_DTYPE.itemsize), dtype=torch.uint8, device=dev) for _ in range(2)]
        idx = [torch.tensor([fold(k + s, n) for s in range(m)], device=dev) for k in range(2 * n - 2)]
        state = {"k": 0}

        def step():
            k = state["k"]
            i = idx[k % len(idx)]
            ctx.streams_step(ids, L[i], R[i], results=bufs[k & 1])
            state["k"] = k + 1

        def sync():
            ctx.sync()
            torch.cuda.synchronize()
        for _ in range(12):                                      # the lists of the on rows reach their steady length
            step()
        sync()
        t0 = time.perf_counter()
        for _ in range(3):
            step()
        sync()
        est = (time.perf_counter() - t0) / 3
        steps = max(8, int(np.ceil(1.2 * MIN_SECONDS / est)))
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        sync()
        dt = time.perf_counter() - t0
        ctx.enable_timing(True)
        ctx.get_timing()
        for _ in range(4):
            step()
        sync()
        stages = dict(ctx.get_timing())
        ctx.enable_timing(False)
        rec = np.frombuffer(bufs[(state["k"] - 1) & 1].cpu().numpy().tobytes(), dtype=pkg.STEP_DTYPE)
        row = {"config": name, "streams": m, "track_carry": bool(carry), "buckets": [CELL, CELL, PER_CELL] if buckets else None,
               "step_ms": dt / steps * 1e3, "frames_per_s": m * steps / dt, "steps_timed": steps, "seconds": dt,
               "carry_stage_ms": float(stages.get("carry", 0.0)), "lk_stage_ms": float(stages.get("lk", 0.0)),
               "fast_stage_ms": float(stages.get("fast", 0.0)), "scatter_stage_ms": float(stages.get("stream_scatter", 0.0)),
               "mean_list_length": float(rec["n_prev_kps"].mean()), "mean_n_tracked": float(rec["n_tracked"].mean()),
               "mean_n_inliers": float(rec["n_inliers"].mean()), "pairs_ok": int(rec["ok"].sum())}
        if carry:
            ages = np.concatenate([ctx.streams_track_ids(i)[1] for i in range(min(m, 4))])
            row["track_age"] = {"mean": float(ages.mean()), "p90": float(np.percentile(ages, 90)), "max": int(ages.max())}
        ctx.close()
        if name not in traj:                                     # one stream, frames 0 .. n-1 in order: the same for every M
            c1 = make_ctx(1, carry, buckets)
            traj[name] = trajectory(seq, L, R, c1, n)
            c1.close()
        row["trajectory"] = traj[name]
        print(json.dumps(row), file=sys.stderr, flush=True)
        return row

    rows = []
    for m in (1, 16, 128):
        rows.append(measure(m, False))
        rows.append(measure(m, True))
    rows.append(measure(128, True, buckets=True))
    rows.append(measure(128, False))                             # the run's own spread on the off row
    rows[-1]["config"] = "off_again"
    for r in rows:
        off = next(o for o in rows if o["streams"] == r["streams"] and o["config"] == "off")
        r["step_ms_vs_off"] = r["step_ms"] / off["step_ms"]
    doc = {"width": W, "height": H, "lk_accum": "exact", "frames": "HBM", "entry_point": "svo_streams_step", "min_distance": 3.0,
           "max_age": 0, "min_seconds": MIN_SECONDS, "device": torch.cuda.get_device_name(0), "rows": rows}
    if args.merge and os.path.exists(args.merge):
        with open(args.merge, encoding="utf-8") as f:
            for k, v in json.load(f).items():
                doc.setdefault(k, v)
    txt = json.dumps(doc, indent=1)
    with open(args.out, "w", encoding="utf-8") as f:
        f.write(txt + "\n")
    print(txt)


if __name__ == "__main__":
    main()
