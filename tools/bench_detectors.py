#!/usr/bin/env python3
"""Detectors of the LK step: cv::FAST, its two selections, and Shi-Tomasi (bench.py stays the one-line contract).

At 1241x376 on the rendered corridor tools/trajectory_check.py uses, LK mode with lk_accum exact, frames resident in HBM,
256 pairs per svo_track_batch step, overlap mode as in bench.py's headline, one process run on one box:

  fast                cv::FAST, every corner (the default)
  buckets 50x50 / 4   the 4 strongest FAST corners per 50 x 50 pixel cell (svo_set_fast_buckets)
  keep_strongest 500  svo_config.fast_keep_strongest = 500: the global top-N
  gftt 500/0.01/20    cv::goodFeaturesToTrack with the reference's literals (svo_set_lk_detector)
  fast_again          the first row once more: the run's own spread

Per row: ms per step and pairs/s over at least one second of steps that ends in a synchronise; the stages of svo_get_timing
from a second, short run with stage marks (the detector stage is `fast` -- detection + selection --; with GFTT it is
`gftt_eigen` + `gftt_emit` + `fast`, where `fast` is then the sort-and-select kernel alone); mean
kept corners, n_tracked and n_inliers of a step; and, from a 301-frame run in batches of 100 as tools/trajectory_check.py does,
the relative-pose errors and the end-point drift against the renderer's ground truth.  No figure here is a pass bar.

Usage: python tools/bench_detectors.py [--out profiles/gftt_bench.json] [--frames 301]
The document goes to stdout and to --out; --merge FILE copies every key of FILE this tool does not write itself (the
bench.py runs against the parent commit are recorded there by hand)."""
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
B = 256
CELL = 50
GFTT = (500, 0.01, 20.0)
MIN_SECONDS = 1.0


def timed(step, sync, n_warm=2):
    for k in range(n_warm):
        step(k)
    sync()
    t0 = time.perf_counter()
    for k in range(3):
        step(k)
    sync()
    est = (time.perf_counter() - t0) / 3
    n = max(8, int(np.ceil(1.2 * MIN_SECONDS / est)))
    t0 = time.perf_counter()
    for k in range(n):
        step(k)
    sync()
    dt = time.perf_counter() - t0
    return dt / n, n, dt


def trajectory(pkg, seq, L, R, make_ctx, n, batch=100):
    c = make_ctx(batch)
    pose, recs = np.eye(4), []
    for f0 in range(0, n - 1, batch):
        f1 = min(f0 + batch, n - 1)
        r = c.track_batch(L[f0:f1 + 1], R[f0:f1 + 1], pose0=pose)
        recs.append(r)
        pose = r["pose"][-1].reshape(4, 4)
    res = np.concatenate(recs)
    c.close()
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
    path = float(np.sum(np.linalg.norm(np.diff(gt_wc[:, :3, 3], axis=0), axis=1)))
    drift = float(np.linalg.norm(est_end[:3, 3] - gt_end[:3, 3]))
    return {"frames": n, "pairs_ok": int(res["ok"].sum()), "pairs": n - 1,
            "rel_translation_err_m": {"mean": float(np.mean(te)), "max": float(np.max(te))},
            "rel_rotation_err_deg": {"mean": float(np.mean(re_)), "max": float(np.max(re_))},
            "path_length_m": path, "end_point_drift_m": drift, "drift_percent_of_path": 100 * drift / path}


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gftt_bench.json"))
    ap.add_argument("--frames", type=int, default=301)
    ap.add_argument("--merge", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: the hot path has no CPU fallback")
    pkg = entry.load_package()
    synth = importlib.import_module(entry.PKG_NAME + ".synth")
    dev = torch.device("cuda", 0)
    n = max(args.frames, B + 1)
    seq = synth.StereoSequence(width=W, height=H, n_frames=n, seed=20200710, device=dev)
    L = torch.zeros((n, H, W), dtype=torch.uint8, device=dev)
    R = torch.zeros((n, H, W), dtype=torch.uint8, device=dev)
    for f in range(n):
        L[f], R[f] = seq.render(f)
    P1, P2 = seq.proj()
    stream = torch.cuda.current_stream()
    bufs = [torch.zeros((B, pkg.STEP_DTYPE.itemsize), dtype=torch.uint8, device=dev) for _ in range(2)]

    def measure(name, per_cell=0, keep=0, gftt=None):
        def make_ctx(max_batch):
            c = pkg.Context(W, H, device=0, max_batch=max_batch, P1=P1, P2=P2, fast_keep_strongest=keep)
            if per_cell:
                c.set_fast_buckets(CELL, CELL, per_cell)
            if gftt:
                c.set_lk_detector("gftt", *gftt)
            return c
        ctx = make_ctx(B)
        ctx.set_stream(stream.cuda_stream)
        ctx.set_overlap(True)

        def step(k):
            ctx.track_batch(L[:B + 1], R[:B + 1], results=bufs[k & 1])

        def sync():
            ctx.sync()
            torch.cuda.synchronize()
        per, steps, dt = timed(step, sync)
        ctx.enable_timing(True)
        ctx.get_timing()
        for k in range(4):
            step(k)
        sync()
        stages = dict(ctx.get_timing())
        ctx.enable_timing(False)
        rec = np.frombuffer(bufs[1].cpu().numpy().tobytes(), dtype=pkg.STEP_DTYPE)
        ctx.close()
        row = {"config": name, "cell": [CELL, CELL] if per_cell else None, "per_cell": per_cell, "fast_keep_strongest": keep,
               "gftt": list(gftt) if gftt else None,
               "step_ms": per * 1e3, "pairs_per_s": B / per, "steps_timed": steps, "seconds": dt,
               "detector_stage_ms": float(sum(stages.get(k, 0.0) for k in ("fast", "gftt_eigen", "gftt_emit"))), "stages_ms": {k: float(v) for k, v in stages.items()},
               "mean_kept_corners": float(rec["n_prev_kps"].mean()), "mean_n_tracked": float(rec["n_tracked"].mean()),
               "mean_n_inliers": float(rec["n_inliers"].mean()), "pairs_ok": int(rec["ok"].sum()),
               "trajectory": trajectory(pkg, seq, L, R, make_ctx, args.frames)}
        print(json.dumps(row), file=sys.stderr, flush=True)
        return row

    rows = [measure("fast"),
            measure(f"buckets_{CELL}x{CELL}_4", per_cell=4),
            measure("keep_strongest_500", keep=500),
            measure("gftt_500_0.01_20", gftt=GFTT),
            measure("fast_again")]
    off = rows[0]
    for r in rows:
        r["step_ms_vs_fast"] = r["step_ms"] / off["step_ms"]
    doc = {"width": W, "height": H, "pairs_per_step": B, "lk_accum": "exact", "frames": "HBM", "overlap": True,
           "min_seconds": MIN_SECONDS, "device": torch.cuda.get_device_name(0), "rows": rows}
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
