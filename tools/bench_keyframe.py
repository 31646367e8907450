#!/usr/bin/env python3
"""Measures keyframe mode (svo_set_keyframe) on one MI355X: one process, one chain of 301 frames at 1241 x 376 through
svo_add_frame (LK `exact`, frames in device memory).  Rows: carry off / carry on / carry + keyframe with min_tracks 60 at
max_gap 0, 5, 10 / the same three with FAST buckets 50 x 50 / 4 / carry off again, last.  Per row: ms per step over the whole
chain (wall time), the kf_join / kf_pnp / kf_update stage times, keyframes taken, mean and maximum gap of a solve, mean n_join,
the share of steps APPLIED, per-pair translation and rotation error and the end-point drift of the step records' `pose`
against the renderer's truth (as tools/trajectory_check.py measures them).  Writes profiles/keyframe_bench.json.  No figure is
a pass bar.

    python tools/bench_keyframe.py [--frames 301] [--out profiles/keyframe_bench.json]"""
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

MIN_TRACKS = 60


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=301)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "keyframe_bench.json"))
    args = ap.parse_args()
    import torch
    pkg = entry.load_package()
    synth = importlib.import_module(entry.PKG_NAME + ".synth")
    W, H, n = 1241, 376, args.frames
    dev = torch.device("cuda", 0)
    seq = synth.StereoSequence(width=W, height=H, n_frames=n, seed=20200710, device=dev)
    frames = [seq.render(f) for f in range(n)]
    P1, P2 = seq.proj()
    gt_wc = seq.poses_wc().numpy()
    gt_end = np.linalg.inv(gt_wc[0]) @ gt_wc[n - 1]
    path = float(np.sum(np.linalg.norm(np.diff(gt_wc[:n, :3, 3], axis=0), axis=1)))
    # (carry, keyframe max_gap or None, buckets)
    configs = [(False, None, False), (True, None, False), (True, 0, False), (True, 5, False), (True, 10, False),
               (True, 0, True), (True, 5, True), (True, 10, True), (False, None, False)]
    rows = []
    for carry, gap, buckets in configs:
        ctx = pkg.Context(W, H, device=0, P1=P1, P2=P2, max_batch=2)
        if buckets:
            ctx.set_fast_buckets(50, 50, 4)
        if carry:
            ctx.set_track_carry(True, 3.0, 0)
        if gap is not None:
            ctx.set_keyframe(True, MIN_TRACKS, gap)
        for L, R in frames[:3]:                                  # warm-up: first launches, allocations
            ctx.add_frame(L, R)
        ctx.reset()
        torch.cuda.synchronize()
        t0, recs = time.perf_counter(), []
        for L, R in frames:
            recs.append(ctx.add_frame(L, R)[1])
        dt = time.perf_counter() - t0
        res = np.array(recs[1:])
        # a second pass for what the timed one must not pay for: the per-step keyframe records and the stage times
        kf = []
        if gap is not None:
            ctx.reset()
            for t, (L, R) in enumerate(frames):
                ctx.add_frame(L, R)
                if t:
                    kf.append(ctx.keyframe_result())
        ctx.enable_timing(True)
        ctx.get_timing()
        ctx.reset()
        for L, R in frames[:16]:
            ctx.add_frame(L, R)
        stages = dict(ctx.get_timing())
        te, re_ = [], []
        for t in range(1, n):
            if res["ok"][t - 1]:
                Tg = seq.relative_gt(t).numpy()
                te.append(np.linalg.norm(res["tvec"][t - 1] - Tg[:3, 3]))
                dR = res["R"][t - 1].reshape(3, 3) @ Tg[:3, :3].T
                re_.append(np.degrees(np.arccos(np.clip((np.trace(dR) - 1) / 2, -1, 1))))
        drift = float(np.linalg.norm(res["pose"][-1].reshape(4, 4)[:3, 3] - gt_end[:3, 3]))
        row = dict(track_carry=carry, keyframe=gap is not None, min_tracks=MIN_TRACKS if gap is not None else None, max_gap=gap,
                   buckets=[50, 50, 4] if buckets else None, frames=n, pairs_ok=int(res["ok"].sum()), ms_per_step=dt / n * 1e3, seconds=dt,
                   kf_join_ms=float(stages.get("kf_join", 0.0)), kf_pnp_ms=float(stages.get("kf_pnp", 0.0)), kf_update_ms=float(stages.get("kf_update", 0.0)),
                   rel_translation_err_mm=float(np.mean(te)) * 1e3, rel_rotation_err_deg=float(np.mean(re_)), path_length_m=path,
                   end_point_drift_m=drift, drift_percent_of_path=100 * drift / path, mean_list_length=float(res["n_prev_kps"].mean()))
        if kf:
            solved = [k for k in kf if k["status"] in (pkg.KF_APPLIED, pkg.KF_REJECTED, pkg.KF_PAIR_FAILED)]
            row.update(keyframes_taken=int(sum(k["switched"] for k in kf)), mean_gap=float(np.mean([k["gap"] for k in solved])) if solved else 0.0,
                       max_gap_seen=int(max([k["gap"] for k in solved], default=0)), mean_n_join=float(np.mean([k["n_join"] for k in solved])) if solved else 0.0,
                       applied_share=float(np.mean([k["status"] == pkg.KF_APPLIED for k in kf])),
                       status_counts={name: int(sum(k["status"] == getattr(pkg, "KF_" + name) for k in kf))
                                      for name in ("NONE", "SHORT", "PAIR_FAILED", "REJECTED", "APPLIED")})
        ctx.close()
        rows.append(row)
        print(json.dumps(row), flush=True)
        doc = dict(tool="tools/bench_keyframe.py", device=torch.cuda.get_device_name(0),
                   note="one chain through svo_add_frame, frames in HBM, 1241x376, LK exact, max_batch 2 on every row; ms per step is wall time "
                        "over the whole chain; the kf_* stage times are means over the first 16 frames with timing marks on; the keyframe "
                        "columns come from a second, untimed pass; drift is that of the step records' pose",
                   rows=rows)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
