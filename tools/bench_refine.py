#!/usr/bin/env python3
"""The pose refinement stage (svo_set_pose_refine) off and in its two modes (bench.py stays the one-line contract).

At 1241x376 on the rendered corridor tools/trajectory_check.py uses, frames resident in HBM, 256 pairs per svo_track_batch
step, overlap mode as in bench.py's headline, one process run on one box:

  lk_off / lk_on / lk_ba                          LK mode, lk_accum exact, every cv::FAST corner
  orb_off / orb_on / orb_ba                       ORB mode (it has no t2_right: one view at t2)
  lk_buckets_off / lk_buckets_on / lk_buckets_ba  LK mode with the 4 strongest FAST corners per 50 x 50 pixel cell
  lk_off_again                                    the first row once more: the run's own spread

_off: the stage off; _on: pose_refine reproj (the pose on both cameras' t2 observations, the triangulated points held fixed);
_ba: pose_refine ba (the two-frame stereo bundle adjustment: pose and points on the observations of both times).

Per row: ms per step and pairs/s over at least one second of steps that ends in a synchronise; the `pnp` and `refine` stages
of svo_get_timing from a second, short run WITHOUT overlap (in overlap mode the pose stage runs on the side stream, where no
stage marks are recorded); mean n_tracked and RANSAC n_inliers of a step and, with the stage on, the mean refined active count,
LM iterations and the share of pairs whose refined pose was applied; and, from a 301-frame run in batches of 100 as
tools/trajectory_check.py does, the relative-pose errors and the end-point drift against the renderer's ground truth.
No figure here is a pass bar.

Usage: python tools/bench_refine.py [--out profiles/refine_ba_bench.json] [--frames 301]
The rows and the default --out are not those of the earlier profiles/refine_bench.json (off / reproj rows only, written by this
tool before it had ba rows): that file is kept as the record of its run and is no longer what a default invocation regenerates.
The document goes to stdout and to --out; --merge FILE copies every key of FILE this tool does not write itself (the bench.py
runs against the parent commit are recorded there by hand)."""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import __graft_entry__ as entry  # noqa: E402
from bench_detectors import B, CELL, H, MIN_SECONDS, W, timed, trajectory  # noqa: E402


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refine_ba_bench.json"))
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

    def measure(name, refine, orb=False, per_cell=0):
        def make_ctx(max_batch):
            kw = dict(track_mode=pkg.MODE_ORB, min_move2=0.05 ** 2, max_move2=10.0 ** 2) if orb else {}
            c = pkg.Context(W, H, device=0, max_batch=max_batch, P1=P1, P2=P2, **kw)
            if per_cell:
                c.set_fast_buckets(CELL, CELL, per_cell)
            if refine != "off":
                c.set_pose_refine(refine)
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
        rec = np.frombuffer(bufs[1].cpu().numpy().tobytes(), dtype=pkg.STEP_DTYPE)
        stats = None
        if refine != "off":
            rr = [ctx.refine_result(p) for p in range(B)]
            stats = {"mean_n_active": float(np.mean([r["n_active"] for r in rr])), "mean_iters": float(np.mean([r["iters"] for r in rr])),
                     "applied_share": float(np.mean([r["status"] == pkg.REFINE_APPLIED for r in rr])),
                     "mean_points": float(np.mean([r["n_points"] for r in rr]))}
        # the pose stage's marks exist on the context's own stream only: a short run without overlap
        ctx.set_overlap(False)
        ctx.enable_timing(True)
        ctx.get_timing()
        for k in range(4):
            step(k)
        sync()
        stages = dict(ctx.get_timing())
        ctx.enable_timing(False)
        ctx.close()
        row = {"config": name, "mode": "orb" if orb else "lk", "pose_refine": refine,
               "cell": [CELL, CELL] if per_cell else None, "per_cell": per_cell,
               "step_ms": per * 1e3, "pairs_per_s": B / per, "steps_timed": steps, "seconds": dt,
               "pnp_stage_ms": float(stages.get("pnp", 0.0)), "refine_stage_ms": float(stages["refine"]) if "refine" in stages else None,
               "stages_ms_no_overlap": {k: float(v) for k, v in stages.items()},
               "mean_n_tracked": float(rec["n_tracked"].mean()), "mean_n_inliers": float(rec["n_inliers"].mean()),
               "pairs_ok": int(rec["ok"].sum()), "refine": stats,
               "trajectory": trajectory(pkg, seq, L, R, make_ctx, args.frames)}
        print(json.dumps(row), file=sys.stderr, flush=True)
        return row

    rows = []
    for base, kw in (("lk", {}), ("orb", dict(orb=True)), (f"lk_buckets_{CELL}x{CELL}_4", dict(per_cell=4))):
        rows += [measure(f"{base}_{tag}", mode, **kw) for tag, mode in (("off", "off"), ("on", "reproj"), ("ba", "ba"))]
    rows.append(measure("lk_off_again", "off"))
    doc = {"width": W, "height": H, "pairs_per_step": B, "lk_accum": "exact", "frames": "HBM", "overlap": True,
           "min_seconds": MIN_SECONDS, "device": torch.cuda.get_device_name(0),
           "pose_refine_settings": {"rounds": 4, "iters": 10, "sigma_px": 1.0, "min_inliers": 6}, "rows": rows}
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
