#!/usr/bin/env python3
"""The two ORB-mode matchers (svo_set_orb_matcher) side by side (bench.py stays the one-line contract).

At 1241x376 on the rendered corridor tools/trajectory_check.py uses, frames resident in HBM, 256 pairs per svo_track_batch
step, ORB mode, overlap mode as in bench.py's headline, one process run on one box:

  brute               the reference's global brute-force matcher (the default)
  guided_r0           the guided matcher, temporal search over the whole image
  guided_r64          ... with a 64-pixel temporal window
  guided_r0_refine    guided_r0 + pose_refine: reproj
  brute_again         the first row once more: the run's own spread

Per row: ms per step and pairs/s over at least one second of steps that ends in a synchronise; the `orb_stereo`, `orb_match`,
`pnp` (and `refine`) stages of svo_get_timing from a second, short run WITHOUT overlap (in overlap mode the pose stage runs on
the side stream, where no stage marks are recorded); mean RANSAC iterations, n_tracked and n_inliers of a step; and, from a
301-frame run in batches of 100 as tools/trajectory_check.py does, the relative-pose errors and the end-point drift against the
renderer's ground truth.  No figure here is a pass bar.

Usage: python tools/bench_orb_matcher.py [--out profiles/orb_matcher_bench.json] [--frames 301]
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
from bench_detectors import B, H, MIN_SECONDS, W, timed, trajectory  # noqa: E402


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "orb_matcher_bench.json"))
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

    def measure(name, guided, radius=0.0, refine=False):
        def make_ctx(max_batch):
            c = pkg.Context(W, H, device=0, max_batch=max_batch, P1=P1, P2=P2, track_mode=pkg.MODE_ORB, min_move2=0.05 ** 2,
                            max_move2=10.0 ** 2)
            if guided:
                c.set_orb_matcher("guided", radius=radius)
            if refine:
                c.set_pose_refine("reproj")
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
        # the stage marks exist on the context's own stream only: a short run without overlap
        ctx.set_overlap(False)
        ctx.enable_timing(True)
        ctx.get_timing()
        for k in range(4):
            step(k)
        sync()
        stages = dict(ctx.get_timing())
        ctx.enable_timing(False)
        ctx.close()
        row = {"config": name, "orb_matcher": "guided" if guided else "brute", "radius": radius, "pose_refine": "reproj" if refine else "off",
               "step_ms": per * 1e3, "pairs_per_s": B / per, "steps_timed": steps, "seconds": dt,
               "orb_stereo_stage_ms": float(stages["orb_stereo"]) if "orb_stereo" in stages else None,
               "orb_match_stage_ms": float(stages.get("orb_match", 0.0)), "pnp_stage_ms": float(stages.get("pnp", 0.0)),
               "refine_stage_ms": float(stages["refine"]) if "refine" in stages else None,
               "stages_ms_no_overlap": {k: float(v) for k, v in stages.items()},
               "mean_ransac_iters": float(rec["ransac_iters"].mean()),
               "mean_n_tracked": float(rec["n_tracked"].mean()), "mean_n_inliers": float(rec["n_inliers"].mean()),
               "pairs_ok": int(rec["ok"].sum()),
               "trajectory": trajectory(pkg, seq, L, R, make_ctx, args.frames)}
        print(json.dumps(row), file=sys.stderr, flush=True)
        return row

    rows = [measure("brute", False), measure("guided_r0", True), measure("guided_r64", True, radius=64.0),
            measure("guided_r0_refine", True, refine=True), measure("brute_again", False)]
    doc = {"width": W, "height": H, "pairs_per_step": B, "mode": "orb", "frames": "HBM", "overlap": True,
           "min_seconds": MIN_SECONDS, "device": torch.cuda.get_device_name(0),
           "orb_matcher_settings": {"th_stereo": 75, "th_track": 100, "ratio": 0.9, "max_disparity": "P1[0]"}, "rows": rows}
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
