#!/usr/bin/env python3
"""Stream sets: aggregate throughput of M lockstep live streams through svo_streams_step (bench.py stays the one-line contract).

At 1241x376 on the synthetic sequence bench.py uses, frames resident in HBM, for M = 1 .. 128 streams, LK (lk_accum exact)
and ORB: aggregate pairs/s and ms per step after two warm-up steps, timed over at least one second of steps that ends in a
synchronise, next to two baselines taken in the same process run:

  (a) add_frame    M one-stream contexts stepped one after the other with svo_add_frame (what a user does without a stream
                   set; M <= 16);
  (b) track_batch  svo_track_batch with n_pairs = M on one context: the same pair work with affine addressing and no
                   gather / scatter -- the ceiling.  Repeated five times at the largest M for the run-to-run spread.

Stream s plays the sequence from frame s, forwards then backwards, so every pair is a pair of neighbouring frames.  For
M <= 16 each stream's pose after a fixed number of steps is compared with baseline (a)'s, byte for byte.

Usage: python tools/bench_streams.py [--out profiles/streams_bench.json] [--modes lk,orb] [--streams 1,2,4,...]
       python tools/bench_streams.py --trace M --modes lk      (a short run of M-stream steps only, for a kernel trace)
One JSON document on stdout and in --out."""
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

W, H, PITCH = 1241, 376, 1280
T = 9                                   # rendered frames; a stream walks 0 .. T-1 .. 0
MAX_BATCH = 256                         # bench.py's value: up to 128 streams a step
MIN_SECONDS = 1.0


def tri(k):
    p = 2 * (T - 1)
    k %= p
    return k if k < T else p - k


def timed(torch, step, sync, n_warm=2):
    """Seconds per call of step(k): two warm-up calls, a short calibration, then >= MIN_SECONDS of calls ending in a sync."""
    for k in range(n_warm):
        step(k)
    sync()
    t0 = time.perf_counter()
    for k in range(4):
        step(n_warm + k)
    sync()
    est = (time.perf_counter() - t0) / 4
    n = max(8, int(np.ceil(1.2 * MIN_SECONDS / est)))
    k0 = n_warm + 4
    t0 = time.perf_counter()
    for k in range(n):
        step(k0 + k)
    sync()
    dt = time.perf_counter() - t0
    assert dt >= MIN_SECONDS or n >= 8, (dt, n)
    return dt / n, n, dt


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "streams_bench.json"))
    ap.add_argument("--modes", default="lk,orb")
    ap.add_argument("--streams", default="1,2,4,8,16,32,64,128")
    ap.add_argument("--trace", type=int, default=0, help="only run 20 steps of this many streams (for rocprofv3 --kernel-trace)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: the hot path has no CPU fallback")
    pkg = entry.load_package()
    synth = importlib.import_module(entry.PKG_NAME + ".synth")
    mg = importlib.import_module(entry.PKG_NAME + ".multigpu")
    dev = torch.device("cuda", 0)
    seq = synth.StereoSequence(width=W, height=H, n_frames=T, seed=mg.sequence_seed(0, 1), device=dev)
    L = torch.zeros((T, H, PITCH), dtype=torch.uint8, device=dev)
    R = torch.zeros((T, H, PITCH), dtype=torch.uint8, device=dev)
    for f in range(T):
        l, r = seq.render(f)
        L[f, :, :W] = l
        R[f, :, :W] = r
    P1, P2 = seq.proj()
    stream = torch.cuda.current_stream()
    period = 2 * (T - 1)
    Ms = [args.trace] if args.trace else [int(x) for x in args.streams.split(",")]
    doc = {"width": W, "height": H, "max_batch": MAX_BATCH, "frames": "HBM", "min_seconds": MIN_SECONDS,
           "device": torch.cuda.get_device_name(0), "modes": {}}
    for mode in args.modes.split(","):
        kw = dict(P1=P1, P2=P2)
        if mode == "orb":
            kw.update(track_mode=pkg.MODE_ORB, min_move2=0.05 ** 2, max_move2=10.0 ** 2)
        ctx = pkg.Context(W, H, device=0, max_batch=MAX_BATCH, **kw)
        ctx.set_stream(stream.cuda_stream)
        ctx.streams_create(max(Ms))
        res_dev = torch.zeros((MAX_BATCH, pkg.STEP_DTYPE.itemsize), dtype=torch.uint8, device=dev)
        rows = []
        for M in Ms:
            ids = np.arange(M, dtype=np.int32)
            # the stacked frames of every step of one period, built before anything is timed
            idx = [torch.tensor([tri(s + k) for s in range(M)], device=dev) for k in range(period)]
            Ls = [L[i][:, :, :W] for i in idx]
            Rs = [R[i][:, :, :W] for i in idx]
            ctx.streams_reset(-1)

            def step(k, Ls=Ls, Rs=Rs, ids=ids):
                ctx.streams_step(ids, Ls[k % period], Rs[k % period], results=res_dev)
            if args.trace:
                for k in range(20):
                    step(k)
                ctx.sync()
                rec = np.frombuffer(res_dev[:M].cpu().numpy().tobytes(), dtype=pkg.STEP_DTYPE)
                print(json.dumps({"mode": mode, "streams": M, "steps": 20, "ok": int(rec["ok"].sum())}))
                continue
            per, n, dt = timed(torch, step, ctx.sync)
            rec = np.frombuffer(res_dev[:M].cpu().numpy().tobytes(), dtype=pkg.STEP_DTYPE)
            row = {"streams": M, "step_ms": per * 1e3, "pairs_per_s": M / per, "steps_timed": n, "seconds": dt,
                   "ok_last_step": int(rec["ok"].sum())}
            # (b) the same pair work as one batch: frames tri(0) .. tri(M)
            bidx = torch.tensor([tri(k) for k in range(M + 1)], device=dev)
            Lb, Rb = L[bidx][:, :, :W], R[bidx][:, :, :W]
            reps = 5 if M == max(Ms) else 1
            b_ms = []
            for _ in range(reps):
                per_b, _, _ = timed(torch, lambda k: ctx.track_batch(Lb, Rb, results=res_dev), ctx.sync)
                b_ms.append(per_b * 1e3)
            row["track_batch_ms"] = float(np.median(b_ms))
            row["track_batch_pairs_per_s"] = M / (row["track_batch_ms"] * 1e-3)
            if reps > 1:
                row["track_batch_ms_repeats"] = b_ms
                row["track_batch_spread"] = (max(b_ms) - min(b_ms)) / float(np.median(b_ms))
            row["vs_track_batch"] = row["step_ms"] / row["track_batch_ms"]
            # (a) M one-stream contexts, one add_frame each per step; and the byte-for-byte pose check
            if M <= 16:
                solo = [pkg.Context(W, H, device=0, max_batch=1, **kw) for _ in range(M)]
                for c in solo:
                    c.set_stream(stream.cuda_stream)

                def step_a(k):
                    for s, c in enumerate(solo):
                        f = tri(s + k)
                        c.add_frame(L[f, :, :W], R[f, :, :W])
                per_a, _, _ = timed(torch, step_a, lambda: None)
                row["add_frame_ms"] = per_a * 1e3
                row["add_frame_pairs_per_s"] = M / per_a
                n_cmp = 7
                ctx.streams_reset(-1)
                for c in solo:
                    c.reset()
                for k in range(n_cmp):
                    step(k)
                    step_a(k)
                same = all(np.array_equal(ctx.streams_get_pose(s), solo[s].get_pose()) for s in range(M))
                moved = all(not np.array_equal(solo[s].get_pose(), np.eye(4)) for s in range(M))
                row["poses_equal_add_frame"] = bool(same and moved)
                assert same and moved, f"{mode} M={M}: stream poses differ from the one-stream contexts'"
                for c in solo:
                    c.close()
            rows.append(row)
            print(json.dumps({"mode": mode, **row}), file=sys.stderr, flush=True)
        ctx.close()
        doc["modes"][mode] = rows
    if args.trace:
        return
    txt = json.dumps(doc, indent=1)
    with open(args.out, "w", encoding="utf-8") as f:
        f.write(txt + "\n")
    print(txt)


if __name__ == "__main__":
    main()
