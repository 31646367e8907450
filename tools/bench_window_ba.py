#!/usr/bin/env python3
"""Times the sliding window's two stage kernels on one MI355X: svo_window_update and svo_window_ba on synthetic tables in device
memory (the scenes of tests/_window_cases.py: a camera advancing through a cloud of landmarks, 30 % outlier observations), for
window lengths W = 3, 5, 8 and two table sizes.  Every figure is the mean of single calls timed with HIP events on the
context's stream, at least one second of calls per figure; the table is restored before every call of the optimiser, which
works in place.  Writes profiles/window_ba_bench.json.  No figure is a pass bar.

--online: the fused path instead -- one chain of 301 frames at 1241 x 376 through svo_add_frame (frames in device memory), rows
carry off / carry on / carry + W = 3, 5, 8, each again with FAST buckets 50 x 50 / 4, the first row repeated last: ms per step
over the whole chain, the win_update / win_ba stage times, the last window's landmarks, observations, active share and LM
iterations, per-pair errors and end-point drift of the step records' `pose` against the renderer's truth.  The rows are merged
into the same file under "online_rows".

    python tools/bench_window_ba.py [--online] [--out profiles/window_ba_bench.json] [--seconds 1.0]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as entry  # noqa: E402


def online(args):
    import importlib
    import torch
    pkg = entry.load_package()
    synth = importlib.import_module(entry.PKG_NAME + ".synth")
    W, H, n = 1241, 376, args.frames
    dev = torch.device("cuda", 0)
    seq = synth.StereoSequence(width=W, height=H, n_frames=n, seed=20200710, device=dev)
    frames = [seq.render(f) for f in range(n)]
    P1, P2 = seq.proj()
    gt_wc = seq.poses_wc().numpy()
    doc = json.load(open(args.out)) if os.path.exists(args.out) else {}
    rows = []
    configs = [(False, 0, False), (True, 0, False), (True, 3, False), (True, 5, False), (False, 0, True), (True, 0, True), (True, 3, True),
               (True, 5, True), (True, 8, True), (True, 8, False), (False, 0, False)]
    for carry, win, buckets in configs:
        ctx = pkg.Context(W, H, device=0, P1=P1, P2=P2)
        if buckets:
            ctx.set_fast_buckets(50, 50, 4)
        if carry:
            ctx.set_track_carry(True, 3.0, 0)
        if win:
            ctx.set_window_ba(win, 4, 5, 1.0, 10)
        for L, R in frames[:3]:                                  # warm-up: first launches, allocations
            ctx.add_frame(L, R)
        ctx.reset()
        torch.cuda.synchronize()
        t0, recs, applied = time.perf_counter(), [], 0
        for L, R in frames:
            recs.append(ctx.add_frame(L, R)[1])
        dt = time.perf_counter() - t0
        last = ctx.window_result() if win else None
        res = np.array(recs[1:])
        te, re_ = [], []
        for t in range(1, n):
            if res["ok"][t - 1]:
                Tg = seq.relative_gt(t).numpy()
                te.append(np.linalg.norm(res["tvec"][t - 1] - Tg[:3, 3]))
                dR = res["R"][t - 1].reshape(3, 3) @ Tg[:3, :3].T
                re_.append(np.degrees(np.arccos(np.clip((np.trace(dR) - 1) / 2, -1, 1))))
        gt_end = np.linalg.inv(gt_wc[0]) @ gt_wc[n - 1]
        path = float(np.sum(np.linalg.norm(np.diff(gt_wc[:n, :3, 3], axis=0), axis=1)))
        drift = float(np.linalg.norm(res["pose"][-1].reshape(4, 4)[:3, 3] - gt_end[:3, 3]))
        ctx.enable_timing(True)
        ctx.get_timing()
        ctx.reset()
        for L, R in frames[:8]:
            ctx.add_frame(L, R)
        stages = dict(ctx.get_timing())
        row = dict(track_carry=carry, window=win, buckets=[50, 50, 4] if buckets else None, frames=n, pairs_ok=int(res["ok"].sum()),
                   ms_per_step=dt / n * 1e3, seconds=dt, win_update_ms=float(stages.get("win_update", 0.0)), win_ba_ms_first_8_frames=float(stages.get("win_ba", 0.0)),
                   rel_translation_err_mm=float(np.mean(te)) * 1e3, rel_rotation_err_deg=float(np.mean(re_)), path_length_m=path,
                   end_point_drift_m=drift, drift_percent_of_path=100 * drift / path, mean_list_length=float(res["n_prev_kps"].mean()))
        if last:
            row.update(last_status=int(last["status"]), landmarks=int(last["n_landmarks"]), usable=int(last["n_usable"]), observations=int(last["n_obs"]),
                       active_share=float(last["n_active"]) / max(int(last["n_obs"]), 1), lm_iterations=int(last["iters"]))
        ctx.close()
        rows.append(row)
        print(json.dumps(row), flush=True)
        doc["online_rows"] = rows
        doc["online_note"] = ("one chain through svo_add_frame, frames in HBM, 1241x376, rounds x iters 4 x 5, sigma 1, min_obs 10; ms per step is wall "
                              "time over the whole chain; drift is that of the step records' pose (the filtered pose)")
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--online", action="store_true")
    ap.add_argument("--frames", type=int, default=301)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "window_ba_bench.json"))
    ap.add_argument("--seconds", type=float, default=1.0)
    args = ap.parse_args()
    if args.online:
        return online(args)
    import torch
    import _window_cases as WC
    import _window_ref as WR
    pkg = entry.load_package()
    from importlib import import_module
    B = import_module(entry.PKG_NAME + ".binding")
    ctx = pkg.Context(64, 64, device=0)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    rows = []
    for W in (3, 5, 8):
        for m in (1000, 4000):
            tab, _ = WC.scene(seed=1, n=W, m=m, holes=True, outliers=0.3)
            t = {k: dev(tab[k]) for k in ("ids", "X", "obs_left", "obs_right", "poses")}
            t["seen"], t["active"] = dev(tab["seen"].view(np.int32)), dev(tab["active"].view(np.int32))
            t["counts"] = dev(np.array([W, m, 0, 0], np.int32))
            keep = {k: t[k].clone() for k in ("X", "poses", "active")}
            for rounds, iters in ((4, 2), (4, 5)):
                ms, raw, t0 = [], None, time.time()
                while time.time() - t0 < args.seconds or len(ms) < 5:
                    for k, v in keep.items():
                        t[k].copy_(v)
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    raw, _ = ctx.window_solve(t, WC.P1, WC.P2, rounds=rounds, iters=iters, sigma_px=1.0, min_obs=10)
                    b.record()
                    b.synchronize()
                    ms.append(a.elapsed_time(b))
                r = B.WindowResult.from_buffer_copy(raw.cpu().numpy().tobytes()).as_dict()
                rows.append(dict(kernel="window_ba", frames=W, landmarks=m, rounds=rounds, iters=iters, calls=len(ms),
                                 ms_mean=float(np.mean(ms[1:])), ms_min=float(np.min(ms)), status=int(r["status"]), lm_iterations=int(r["iters"]),
                                 usable=int(r["n_usable"]), observations=int(r["n_obs"]), active_share=float(r["n_active"]) / max(int(r["n_obs"]), 1)))
                print(rows[-1], flush=True)
            # the update: a full window slides and takes a pair of m / 3 tracks, half of them new
            full, _, step, _ = WC._sized(7, W, m, max(m // 3, 2))
            p = step["pair"]
            args_dev = [dev(p[k]) for k in ("t1_left", "t1_right", "t2_left", "t2_right", "ids", "tri")] + [dev(step["pose_a"]), dev(step["pose_b"])]
            tin = {k: dev(full[k]) for k in ("ids", "X", "obs_left", "obs_right", "poses")}
            tin["seen"], tin["active"] = dev(full["seen"].view(np.int32)), dev(full["active"].view(np.int32))
            tin["counts"] = dev(np.array([W, m, 0, 0], np.int32))
            ms, t0 = [], time.time()
            while time.time() - t0 < args.seconds or len(ms) < 5:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                out = ctx.window_update(tin, W, *args_dev, cap=2 * m)
                b.record()
                b.synchronize()
                ms.append(a.elapsed_time(b))
            rows.append(dict(kernel="window_update", frames=W, rows_in=m, tracks=len(p["ids"]), rows_out=int(out["counts"][1]), calls=len(ms),
                             ms_mean=float(np.mean(ms[1:])), ms_min=float(np.min(ms))))
            print(rows[-1], flush=True)
    ctx.close()
    doc = json.load(open(args.out)) if os.path.exists(args.out) else {}
    doc.update(tool="tools/bench_window_ba.py", device=torch.cuda.get_device_name(0),
               note="single stage calls on device tables, HIP events on the context's stream; the event pair also spans the binding's "
                    "allocation of the output tensors (window_update) and of the result buffer (window_ba)", rows=rows)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
