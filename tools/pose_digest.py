#!/usr/bin/env python3
"""SHA-256 digests of everything the three pose optimisers and the tail of the pose stage write, for byte-for-byte comparisons
between two builds of the library (a refactor of refine.hip / ba.hip / window.hip / pose_chain.hip must not move one bit).  No figure here is a pass bar: run the tool at
both commits and compare the lists.

Cases (the builders the GPU tests use: tests/_refine_cases.py, tests/_ba_cases.py, tests/_window_cases.py):
  refine_pose   one and two views, n = 0, 1, 255, 256, 257, 2500 points, HOST and DEVICE memory, three kinds of scene, sigma 0.5,
                the lambda exit and the unprojectable-point rejection
  refine_ba     three and four views, the same
  window        svo_window_update on every update case (2 .. 8 frames, up to 2049 rows), svo_window_ba on every optimiser scene
                (2 .. 8 frames, up to 2049 landmarks), and the optimiser on updated tables of 2, 3 and 8 frames
  fused         svo_add_frame over the 9 frames of tests/test_gpu_window.py plus one blank frame (a failed pair: the SKIPPED
                record), in reproj mode, in ba mode, and with track carry and the window at W = 3
  chain         the tail of the pose stage (pose_chain.hip, keyframe.hip): svo_track_batch's records over the same ten frames with
                and without pose0; svo_streams_step's records and svo_streams_get_pose for 3 streams over 3 steps, one reset and
                one seeded with svo_streams_set_pose in between; svo_chain_relative on tests/_pose_ref.py's chain_cases(), HOST
                and DEVICE; the fused keyframe chain at max_gap 0 and 2 (result, matches, table, records)
Per case: one digest over the raw bytes of every output (record, flags, points, table, step records).

    python tools/pose_digest.py [--out digests.json]"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as entry  # noqa: E402

POINT_COUNTS = (0, 1, 255, 256, 257, 2500)


def feed(h, v):
    """Every output in a fixed order: dicts by sorted key, arrays as their bytes, scalars as 8-byte numbers."""
    if isinstance(v, dict):
        for k in sorted(v):
            h.update(k.encode())
            feed(h, v[k])
    elif isinstance(v, (list, tuple)):
        for x in v:
            feed(h, x)
    elif v is None:
        h.update(b"none")
    elif isinstance(v, (bytes, str)):
        h.update(v if isinstance(v, bytes) else v.encode())
    elif isinstance(v, (bool, int, np.integer)):
        h.update(np.int64(v).tobytes())
    elif isinstance(v, (float, np.floating)):
        h.update(np.float64(v).tobytes())
    else:
        a = np.ascontiguousarray(v)
        h.update(str((a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())


def digest(*outputs):
    h = hashlib.sha256()
    feed(h, outputs)
    return h.hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import importlib
    import torch
    import _ba_cases as BC
    import _pose_ref as PR
    import _refine_cases as RC
    import _refine_ref as RR
    import _window_cases as WC
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: the hot path has no CPU fallback")
    pkg = entry.load_package()
    B = importlib.import_module(entry.PKG_NAME + ".binding")
    synth = importlib.import_module(entry.PKG_NAME + ".synth")
    out = {}

    def put(name, *outputs):
        assert name not in out, name
        out[name] = digest(*outputs)
        print(name, out[name], flush=True)

    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()

    # ---- the two-frame stage calls
    def rf_call(ctx, c, d, device):
        a = [c["X"], c["xl"], c["xr"] if d == 4 else None]
        return ctx.refine_pose(*([dev(x) for x in a] if device else a), c["P1"], c["P2"], c["rvec0"], c["t0"])

    def ba_call(ctx, c, d, device):
        a = [c["X0"], c["x1l"], c["x1r"], c["xl"], c["xr"] if d == 8 else None]
        return ctx.refine_ba(*([dev(x) for x in a] if device else a), c["P1"], c["P2"], c["rvec0"], c["t0"])

    ctx = pkg.Context(416, 128, device=0, max_keypoints=4096)
    for mode, call, make, views, kw in (("refine_pose", rf_call, RC.make_case, (2, 4), dict(rounds=RC.ROUNDS, iters=RC.ITERS)),
                                        ("refine_ba", ba_call, BC.make_case, (6, 8), dict(rounds=BC.ROUNDS, iters=BC.ITERS))):
        for d in views:
            for n in POINT_COUNTS:
                for kind in RC.KINDS:
                    if n == 0 and kind != "outliers":
                        continue
                    c = make("R0" if kind != "some_behind" else "R3", n, kind, RC.SEED0 + d)
                    ctx.set_pose_refine("off", **kw)
                    for device in (False, True):
                        put("%s d=%d n=%d %s %s" % (mode, d, n, kind, "device" if device else "host"), call(ctx, c, d, device))
            c = make("R2", 257, "outliers", RC.SEED0 + 7)
            ctx.set_pose_refine("off")                                      # the default settings: 4 x 10
            put("%s d=%d n=257 R2 defaults" % (mode, d), call(ctx, c, d, False))
            ctx.set_pose_refine("off", sigma_px=0.5, min_inliers=200, **kw)
            put("%s d=%d n=257 R2 sigma 0.5 min_inliers 200" % (mode, d), call(ctx, c, d, False))
            lam = (RC if mode == "refine_pose" else BC).lambda_case()
            ctx.set_pose_refine("off", rounds=2, iters=16)
            put("%s d=%d lambda exit" % (mode, d), call(ctx, lam, d, False))
            near = (RC if mode == "refine_pose" else BC).near_case(d)
            ctx.set_pose_refine("off", rounds=1, iters=6)
            put("%s d=%d unprojectable" % (mode, d), call(ctx, near, d, False))
    ctx.set_pose_refine("off")
    ctx.close()

    # ---- the window's stage calls
    ctx = pkg.Context(64, 64, device=0)

    def update(tab, frames, step, cap=None):
        p = step["pair"]
        return ctx.window_update(tab, frames, p["t1_left"], p["t1_right"], p["t2_left"], p["t2_right"], p["ids"], p["tri"], step["pose_a"],
                                 step["pose_b"], cap=cap)

    def solve(tab, **kw):
        s = dict(WC.BA_SETTINGS, **kw)
        return ctx.window_solve(tab, WC.P1, WC.P2, rounds=s["rounds"], iters=s["iters"], sigma_px=s["sigma"], min_obs=s["min_obs"])

    def device_table(tab, rows=None):
        m = tab["m"] if rows is None else rows
        t = {k: dev(tab[k][:m]) for k in ("ids", "X", "obs_left", "obs_right")}
        t["seen"], t["active"] = dev(tab["seen"][:m].view(np.int32)), dev(tab["active"][:m].view(np.int32))
        t["poses"], t["counts"] = dev(tab["poses"]), dev(np.array([tab["n"], tab["m"], 0, 0], np.int32))
        return t

    for name in sorted(WC.UPDATE_CASES):
        tab, frames, step, cap = WC.UPDATE_CASES[name]()
        got = update(tab, frames, step, cap)
        put("window_update %s host" % name, got)
        if name in ("slide_w2", "slide_w3_many_bad", "slide_w8", "rows_2049_tracks_1025"):
            put("window_update+solve %s host" % name, solve(got))
            p = step["pair"]
            o = ctx.window_update(device_table(tab), frames, *[dev(p[k]) for k in ("t1_left", "t1_right", "t2_left", "t2_right", "ids", "tri")],
                                  dev(step["pose_a"]), dev(step["pose_b"]), cap=tab["m"] + len(p["ids"]) + 7)
            ctx.sync()
            o = {k: v.cpu().numpy() for k, v in o.items()}
            m = int(o["counts"][1])
            put("window_update %s device" % name, {k: (v if k in ("poses", "counts") else v[:m]) for k, v in o.items()})
    for name in sorted(WC.BA_CASES):
        tab, _ = WC.scene(**{k: v for k, v in WC.BA_CASES[name].items() if k != "settings"})
        put("window_solve %s host" % name, solve(tab, **WC.BA_CASES[name].get("settings", {})))
        if name in ("n2_Tm1", "n3_T_holes", "n8_2Tp1_holes"):
            t = device_table(tab)
            raw, _ = solve(t)
            ctx.sync()
            put("window_solve %s device" % name, raw.cpu().numpy(), {k: t[k].cpu().numpy() for k in ("poses", "X", "active")})
    tab, _ = WC.scene(seed=1, n=4, m=300, starve=2, starve_left=0, outliers=0.3)
    put("window_solve lambda exit", solve(tab, rounds=2, iters=20))
    put("window_solve one frame", solve(dict(tab, n=1)))
    ctx.close()

    # ---- the fused online path
    n_frames = 9
    seq = synth.StereoSequence(width=416, height=128, n_frames=n_frames, seed=11, device=torch.device("cuda", 0))
    frames = [tuple(x.cpu().numpy() for x in seq.render(t)) for t in range(n_frames)]
    frames.append((np.zeros_like(frames[0][0]), np.zeros_like(frames[0][0])))
    for mode in ("reproj", "ba", "carry_window_3"):
        ctx = pkg.Context(416, 128, device=0, P1=seq.proj()[0], P2=seq.proj()[1])
        if mode == "carry_window_3":
            ctx.set_track_carry(True, 3.0, 0)
            ctx.set_window_ba(3, 4, 2, 1.0, 10)
        else:
            ctx.set_pose_refine(mode)
        steps = []
        for f, (L, R) in enumerate(frames):
            rc, rec = ctx.add_frame(L, R)
            if f == 0:
                continue
            step = [rc, np.asarray(rec).tobytes(), ctx.get_pose()]
            if mode == "carry_window_3":
                step += [ctx.window(), ctx.window_result()]
            else:
                step.append(ctx.refine_result(0))
                if mode == "ba":
                    step.append(ctx.refine_points(0))
            steps.append(digest(step))
            print("fused %s frame %d %s" % (mode, f, steps[-1]), flush=True)
        put("fused %s" % mode, steps)
        ctx.close()

    # ---- the tail of the pose stage
    P1, P2 = seq.proj()
    L, R = (torch.from_numpy(np.stack([f[k] for f in frames])).cuda() for k in (0, 1))
    seed = PR.rigid_motions(np.random.default_rng(5), 1)[0]
    for name, pose0 in (("identity", None), ("pose0", seed)):
        ctx = pkg.Context(416, 128, device=0, P1=P1, P2=P2, max_batch=16)
        put("chain track_batch %s" % name, ctx.track_batch(L, R, pose0=pose0).tobytes())
        ctx.close()
    ctx = pkg.Context(416, 128, device=0, P1=P1, P2=P2, max_batch=5)       # a step of m streams needs max_batch >= 2 m - 1
    ctx.streams_create(3)
    ids = [2, 0, 1]
    for t in range(3):
        if t == 2:
            ctx.streams_reset(ids[1])
            ctx.streams_set_pose(ids[2], seed)
        recs = ctx.streams_step(ids, [frames[t + 2 * k][0] for k in range(3)], [frames[t + 2 * k][1] for k in range(3)])
        put("chain streams step %d" % t, recs.tobytes(), [ctx.streams_get_pose(i) for i in ids])
    ctx.close()
    ctx = pkg.Context(64, 64, device=0)
    for (n, seeded), (T, ok, pose0) in sorted(PR.chain_cases().items()):
        put("chain relative n=%d %s host" % (n, "pose0" if seeded else "identity"), ctx.chain_relative(T.reshape(n, 16), ok, pose0))
        got = ctx.chain_relative(dev(T.reshape(n, 16)), dev(ok), pose0)
        ctx.sync()
        put("chain relative n=%d %s device" % (n, "pose0" if seeded else "identity"), got.cpu().numpy())
    ctx.close()
    for max_gap in (0, 2):
        ctx = pkg.Context(416, 128, device=0, P1=P1, P2=P2, max_batch=2)
        ctx.set_track_carry(True)
        ctx.set_keyframe(True, 60, max_gap)
        steps = []
        for f, (Lf, Rf) in enumerate(frames):
            rc, rec = ctx.add_frame(Lf, Rf)
            step = [rc, np.asarray(rec).tobytes(), ctx.get_pose()]
            if f:
                step += [ctx.keyframe_result(), ctx.keyframe_matches(), list(ctx.keyframe_table())]
            steps.append(digest(step))
        put("chain keyframe max_gap %d" % max_gap, steps)
        ctx.close()

    doc = {"tool": "tools/pose_digest.py", "device": torch.cuda.get_device_name(0), "cases": len(out), "digests": out}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w", encoding="utf-8") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
        print("wrote", args.out)


if __name__ == "__main__":
    main()
