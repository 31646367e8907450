#!/usr/bin/env python3
"""The ingest stage (svo_resize / svo_ingest_*): what downscaling full-size frames on the GPU costs, and what it buys.

Frames resident in HBM; every figure is from at least one second of calls after warm-up, ending in a synchronise; the two
sides of a comparison alternate inside this one process.

  kernel   the resize launch alone (Context.resize on device stacks) for 1, 16 and 128 stereo pairs 1920x1080 -> 960x540,
           nearest and linear (f 0.5: the 2x2 mean), and 1241x376 -> 620x188; beside it a plain 16-byte-per-lane device copy
           (tools/gpu/copy16.hip) that moves the same bytes: source bytes in the 128-byte lines the resize touches +
           destination bytes, counted from the tap geometry below; the copy reads half of that count and writes half.
           Wall time per call, launch boundary included; `--trace` runs the same launches a few times each for
           `rocprofv3 --kernel-trace --stats`, which gives the kernel times without it.
  step     ingest_streams_step from 1920x1080 against streams_step on ready 960x540 frames (the _same_ pixels: made by
           Context.resize), M = 1, 16, 128, LK and ORB: ms per step of each, and the difference.
  buys     the same rows as aggregate pairs/s of 1080p streams through the ingest path (ORB mode refuses a 1920x1080
           context, so it has no other path; for LK the comparison is the 1920x1080 `hd` figures of README.md).

Usage: python tools/bench_ingest.py [--out profiles/ingest_bench.json] [--modes lk,orb] [--streams 1,16,128] [--skip-steps]
       python tools/bench_ingest.py --trace        (under rocprofv3 --kernel-trace --stats, in a run of its own)
One JSON document on stdout and in --out."""
import argparse
import ctypes
import importlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

SW, SH, DW, DH, F = 1920, 1080, 960, 540, 0.5
T = 5                                   # rendered frames; a stream walks 0 .. T-1 .. 0
MAX_BATCH = 256
MIN_SECONDS = 1.0
LINE = 128


def tri(k):
    p = 2 * (T - 1)
    k %= p
    return k if k < T else p - k


def timed(step, sync, n_warm=2):
    for k in range(n_warm):
        step(k)
    sync()
    t0 = time.perf_counter()
    for k in range(4):
        step(n_warm + k)
    sync()
    est = (time.perf_counter() - t0) / 4
    n = max(8, int(np.ceil(1.2 * MIN_SECONDS / est)))
    t0 = time.perf_counter()
    for k in range(n):
        step(n_warm + 4 + k)
    sync()
    dt = time.perf_counter() - t0
    return dt / n, n, dt


def alternating(step_a, step_b, sync, rounds=3):
    """Median seconds per call of each side; the sides alternate (a, b, a, b, ...), each slice >= MIN_SECONDS / rounds."""
    global MIN_SECONDS
    keep, MIN_SECONDS = MIN_SECONDS, MIN_SECONDS / rounds
    try:
        a, b = [], []
        for _ in range(rounds):
            a.append(timed(step_a, sync)[0])
            b.append(timed(step_b, sync)[0])
    finally:
        MIN_SECONDS = keep
    return float(np.median(a)), float(np.median(b)), a, b


def touched_bytes(sw, sh, dw, dh, interp, f, pitch):
    """Source bytes in the 128-byte lines one image's resize reads (rows of `pitch` bytes from a line-aligned base) +
    destination bytes: the tap geometry of include/svo_abi.h in factor form."""
    scale = 1.0 / f
    if interp == "nearest":
        ys = np.unique(np.minimum(np.floor(np.arange(dh) * scale).astype(np.int64), sh - 1))
        xs = np.minimum(np.floor(np.arange(dw) * scale).astype(np.int64), sw - 1)
    elif scale == 2.0:
        ys, xs = np.arange(2 * dh), np.arange(2 * dw)
    else:
        fy = ((np.arange(dh) + 0.5) * scale - 0.5).astype(np.float32)
        y0 = np.floor(fy).astype(np.int64)
        ys = np.unique(np.clip(np.r_[y0, y0 + 1], 0, sh - 1))
        fx = ((np.arange(dw) + 0.5) * scale - 0.5).astype(np.float32)
        x0 = np.floor(fx).astype(np.int64)
        xs = np.clip(np.r_[x0, x0 + 1], 0, sw - 1)
    lines = 0
    for y in ys:
        lines += len(np.unique((y * pitch + xs) // LINE))
    return int(lines) * LINE + dw * dh


def load_copy16():
    so = os.path.join(ROOT, "tools", "gpu", "copy16.so")
    src = os.path.join(ROOT, "tools", "gpu", "copy16.hip")
    if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
        subprocess.check_call(["hipcc", "-O3", "--offload-arch=gfx950", "-shared", "-fPIC", "-o", so, src])
    lib = ctypes.CDLL(so)
    lib.copy16.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    return lib


KERNEL_CASES = [(SW, SH, DW, DH, 1), (SW, SH, DW, DH, 16), (SW, SH, DW, DH, 128), (1241, 376, 620, 188, 1), (1241, 376, 620, 188, 128)]


def kernel_section(torch, pkg, trace, pitch_align=256):
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream()
    ctx = pkg.Context(416, 128, device=0)
    ctx.set_stream(stream.cuda_stream)
    copy = load_copy16()
    rows = []
    for sw, sh, dw, dh, pairs in KERNEL_CASES:
        n = 2 * pairs
        pitch = (sw + pitch_align - 1) // pitch_align * pitch_align
        src = torch.randint(0, 256, (n, sh, pitch), dtype=torch.uint8, device=dev)
        dst = torch.zeros((n, dh, (dw + 255) // 256 * 256), dtype=torch.uint8, device=dev)
        for interp in ("nearest", "linear"):
            total = n * touched_bytes(sw, sh, dw, dh, interp, F, pitch)
            half = total // 2 // 16 * 16
            a = torch.empty(half, dtype=torch.uint8, device=dev)
            b = torch.empty(half, dtype=torch.uint8, device=dev)

            def k_resize(k):
                ctx.resize(src[:, :, :sw], dw, dh, interp, F, F, out=dst[:, :, :dw])

            def k_copy(k):
                rc = copy.copy16(a.data_ptr(), b.data_ptr(), half, stream.cuda_stream)
                assert rc == 0, rc
            if trace:
                for k in range(10):
                    k_resize(k)
                    k_copy(k)
                ctx.sync()
                print(json.dumps({"src": [sw, sh], "src_pitch": pitch, "pairs": pairs, "interp": interp, "bytes": total}), flush=True)
                continue
            tr, tc_, ra, rb = alternating(k_resize, k_copy, ctx.sync)
            row = {"src": [sw, sh], "src_pitch": pitch, "dst": [dw, dh], "pairs": pairs, "interp": interp, "bytes": total,
                   "resize_us": tr * 1e6, "copy_us": tc_ * 1e6, "resize_over_copy": tr / tc_,
                   "resize_TBps": total / tr / 1e12, "copy_TBps": 2 * half / tc_ / 1e12}
            rows.append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
            del a, b
    ctx.close()
    return rows


def step_section(torch, pkg, synth, modes, Ms):
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream()
    seq = synth.StereoSequence(width=SW, height=SH, n_frames=T, seed=11, device=dev)
    L = torch.zeros((T, SH, SW), dtype=torch.uint8, device=dev)
    R = torch.zeros((T, SH, SW), dtype=torch.uint8, device=dev)
    for f in range(T):
        L[f], R[f] = seq.render(f)
    period = 2 * (T - 1)
    out = {}
    for mode in modes:
        for interp in ("nearest", "linear"):
            P1, P2 = (pkg.scale_projection(P, F, F, interp).reshape(12) for P in seq.proj())
            kw = dict(P1=P1, P2=P2)
            if mode == "orb":
                kw.update(track_mode=pkg.MODE_ORB, min_move2=0.05 ** 2, max_move2=10.0 ** 2)
            a = pkg.Context(DW, DH, device=0, max_batch=MAX_BATCH, **kw)
            b = pkg.Context(DW, DH, device=0, max_batch=MAX_BATCH, **kw)
            for c in (a, b):
                c.set_stream(stream.cuda_stream)
                c.streams_create(max(Ms))
            a.ingest_create(SW, SH, interp, F, F)
            Ls, Rs = a.resize(L, DW, DH, interp, F, F), a.resize(R, DW, DH, interp, F, F)      # the ready working-size frames
            res_a = torch.zeros((MAX_BATCH, pkg.STEP_DTYPE.itemsize), dtype=torch.uint8, device=dev)
            res_b = torch.zeros_like(res_a)
            rows = []
            for M in Ms:
                ids = np.arange(M, dtype=np.int32)
                idx = [torch.tensor([tri(s + k) for s in range(M)], device=dev) for k in range(period)]
                big = [(L[i], R[i]) for i in idx]
                small = [(Ls[i], Rs[i]) for i in idx]
                a.streams_reset(-1)
                b.streams_reset(-1)

                def step_a(k):
                    a.ingest_streams_step(ids, big[k % period][0], big[k % period][1], results=res_a)

                def step_b(k):
                    b.streams_step(ids, small[k % period][0], small[k % period][1], results=res_b)
                ta, tb, ra, rb = alternating(step_a, step_b, lambda: (a.sync(), b.sync()))
                # both contexts have now played the same number of steps from the same reset: their records are equal
                a.streams_reset(-1)
                b.streams_reset(-1)
                for k in range(3):
                    step_a(k)
                    step_b(k)
                a.sync()
                b.sync()
                same = bool(torch.equal(res_a[:M], res_b[:M]))
                rec = np.frombuffer(res_a[:M].cpu().numpy().tobytes(), dtype=pkg.STEP_DTYPE)
                assert same, f"{mode} {interp} M={M}: ingest records differ from the plain step's"
                row = {"streams": M, "ingest_step_ms": ta * 1e3, "plain_step_ms": tb * 1e3, "difference_ms": (ta - tb) * 1e3,
                       "ingest_pairs_per_s": M / ta, "plain_pairs_per_s": M / tb, "records_equal": same,
                       "ok_last_step": int(rec["ok"].sum()), "ingest_ms_rounds": [x * 1e3 for x in ra],
                       "plain_ms_rounds": [x * 1e3 for x in rb]}
                rows.append(row)
                print(json.dumps({"mode": mode, "interp": interp, **row}), file=sys.stderr, flush=True)
                del big, small, idx
            a.close()
            b.close()
            out[f"{mode}_{interp}"] = rows
    return out


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ingest_bench.json"))
    ap.add_argument("--modes", default="lk,orb")
    ap.add_argument("--streams", default="1,16,128")
    ap.add_argument("--trace", action="store_true", help="ten launches of every kernel case only (for rocprofv3 --kernel-trace --stats)")
    ap.add_argument("--skip-steps", action="store_true")
    ap.add_argument("--pitch-align", type=int, default=256, help="source row pitch of the kernel section = width rounded up to this (16: 1920 stays 1920)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: the hot path has no CPU fallback")
    pkg = entry.load_package()
    synth = importlib.import_module(entry.PKG_NAME + ".synth")
    doc = {"source": [SW, SH], "working": [DW, DH], "factor": F, "frames": "HBM", "min_seconds": MIN_SECONDS,
           "device": torch.cuda.get_device_name(0)}
    doc["kernel_vs_copy"] = kernel_section(torch, pkg, args.trace, args.pitch_align)
    if args.trace:
        return
    if not args.skip_steps:
        doc["streams_step"] = step_section(torch, pkg, synth, args.modes.split(","), [int(x) for x in args.streams.split(",")])
    txt = json.dumps(doc, indent=1)
    with open(args.out, "w", encoding="utf-8") as f:
        f.write(txt + "\n")
    print(txt)


if __name__ == "__main__":
    main()
