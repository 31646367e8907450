#!/usr/bin/env python3
"""The carry / keyframe / window chain against the renderer's ground truth, on the CPU (the oracle and the numpy twins; no GPU).

  exact_chain   tests/_exact_chain.py's exact correspondences through the twins (both rigs, max_gap 0 and 4, W = 3 and 8): the
                worst absolute element difference of any pose from the truth -- the constant WORST of tests/test_exact_chain.py;
  rendered      test_gpu_keyframe's twin chain (the oracle's LK, _carry_ref, _keyframe_ref) on its 12 rendered frames: the
                transfer error of one pair's PnP inliers, the slide of a carried id by age, the share of inlier observations
                beyond 10 px, the disparity error of the keyframe tables -- the constants of tests/test_gpu_chain_truth.py --
                and per step the error of the pair-chained and the keyframe pose against the truth, by gap.

Writes profiles/chain_truth.json (or --out) and prints the constants the tests commit.  The HIP chain equals the twin chain
byte for byte in tracks, ids and tables (tests/test_gpu_keyframe.py), so the figures are the GPU's as well."""
import argparse
import importlib
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import __graft_entry__ as entry  # noqa: E402


def exact_chain(oracle, synth):
    import _exact_chain as EC
    seq, rows = EC.sequence(synth), []
    for rig in ("default", "R3X"):
        P1, P2 = EC.rig_matrices(seq, rig)
        case = EC.make(seq, P1=P1, P2=P2)
        for max_gap in (0, 4):
            for W in (3, 8):
                r = EC.twin_run(oracle, case, W, max_gap)
                rows.append(dict(rig=rig, max_gap=max_gap, W=W, tracks_max=max(len(p["ids"]) for p in case["pairs"]),
                                 rows_max=max(e["mid"]["m"] for e in r.steps), gap_max=max(e["kf"]["gap"] for e in r.steps), **r.worst()))
                print("exact", rows[-1])
    worst = max(max(v for k, v in r.items() if isinstance(v, float)) for r in rows)
    return dict(generator=dict(n_frames=EC.N_FRAMES, births=EC.BIRTHS, every=EC.EVERY, seed=EC.SEED), runs=rows, worst=worst)


def rendered(oracle, synth):
    import _keyframe_ref as KR
    import _truth as TR
    import test_gpu_keyframe as TK
    seq = synth.StereoSequence(width=416, height=128, n_frames=TK.N_FRAMES, seed=11)
    frames = [tuple(x.numpy() for x in seq.render(t)) for t in range(TK.N_FRAMES)]
    ref = TK.twin_chain(oracle, seq, frames)
    truth = seq.poses_wc().numpy()
    steps, poses = [], []
    for t, e in enumerate(ref[1:], 1):
        k = e["kf"]
        steps.append(dict(tracks=list(e["res"]["tracks"]) + [e["pnp"]["mask"]], ids=e["trk_ids"],
                          table=(t - 1, e["tab_X"]) if k["switched"] else None))
        err = lambda P: dict(rot=float(np.abs(P[:3, :3] - truth[t][:3, :3]).max()), trans_m=float(np.linalg.norm(P[:3, 3] - truth[t][:3, 3])))
        poses.append(dict(frame=t, status=int(k["status"]), gap=int(k["gap"]), switched=int(k["switched"]), n_join=int(k["n_join"]),
                          n_inliers=int(k["n_inliers"]), pair_chained=err(k["pose_pair"]), reported=err(k["pose"])))
    st = TR.chain_stats(seq, steps)
    st["age"], st["age_n"], st["age_over3"] = ({str(a): v for a, v in st[q].items()} for q in ("age", "age_n", "age_over3"))
    return dict(sequence=dict(width=416, height=128, n_frames=TK.N_FRAMES, seed=11, min_tracks=TK.MIN_TRACKS, max_gap=TK.MAX_GAP),
                applied=sum(p["status"] == KR.APPLIED for p in poses), stats=st, poses=poses)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chain_truth.json"))
    a = ap.parse_args()
    oracle = entry.load_oracle()
    oracle.build()
    entry.load_package()
    synth = importlib.import_module(entry.PKG_NAME + ".synth")
    out = dict(tool="tools/chain_truth.py", exact_chain=exact_chain(oracle, synth), rendered=rendered(oracle, synth))
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    st = out["rendered"]["stats"]
    print("\n# tests/test_exact_chain.py")
    w = out["exact_chain"]["worst"]
    unit = 10.0 ** math.floor(math.log10(w))
    print("WORST = %.0e      # measured %.3e, rounded up to one digit" % (math.ceil(w / unit) * unit, w))
    print("\n# tests/test_gpu_chain_truth.py")
    print("PAIR = dict(median=%.4f, p99=%.4f, max=%.4f)" % (st["pair"]["median"], st["pair"]["p99"], st["pair"]["max"]))
    print("AGE_MEDIAN = {%s}" % ", ".join("%s: %.4f" % (a, v) for a, v in st["age"].items()))
    print("BEYOND_10PX = %.5f      # of %d inlier observations; the condition is <= 0.005" % (st["beyond10"]["share"], st["beyond10"]["n"]))
    print("TABLE = dict(median_abs=%.4f, abs_mean=%.4f)      # %d rows" % (st["table"]["median_abs"], st["table"]["abs_mean"], st["table"]["n"]))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
