#!/usr/bin/env python3
"""How many waves of lk_kernel are resident, by workgroup shape (CPU only; the reasoning's record, not a pass bar).

The waves of an lk_kernel workgroup share nothing but the LDS allocation, and a workgroup gives its LDS back only when
the SLOWEST of its W waves has ended: until then the slots of the finished waves stay empty, because no other workgroup
fits into a CU's LDS.  This script prices every wave of a few S0 pairs (lk_wave_model.collect(): the oracle's
iteration counts, four consecutive points a wave, four chained calls, lockstep policy, the "exact" instruction constants
of lk_wave_model.py), groups W consecutive waves into a workgroup as the kernel does and prints for W = 4, 2, 1

  * the mean and the tail of the wave cost,
  * the mean workgroup lifetime (slowest of its W waves) against the mean wave,
  * the in-order list-scheduling makespan of 32 items (what one XCD gets of a 256-pair launch) on the XCD's
    96 * 4 / W workgroup slots (32 CUs x 12 waves; for W = 1 also with the 11 per CU that the LDS granule left the
    28-column tiles) against the ideal (all 12 wave slots busy to the end), and the mean number of waves per SIMD that
    are still running while their workgroup is resident,

and, first, the LDS granule arithmetic of a workgroup's tiles at 28 and at 27 columns a slot tile.

usage: lk_wg_residency.py [pairs=2]"""
import heapq
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(os.path.dirname(HERE))]
from lk_wave_model import collect  # noqa: E402

LPF, LPS, ITF, ITS = 350, 208, 92, 32         # lk_wave_model.py "exact": per level pass 350 + 208 per slot, per iteration 92 + 32 per active slot
WAVE_SLOTS_PER_XCD = 32 * 12                  # 32 CUs x 4 SIMDs x 3 waves
ITEMS_PER_XCD = 32                            # 256 pairs dealt one per XCD in groups of 8
WAVES_PER_ITEM = 768                          # launch_lk: 3072 points per pass
LDS_PER_CU, LDS_GRANULE = 160 * 1024, 1280    # tools/gpu/lds_granule_probe.hip: 12 800 B -> 12 workgroups per CU, 12 801 B -> 11
COL_DW, SLOTS = 29, 4                         # csrc/lk.hip ExactTile: words per tile column (bank-conflict freedom), slot tiles per wave


def lds_fit(cols, W):
    """(bytes declared, bytes taken, workgroups per CU, waves per CU) of a W-wave workgroup with `cols`-column slot tiles"""
    declared = W * SLOTS * cols * COL_DW * 4
    taken = -(-declared // LDS_GRANULE) * LDS_GRANULE
    wgs = LDS_PER_CU // taken
    return declared, taken, wgs, min(12, wgs * W)


def wave_costs(its, livec):
    """instructions of every wave of one item: four consecutive points, the chained calls until all four are rejected"""
    n = its.shape[0]
    out = []
    for w0 in range(0, n, 4):
        I, Lv = its[w0:w0 + 4], livec[w0:w0 + 4]
        tot = 0.0
        for c in range(4):
            lv = Lv[:, c]
            if not lv.any():
                break
            for l in (3, 2, 1, 0):
                x = I[:, c, l][lv]
                tot += LPF + LPS * int(lv.sum())
                for j in range(int(x.max()) if len(x) else 0):
                    tot += ITF + ITS * int((x > j).sum())
        out.append(tot)
    return np.array(out)


def item_workgroups(costs, W):
    """lifetimes of an item's workgroups: wave k of the item is wave k % W of workgroup k // W (one pass when the item
    has at most 768 waves; a denser item's waves loop, which chains the chunks of a wave)"""
    waves = np.zeros(WAVES_PER_ITEM)
    k = np.arange(len(costs))
    np.add.at(waves, k % WAVES_PER_ITEM, costs)
    waves = waves[:min(len(costs), WAVES_PER_ITEM)]
    pad = (-len(waves)) % W
    return np.concatenate([waves, np.zeros(pad)]).reshape(-1, W).max(axis=1)


def makespan(lifetimes, slots):
    """workgroups dealt in order, each to the slot that frees first"""
    free = [0.0] * slots
    heapq.heapify(free)
    end = 0.0
    for t in lifetimes:
        e = heapq.heappop(free) + t
        end = max(end, e)
        heapq.heappush(free, e)
    return end


def main():
    npairs = int(sys.argv[1]) if len(sys.argv) > 1 else 2
    items = [wave_costs(its, livec) for its, livec in collect(npairs, 0)]
    allw = np.concatenate(items)
    print(f"waves {allw.size} ({npairs} pairs): cost mean {allw.mean() / 1e3:.1f} k instructions, p99 {np.percentile(allw, 99) / 1e3:.1f} k, "
          f"max {allw.max() / 1e3:.1f} k")
    for cols in (28, 27):
        for W in (4, 2, 1):
            declared, taken, wgs, waves = lds_fit(cols, W)
            print(f"{cols}-column tiles, W = {W}: {declared} B declared = {taken // LDS_GRANULE} granules = {taken} B; {wgs} workgroups = "
                  f"{waves} waves per CU ({waves / 4:.2f} per SIMD)")
    work = sum(items[i % npairs].sum() for i in range(ITEMS_PER_XCD))
    ideal = work / WAVE_SLOTS_PER_XCD
    # (W, workgroup slots of an XCD): LDS comes in 1280-byte granules.  A lone wave's 27-column tiles, 12 528 B, take ten
    # granules and twelve single-wave workgroups fit into a CU's 160 KB; at 28 columns (12 992 B, eleven granules) only
    # eleven did -- the last line -- while 3 x 4 and 6 x 2 waves fit at either width
    for W, slots in ((4, 96), (2, 192), (1, 384), (1, 32 * 11)):
        wgs = [item_workgroups(c, W) for c in items]
        life = np.concatenate(wgs)
        order = np.concatenate([wgs[i % npairs] for i in range(ITEMS_PER_XCD)])
        ms = makespan(order, slots)
        # a workgroup holds W wave slots for its lifetime; its waves run for their own cost only
        running = allw.sum() / (W * life.sum())
        print(f"W = {W}: workgroup lifetime mean {life.mean() / 1e3:.1f} k = {life.mean() / allw.mean():.3f} x mean wave; waves running while resident "
              f"{3 * running:.2f} of 3 per SIMD; makespan of {ITEMS_PER_XCD} items on {slots} slots {ms / 1e6:.3f} M = {ms / ideal:.3f} x ideal "
              f"({3 * ideal / ms:.2f} waves per SIMD over the launch)")


if __name__ == "__main__":
    main()
