"""Input builders for the FAST record, group and batch bounds (numpy only; no GPU, no oracle).

fast.hip hands its corners from the score kernel to the emit kernel through per-tile records -- 64 bytes per (image row,
64-pixel tile column): up to 32 two-byte records with NMS, up to 64 one-byte records without -- and one count byte per
(row, tile column), which the emit kernel walks in groups of 1024 (csrc/fast_scratch.h).  The builders here make images
that REACH those bounds; tests/test_fast_cases.py shows on the CPU oracle that they do, tests/test_gpu_fast_bounds.py then
holds the kernels to the oracle on them."""
import numpy as np

from conftest import rand_image

TILE_W = 64                 # kFastTileW: pixels per tile column = bytes per (row, tile column) of records
GROUP = 1024                # kEmitEntries: count bytes per workgroup of the emit kernel


def staircase_rows(w, h, rows, x_lo=61, x_hi=127, steps=(9, 12)):
    """255 everywhere; every row y0 of `rows` is 0 except for a staircase on x_lo .. x_hi + 3 that starts at 0 and obeys
    v(x + 3) = v(x) + steps[x & 1] for x_lo <= x <= x_hi (clipped at 255).

    Every pixel x_lo <= x <= x_hi of such a row is a FAST corner for thr < min(steps) as long as the staircase stays below
    255: the 15 circle pixels other than (-3, 0) are brighter -- 14 of them 255, (3, 0) by steps[x & 1] -- and every 9-arc
    that avoids (-3, 0) holds (3, 0), so the score is steps[x & 1] - 1.  With steps[1] > steps[0] strict 3x3 NMS keeps
    exactly the odd x.  The rows above and below are flat 255 and hold no corner; rows must be at least 4 apart (a
    radius-3 circle then never meets a second row).  Past x_hi + 3 the row is 0 again: x_hi + 1 .. x_hi + 3 see a darker
    pixel at (-3, 0) AND at (3, 0) and are no corners, x_hi + 4 is one (response v(x_hi + 1) - 1) where the image has it."""
    rows = tuple(rows)
    assert all(b - a >= 4 for a, b in zip(rows, rows[1:])) and x_lo >= 3 and x_hi + 3 < w
    img = np.full((h, w), 255, np.uint8)
    v = np.zeros(w, np.int64)
    for x in range(x_lo, x_hi + 1):
        v[x + 3] = min(255, v[x] + steps[x & 1])
    for y0 in rows:
        img[y0] = v
    return img


def minus_one(w, h, x, y):
    """Flat 100 with one pixel of 99: at thr 0 that pixel is a corner (16 brighter pixels) whose score is 0."""
    img = np.full((h, w), 100, np.uint8)
    img[y, x] = 99
    return img


def lattice(w, h, lo, hi):
    """`hi` on the 4-pixel lattice (3 + 4i, 3 + 4j) over `lo`: every testable lattice point a corner of score hi - lo - 1."""
    img = np.full((h, w), lo, np.uint8)
    img[3::4, 3::4] = hi
    return img


# (w, h): tile columns x rows = count bytes of the emit kernel
EMIT_SHAPES = [
    (512, 128),             # 1024: one group exactly
    (64, 1025),             # 1025: the second group holds one dead row (y = 1024 >= h - 3) and no corner
    (64, 1029),             # 1029 = 1 mod 4, one tile column: a thread's four counts are four image rows
    (128, 517),             # 1034 = 2 mod 4
    (192, 345),             # 1035 = 3 mod 4, three tile columns
]


def emit_image(w, h):
    return rand_image(h, w, 3, blocks=False)


def tile_cols(w):
    return (w + TILE_W - 1) // TILE_W


def count_bytes(w, h):
    return tile_cols(w) * h


def per_tile_row(kps, w, h):
    """(h, tile columns) corners per (image row, tile column): what the score kernel's count bytes must hold."""
    out = np.zeros((h, tile_cols(w)), np.int64)
    np.add.at(out, (kps["y"].astype(np.int64), kps["x"].astype(np.int64) // TILE_W), 1)
    return out


def per_group(kps, w, h):
    """corners per workgroup of the emit kernel (1024 consecutive count bytes in raster order)"""
    c = per_tile_row(kps, w, h).ravel()
    n = (len(c) + GROUP - 1) // GROUP
    return np.pad(c, (0, n * GROUP - len(c))).reshape(n, GROUP).sum(1)
