"""numpy restatement of the FAST corner buckets (include/svo_abi.h, svo_set_fast_buckets): a grid of cell_w x cell_h pixel
cells anchored at (0, 0); per cell the per_cell corners of highest response stay, ties to the corner that comes first in
raster order (the order of the list); the survivors stay in raster order, records untouched."""
import numpy as np


def bucket_cells(kps, width, cell_w, cell_h):
    cols = (int(width) + cell_w - 1) // cell_w
    return (kps["y"].astype(np.int64) // cell_h) * cols + kps["x"].astype(np.int64) // cell_w


def bucket(kps, width, height, cell_w, cell_h, per_cell):
    cell = bucket_cells(kps, width, cell_w, cell_h)
    keep = []
    for c in np.unique(cell):
        idx = np.flatnonzero(cell == c)
        keep.append(idx[np.argsort(-kps["response"][idx], kind="stable")[:per_cell]])
    keep = np.sort(np.concatenate(keep)) if keep else np.zeros(0, np.int64)
    return kps[keep]
