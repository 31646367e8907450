"""numpy restatement of cv::goodFeaturesToTrack(img, maxCorners, qualityLevel, minDistance, noArray(), 3, false, 0.04) -- what
cv::GFTTDetector::detect calls -- as include/svo_abi.h (svo_gftt_detect) and DESIGN.md state it.  Restated from memory of
OpenCV 3.4 (corner.cpp, featureselect.cpp, deriv.cpp, filter.cpp, smooth.cpp); unpinned, like the rest of the project.

All arithmetic is float32, one rounding per operation (no fused multiply-add), except the 3x3 box sums, which are accumulated
in float64 and rounded once."""
import numpy as np

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                     ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])

S = np.float32(1.0 / (4.0 * 3.0 * 255.0))
F0 = np.float32(2) * S
F1 = S


def _pad101(a):
    return np.pad(a, 1, mode="reflect")


def sobel(img):
    """(dx, dy) float32: 3x3 Sobel scaled by S, image border reflect-101."""
    p = _pad101(np.asarray(img, np.uint8).astype(np.int32))            # (h + 2, w + 2)
    # Dx: row pass in exact integers, the scale on the column kernel
    r = p[:, 2:] - p[:, :-2]                                           # (h + 2, w)
    dx = r[1:-1].astype(np.float32) * F0 + (r[:-2] + r[2:]).astype(np.float32) * F1
    # Dy: the scale on the row kernel, the column pass a difference
    q = p[:, 1:-1].astype(np.float32) * F0 + (p[:, :-2] + p[:, 2:]).astype(np.float32) * F1    # (h + 2, w)
    dy = q[2:] - q[:-2]
    return dx.astype(np.float32), dy.astype(np.float32)


def box3_f64(c):
    """3x3 unnormalised box sum of a float32 map, border reflect-101 OF THE MAP, float64 accumulation in the order of a box
    filter: the three values of a row first, (p0 + p1) + p2, then the three rows, (r0 + r1) + r2 (the nine products are not
    always exact in 53 bits, see tests/test_gftt_ref.py, so the order is part of the recipe)."""
    h, w = c.shape
    p = _pad101(c).astype(np.float64)
    rows = (p[:, 0:w] + p[:, 1:w + 1]) + p[:, 2:w + 2]                  # (h + 2, w)
    return (rows[0:h] + rows[1:h + 1]) + rows[2:h + 2]


def cov_sums(img):
    """The three box sums in float64 (before the single rounding to float32)."""
    dx, dy = sobel(img)
    return box3_f64(dx * dx), box3_f64(dx * dy), box3_f64(dy * dy)


def min_eigen_map(img):
    sxx, sxy, syy = cov_sums(img)
    a = sxx.astype(np.float32) * np.float32(0.5)
    b = sxy.astype(np.float32)
    c = syy.astype(np.float32) * np.float32(0.5)
    d = a - c
    return ((a + c) - np.sqrt(d * d + b * b)).astype(np.float32)


def threshold(eig, quality_level):
    return np.float32(np.float64(eig.max()) * np.float64(quality_level))


def candidates(eig, quality_level):
    """Raster indices y * w + x of the interior local maxima above the threshold, in selection order: eigenvalue descending,
    ties to the LARGER raster index first."""
    h, w = eig.shape
    if h < 3 or w < 3:
        return np.zeros(0, np.int64)
    thr = threshold(eig, quality_level)
    c = eig[1:-1, 1:-1]
    ok = c > thr
    for j in range(3):
        for i in range(3):
            if i == 1 and j == 1:
                continue
            ok &= c >= eig[j:j + h - 2, i:i + w - 2]
    ys, xs = np.nonzero(ok)
    idx = (ys + 1).astype(np.int64) * w + (xs + 1)
    val = eig.reshape(-1)[idx]
    order = np.lexsort((-idx, -val.astype(np.float64)))
    return idx[order]


def cv_round(v):
    """cvRound: round half to even."""
    return int(np.rint(np.float64(v)))


def greedy_grid(xs, ys, width, height, max_corners, min_distance):
    """Indices (into the ordered candidate list) of the corners kept by the cell-grid greedy pass."""
    kept = []
    if min_distance >= 1:
        cell = cv_round(min_distance)
        gw, gh = (width + cell - 1) // cell, (height + cell - 1) // cell
        grid = [[] for _ in range(gw * gh)]
        md2 = float(min_distance) * float(min_distance)
        for k in range(len(xs)):
            x, y = int(xs[k]), int(ys[k])
            cx, cy = x // cell, y // cell
            good = True
            for yy in range(max(0, cy - 1), min(gh - 1, cy + 1) + 1):
                for xx in range(max(0, cx - 1), min(gw - 1, cx + 1) + 1):
                    for (px, py) in grid[yy * gw + xx]:
                        dx, dy = x - px, y - py
                        if float(dx * dx + dy * dy) < md2:
                            good = False
                            break
                    if not good:
                        break
                if not good:
                    break
            if good:
                grid[cy * gw + cx].append((x, y))
                kept.append(k)
                if max_corners > 0 and len(kept) == max_corners:
                    break
    else:
        n = len(xs) if max_corners <= 0 else min(len(xs), max_corners)
        kept = list(range(n))
    return np.asarray(kept, np.int64)


def greedy_brute(xs, ys, max_corners, min_distance):
    """The same selection without the grid: O(n^2)."""
    kept = []
    md2 = float(min_distance) * float(min_distance)
    for k in range(len(xs)):
        x, y = int(xs[k]), int(ys[k])
        if min_distance >= 1 and any(float((x - int(xs[j])) ** 2 + (y - int(ys[j])) ** 2) < md2 for j in kept):
            continue
        kept.append(k)
        if max_corners > 0 and len(kept) == max_corners:
            break
    return np.asarray(kept, np.int64)


def records(xs, ys):
    """The cv::KeyPoint records GFTTDetector::detect makes."""
    out = np.zeros(len(xs), KP_DTYPE)
    out["x"] = xs
    out["y"] = ys
    out["size"] = 3.0
    out["angle"] = -1.0
    out["response"] = 0.0
    out["octave"] = 0
    out["class_id"] = -1
    return out


def n_candidates(img, quality_level=0.01):
    return int(len(candidates(min_eigen_map(img), quality_level)))


def gftt(img, max_corners=500, quality_level=0.01, min_distance=20.0, eig=None):
    """(records in selection order, float32 strength of each) of one uint8 image."""
    img = np.asarray(img, np.uint8)
    h, w = img.shape
    if eig is None:
        eig = min_eigen_map(img)
    idx = candidates(eig, quality_level)
    xs, ys = idx % w, idx // w
    keep = greedy_grid(xs, ys, w, h, int(max_corners), float(min_distance))
    return records(xs[keep], ys[keep]), eig.reshape(-1)[idx[keep]].astype(np.float32)
