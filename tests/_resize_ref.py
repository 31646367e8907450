"""numpy restatement of the three cv::resize branches of include/svo_abi.h (the yardstick of the resize / ingest tests).

Source sw x sh, destination dw x dh, 8-bit gray.  Factor form (fx, fy > 0): inv = f and the destination size must be
cvRound(source size * f); size form (fx = fy = 0): inv = destination / source.  scale = 1.0 / inv in double.

  resize_nearest : dst[dy][dx] = src[min(floor(dy * scale_y), sh - 1)][min(floor(dx * scale_x), sw - 1)]
  resize_linear  : scale 2.0 on both axes exactly -> the rounded mean of 2 x 2 blocks (upstream's integer-area reroute);
                   any other scale -> the 11-bit fixed-point bilinear of oracle/orb.c (orc_resize_linear_u8)

tests/test_resize_ref.py checks the bilinear branch against the oracle's C restatement."""
import numpy as np

INTERP_NEAREST, INTERP_LINEAR = 0, 1


def cv_round(x):
    """cvRound: rint, ties to even."""
    return np.rint(x)


def scales(sw, sh, dw, dh, fx=0.0, fy=0.0):
    """(scale_x, scale_y) = 1 / inv of the call, after the checks of the factor / size form."""
    assert (fx > 0 and fy > 0) or (fx == 0 and fy == 0), "factor form needs both factors"
    ix = float(fx) if fx else dw / sw
    iy = float(fy) if fy else dh / sh
    if fx:
        assert int(cv_round(sw * ix)) == dw and int(cv_round(sh * iy)) == dh, "dsize != cvRound(ssize * f)"
    assert 0 < ix <= 1 and 0 < iy <= 1, "downscale or identity only"
    return 1.0 / ix, 1.0 / iy


def out_size(sw, sh, fx, fy):
    """Destination size of the factor form."""
    return int(cv_round(sw * fx)), int(cv_round(sh * fy))


def resize_nearest(img, dw, dh, fx=0.0, fy=0.0):
    sh, sw = img.shape
    scx, scy = scales(sw, sh, dw, dh, fx, fy)
    xs = np.minimum(np.floor(np.arange(dw, dtype=np.float64) * scx).astype(np.int64), sw - 1)
    ys = np.minimum(np.floor(np.arange(dh, dtype=np.float64) * scy).astype(np.int64), sh - 1)
    return np.ascontiguousarray(img[ys][:, xs])


def _taps(n_dst, n_src, scale, clamp_like_x):
    f = ((np.arange(n_dst, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = (f - s.astype(np.float32)).astype(np.float32)
    if clamp_like_x:
        lo = s < 0
        f[lo] = 0
        s[lo] = 0
        hi = s >= n_src - 1
        f[hi] = 0
        s[hi] = n_src - 1
    a0 = cv_round((np.float32(1) - f) * np.float32(2048)).astype(np.int64)
    a1 = cv_round(f * np.float32(2048)).astype(np.int64)
    return s, a0, a1


def is_box(sw, sh, dw, dh, fx=0.0, fy=0.0):
    scx, scy = scales(sw, sh, dw, dh, fx, fy)
    return scx == 2.0 and scy == 2.0


def resize_linear(img, dw, dh, fx=0.0, fy=0.0):
    sh, sw = img.shape
    scx, scy = scales(sw, sh, dw, dh, fx, fy)
    if scx == 2.0 and scy == 2.0:                       # upstream reroutes exact 2x INTER_LINEAR to the 2x2 box mean
        assert 2 * dw <= sw and 2 * dh <= sh
        a = img[:2 * dh, :2 * dw].astype(np.int64)
        return np.ascontiguousarray(((a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2] + 2) >> 2).astype(np.uint8))
    sx, a0, a1 = _taps(dw, sw, scx, True)
    sy, b0, b1 = _taps(dh, sh, scy, False)
    sx1 = np.minimum(sx + 1, sw - 1)
    y0 = np.clip(sy, 0, sh - 1)
    y1 = np.clip(sy + 1, 0, sh - 1)
    I = img.astype(np.int64)
    r0 = I[y0][:, sx] * a0 + I[y0][:, sx1] * a1
    r1 = I[y1][:, sx] * a0 + I[y1][:, sx1] * a1
    out = (((b0[:, None] * (r0 >> 4)) >> 16) + ((b1[:, None] * (r1 >> 4)) >> 16) + 2) >> 2
    assert out.min() >= 0 and out.max() <= 255
    return np.ascontiguousarray(out.astype(np.uint8))


def resize(img, dw, dh, interp=INTERP_NEAREST, fx=0.0, fy=0.0):
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 2
    if interp in (INTERP_NEAREST, "nearest"):
        return resize_nearest(img, dw, dh, fx, fy)
    assert interp in (INTERP_LINEAR, "linear")
    return resize_linear(img, dw, dh, fx, fy)


def scale_projection(P, inv_x, inv_y, interp):
    """P_out = S P of include/svo_abi.h, in plain numpy (3 x 4)."""
    lin = interp in (INTERP_LINEAR, "linear")
    ox = 0.5 * (inv_x - 1) if lin else 0.0
    oy = 0.5 * (inv_y - 1) if lin else 0.0
    S = np.array([[inv_x, 0, ox], [0, inv_y, oy], [0, 0, 1.0]])
    return S @ np.asarray(P, np.float64).reshape(3, 4)
