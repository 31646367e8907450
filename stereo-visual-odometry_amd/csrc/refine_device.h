// refine_device.h -- what the three Levenberg-Marquardt optimisers share (refine.hip: pose_refine_kernel; ba.hip: pose_ba_kernel;
// window.hip: window_ba_kernel).  All three: the stereo rig, one view of one point (projection, residual, derivative rows), the
// pose-derivative row, the Huber weight, a point's 3 x 3 Cholesky elimination, the pair-valued cost and its wave butterfly (the plain one: wave_allsum_f64, svo_device.h), the
// small SO(3) / SE(3) helpers.  The two-frame kernels also: the 6 x 6 Cholesky solve every thread runs redundantly, the common
// part of their arguments (RefineCommon), the cut of the stage's device block and the host plumbing around a launch (defined
// in refine.hip).  The LM loops and the kernels' prologues and epilogues stay in the kernels.  Internal.
#pragma once
#include <cmath>
#include "abi_io.h"
#include "block_cut.h"

namespace svo {

constexpr int kRefineThreads = 256;
constexpr double kRefineMinDepth = 1e-6;

// The cost of a round is carried as an unevaluated pair (s, e): TwoSum keeps what every addition rounds away.  "The cost
// decreases" (R6) is decided on the pair, so the decision does not depend on the order the lanes add in (a plain sum of ~1000
// terms carries ~1e-13 of order-dependent noise).  The terms' own rounding -- u - x cancels at ~1e2 px -- remains.
__device__ inline bool refine_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }    // false for NaN and +-inf

__device__ inline void refine_dd_add(double &s, double &e, double bs, double be)
{
    const double t = s + bs, bb = t - s;
    // (an infinite sum has no tail: inf - inf would turn the infinite cost of an inf pixel into NaN)
    const double err = refine_finite(t) ? (s - (t - bb)) + (bs - bb) : 0.0;
    s = t;
    e = (e + be) + err;
}

// The cost pair across a wave: the butterfly with pair additions (TwoSum is symmetric, so every lane ends with the same pair)
__device__ inline void refine_wave_cost(double &cs, double &ce)
{
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        const double os = __shfl_xor(cs, m, 64), oe = __shfl_xor(ce, m, 64);
        refine_dd_add(cs, ce, os, oe);
    }
}
// ... and across the workgroup: the wave totals at red[w * stride] (sum) and red[w * stride + lo_at] (tail), added in wave order
// and normalised -- hi the rounded sum, lo what is left
__device__ inline void refine_block_cost(const double *red, int stride, int lo_at, int waves, double &hi, double &lo)
{
    double cs = red[0], ce = red[lo_at];
    for (int w = 1; w < waves; w++) refine_dd_add(cs, ce, red[w * stride], red[w * stride + lo_at]);
    const double h = cs + ce;
    hi = h;
    lo = ce - (h - cs);
}

// ---- one view of one point
struct StereoCam { double ML[9], MR[9], p4R[3]; };         // view L: [K1 | 0]; view R: P2 = [MR | p4R]

// K1 = (fx, fy, cx, cy) of P1 as the PnP stage takes it; P2 whole (null: a launch without a right view, zeros)
inline StereoCam stereo_cam(const double *P1, const double *P2)
{
    StereoCam c{{P1[0], 0.0, P1[2], 0.0, P1[5], P1[6], 0.0, 0.0, 1.0}, {}, {}};
    for (int i = 0; i < 3 && P2; i++) {
        for (int j = 0; j < 3; j++) c.MR[i * 3 + j] = P2[i * 4 + j];
        c.p4R[i] = P2[i * 4 + 3];
    }
    return c;
}

// The point Z (in the left camera's frame) in the left or the right view against the observation o: the residuals r[0], r[1],
// the rows A[0], A[1] = d pixel / dZ, and whether the view sees it (R3; where it does not, the depth counts as 1)
__device__ inline bool refine_project(const StereoCam &cam, bool right, const double *Z, float2 o, double *r, double (*A)[3])
{
    const double *M = right ? cam.MR : cam.ML;
    double h[3];
    for (int k = 0; k < 3; k++) {
        h[k] = (Z[0] * M[k * 3] + Z[1] * M[k * 3 + 1]) + Z[2] * M[k * 3 + 2];
        if (right) h[k] = h[k] + cam.p4R[k];
    }
    const bool ok = h[2] > kRefineMinDepth;
    const double h2 = ok ? h[2] : 1.0;
    const double u = h[0] / h2, w = h[1] / h2;
    r[0] = u - (double)o.x;
    r[1] = w - (double)o.y;
    for (int k = 0; k < 3; k++) { A[0][k] = (M[k] - u * M[6 + k]) / h2; A[1][k] = (M[3 + k] - w * M[6 + k]) / h2; }
    return ok;
}

// the row of d pixel / d xi that belongs to a = d pixel / dY at Y = R X + t: [a | -a^T [Y]x] = [a | (Y x a)^T]
__device__ inline void refine_pose_row(const double *a, const double *Y, double *J6)
{
    J6[0] = a[0]; J6[1] = a[1]; J6[2] = a[2];
    J6[3] = Y[1] * a[2] - Y[2] * a[1];
    J6[4] = Y[2] * a[0] - Y[0] * a[2];
    J6[5] = Y[0] * a[1] - Y[1] * a[0];
}

__device__ inline void refine_huber(bool robust, double c, double tau, double &w, double &rho)
{
    w = 1.0; rho = c;
    if (robust && c > tau) { w = sqrt(tau / c); rho = 2.0 * sqrt(tau * c) - tau; }
}

// ---- a point's own 3 x 3 block V (packed 00 10 11 20 21 22): L (l00 l10 l11 l20 l21 l22) the Cholesky factor of
// V + lam diag V, row by row; false when a pivot is <= 0 (that pivot counts as 1, and the solves below give 0)
__device__ inline bool refine_chol3(const double (&V)[6], double lam, double (&L)[6])
{
    const double d0 = V[0] + lam * V[0];
    bool ok = d0 > 0.0;
    L[0] = sqrt(ok ? d0 : 1.0);
    L[1] = V[1] / L[0];
    const double d1 = (V[2] + lam * V[2]) - L[1] * L[1];
    ok = ok && d1 > 0.0;
    L[2] = sqrt(ok ? d1 : 1.0);
    L[3] = V[3] / L[0];
    L[4] = (V[4] - L[3] * L[1]) / L[2];
    const double d2 = ((V[5] + lam * V[5]) - L[3] * L[3]) - L[4] * L[4];
    ok = ok && d2 > 0.0;
    L[5] = sqrt(ok ? d2 : 1.0);
    return ok;
}
// y = L^-1 b (y may be b)
__device__ inline void refine_fwd3(const double *L, const double *b, bool ok, double *y)
{
    const double y0 = b[0] / L[0];
    const double y1 = (b[1] - L[1] * y0) / L[2];
    const double y2 = ((b[2] - L[3] * y0) - L[4] * y1) / L[5];
    y[0] = ok ? y0 : 0.0; y[1] = ok ? y1 : 0.0; y[2] = ok ? y2 : 0.0;
}
// dX = -L^-T z
__device__ inline void refine_back3(const double *L, const double *z, bool ok, double (&dX)[3])
{
    const double e2 = z[2] / L[5];
    const double e1 = (z[1] - L[4] * e2) / L[2];
    const double e0 = ((z[0] - L[1] * e1) - L[3] * e2) / L[0];
    dX[0] = ok ? -e0 : 0.0; dX[1] = ok ? -e1 : 0.0; dX[2] = ok ? -e2 : 0.0;
}

__device__ inline void refine_mm3(const double A[9], const double B[9], double C[9])
{
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) C[i * 3 + j] = (A[i * 3] * B[j] + A[i * 3 + 1] * B[3 + j]) + A[i * 3 + 2] * B[6 + j];
}
__device__ inline void refine_mv3(const double A[9], const double v[3], double o[3])
{
    for (int i = 0; i < 3; i++) o[i] = (A[i * 3] * v[0] + A[i * 3 + 1] * v[1]) + A[i * 3 + 2] * v[2];
}

// exp(xi) of SE(3), xi = (rho, phi): E = exp([phi]x), Vr = V(phi) rho (R2)
__device__ inline void refine_se3_exp(const double xi[6], double E[9], double Vr[3])
{
    const double *phi = xi + 3;
    const double th2 = (phi[0] * phi[0] + phi[1] * phi[1]) + phi[2] * phi[2];
    const double th = sqrt(th2);
    double A = 1.0, B = 0.5, C = 1.0 / 6.0;
    if (!(th < 1e-10)) {
        const double sh = sin(0.5 * th), s = sin(th);
        A = s / th;
        B = 2.0 * sh * sh / th2;
        C = (th - s) / (th2 * th);
    }
    const double K[9] = {0.0, -phi[2], phi[1], phi[2], 0.0, -phi[0], -phi[1], phi[0], 0.0};
    double K2[9], V[9];
    refine_mm3(K, K, K2);
    for (int k = 0; k < 9; k++) {
        const double I = (k % 4 == 0) ? 1.0 : 0.0;
        E[k] = (I + A * K[k]) + B * K2[k];
        V[k] = (I + B * K[k]) + C * K2[k];
    }
    refine_mv3(V, xi, Vr);
}

// cv::Rodrigues vector -> matrix
__device__ inline void refine_rodrigues(const double r[3], double R[9])
{
    const double th = sqrt((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]);
    if (th < 2.220446049250313e-16) {
        for (int k = 0; k < 9; k++) R[k] = (k % 4 == 0) ? 1.0 : 0.0;
        return;
    }
    const double k0 = r[0] / th, k1 = r[1] / th, k2 = r[2] / th, kk[3] = {k0, k1, k2};
    const double c = cos(th), s = sin(th), c1 = 1.0 - c;
    const double Kx[9] = {0.0, -k2, k1, k2, 0.0, -k0, -k1, k0, 0.0};
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) R[i * 3 + j] = (c * (i == j ? 1.0 : 0.0) + c1 * (kk[i] * kk[j])) + s * Kx[i * 3 + j];
}

// rotation matrix -> rotation vector
__device__ inline void refine_so3_log(const double R[9], double r[3])
{
    const double v[3] = {0.5 * (R[7] - R[5]), 0.5 * (R[2] - R[6]), 0.5 * (R[3] - R[1])};
    const double s = sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
    const double c = 0.5 * (((R[0] + R[4]) + R[8]) - 1.0);
    const double th = atan2(s, c);
    if (s >= 1e-5 || c > 0) {
        const double f = s >= 1e-10 ? th / s : 1.0;
        for (int i = 0; i < 3; i++) r[i] = v[i] * f;
        return;
    }
    // near pi: the axis from the diagonal, signs from the off-diagonal sums (cv::Rodrigues)
    double ax[3];
    for (int i = 0; i < 3; i++) { const double q = (R[i * 4] + 1.0) * 0.5; ax[i] = sqrt(q > 0.0 ? q : 0.0); }
    if (R[1] < 0) ax[1] = -ax[1];
    if (R[2] < 0) ax[2] = -ax[2];
    if (fabs(ax[0]) < fabs(ax[1]) && fabs(ax[0]) < fabs(ax[2]) && (R[5] > 0) != (ax[1] * ax[2] > 0)) ax[2] = -ax[2];
    const double f = th / sqrt((ax[0] * ax[0] + ax[1] * ax[1]) + ax[2] * ax[2]);
    for (int i = 0; i < 3; i++) r[i] = ax[i] * f;
}

// 6 x 6 Cholesky solve A x = b, row by row; fails unless every pivot is > 0 (R6, R7).  Registers only: every thread of the
// workgroup solves the same system.
__device__ inline bool refine_chol6(const double (&A)[36], const double (&b)[6], double (&x)[6])
{
    double L[21];
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 6; i++) {
#pragma unroll
        for (int j = 0; j <= i; j++) {
            double s = A[i * 6 + j];
#pragma unroll
            for (int k = 0; k < j; k++) s -= L[i * (i + 1) / 2 + k] * L[j * (j + 1) / 2 + k];
            if (i == j) {
                ok = ok && s > 0.0;
                L[i * (i + 1) / 2 + i] = sqrt(s);
            } else {
                L[i * (i + 1) / 2 + j] = s / L[j * (j + 1) / 2 + j];
            }
        }
    }
    double y[6];
#pragma unroll
    for (int i = 0; i < 6; i++) {
        double s = b[i];
#pragma unroll
        for (int k = 0; k < i; k++) s -= L[i * (i + 1) / 2 + k] * y[k];
        y[i] = s / L[i * (i + 1) / 2 + i];
    }
#pragma unroll
    for (int i = 5; i >= 0; i--) {
        double s = y[i];
#pragma unroll
        for (int k = i + 1; k < 6; k++) s -= L[k * (k + 1) / 2 + i] * x[k];
        x[i] = s / L[i * (i + 1) / 2 + i];
    }
    return ok;
}

// ---- what pose_refine_kernel and pose_ba_kernel take alike (RefineArgs and BaArgs put their point and observation pointers
// beside it); the host plumbing below fills it
struct RefineCommon {
    int n_fixed, cap;                                            // stage call: the point count; points per item at most
    StereoCam cam;
    int rounds, iters, min_inliers; double sigma;
    PnpRecord *pnp;                                              // fused: the pairs' PnP records (start pose; rewritten when R7 says so)
    double rvec0[3], tvec0[3];                                   // stage call (pnp null): the start pose
    svo_refine_result *res; uint8_t *flags; int64_t flag_stride; // per item
};

// ---- the stage's device block: [records x (B + 1)][flags x (B + 1) x cap][stage-call X, xl, xr x cap]; item B is the stage call's
struct RefineCut { size_t flags, X, xl, xr, end; };
inline RefineCut refine_cut(const svo_config &c)
{
    const size_t items = (size_t)c.max_batch + 1, cap = (size_t)c.max_keypoints;
    BlockCut cut;
    cut.add(sizeof(svo_refine_result) * items);             // the records, at the front
    RefineCut r;
    r.flags = cut.add(items * cap); r.X = cut.add(sizeof(float) * 3 * cap);
    r.xl = cut.add(sizeof(float2) * cap); r.xr = cut.add(sizeof(float2) * cap); r.end = cut.total();
    return r;
}

// ---- the host plumbing both modes use (refine.hip).  refine_fill: a fused launch's common arguments (P2 null: no right view);
// refine_fill_stage: a stage call's -- item max_batch of the block, n points, the start pose by value; refine_stage_finish: after
// a stage call's launch, the record back through the pinned block and the flags back (mem); refine_fetch_record: record `pair`
// of the last fused launch into the pinned block, n_out its point count -- reported also when `cap` is too small for dst.
void refine_fill(const svo_ctx *ctx, RefineCommon &c, const double P1[12], const double P2[12]);
void refine_fill_stage(const svo_ctx *ctx, RefineCommon &c, const double P1[12], const double P2[12], int n, const double rvec0[3],
                       const double tvec0[3]);
int refine_stage_finish(svo_ctx *ctx, const RefineCommon &c, int n, svo_refine_result *res, uint8_t *active, int mem);
int refine_fetch_record(svo_ctx *ctx, int pair, const void *dst, int cap, const char *too_small, svo_refine_result **h, int *n_out);

}  // namespace svo
