// refine_device.h -- what the pose refinement kernels share (refine.hip: pose_refine_kernel; ba.hip: pose_ba_kernel): the
// wave butterfly and the pair addition of the cost, the small SO(3) / SE(3) helpers, the 6 x 6 Cholesky solve every thread runs
// redundantly, and the cut of the stage's device block.  Internal.
#pragma once
#include <cmath>
#include "abi_io.h"
#include "block_cut.h"

namespace svo {

constexpr int kRefineThreads = 256;
constexpr double kRefineMinDepth = 1e-6;

__device__ inline double refine_wave_allsum(double v)
{
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v = v + __shfl_xor(v, m, 64);
    return v;
}

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

}  // namespace svo
