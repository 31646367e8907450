// ba.hip -- two-frame stereo bundle adjustment after solvePnPRansac for gfx950: the pose refinement stage's second mode
// (SVO_REFINE_BA).  Where pose_refine_kernel (refine.hip) holds the triangulated t1 points fixed, this kernel minimises the
// reprojection error in all four images (three in ORB mode) over the pose AND the points.  The arithmetic is stated in
// include/svo_abi.h and DESIGN.md section 5g; tests/_ba_ref.py is its numpy twin.
//
// pose_ba_kernel: ONE workgroup of four waves per pair, lanes stride the pair's points -- the mapping, the butterfly, the
// fixed-order cross-wave sum and the pair-valued cost of pose_refine_kernel (refine_device.h, which also holds the per-view
// math and the 3 x 3 elimination), so that every thread holds the same reduced 6 x 6 system, solves it redundantly in registers
// and takes the same accept / reject / round decisions.
// A point is eliminated by the 3 x 3 Cholesky factor of its own block in its lane's registers; one LM iteration is two passes
// over the points: ba_build (the reduced sums at the accepted estimate and the current damping) and ba_trial (the
// back-substitution, the trial points, the cost at the trial estimate).  The accepted and the trial points of a pair live in
// device memory in two buffers swapped by pointer; a point and its flag are only ever touched by the lane that strides over it.
#include "refine_device.h"

namespace svo {

// cost | H (21, row-major upper triangle) | g (6) | diag of sum U (6) | active count | cost tail | bad count | largest |dX|^2
constexpr int kBaAcc = 38;
constexpr int kBaG = 22, kBaDiag = 28, kBaCount = 34, kBaCostLo = 35, kBaBad = 36, kBaStep = 37;

struct BaArgs {
    const float *X3; const float2 *x1l, *x1r, *x2l, *x2r; int64_t stride;     // points of item b at + b * stride (x2r: d = 8 only)
    RefineCommon c;
    double *Xa, *Xb; int64_t x_stride;                                       // the two point buffers of item b at + b * x_stride * 3
};

// One point in all its views: residuals (t1_left, t1_right, t2_left[, t2_right]), the derivative rows of each pixel with
// respect to the 3-D point it projects (X at t1, Y = R X + t at t2), and whether every view sees it (R3)
template <int V2>
struct BaPoint { double r[4 + 2 * V2], A[4 + 2 * V2][3], Y[3]; bool proj; };

template <int V2>
__device__ inline void ba_eval(const BaArgs &a, const double (&X)[3], const double (&R)[9], const double (&t)[3], const float2 (&o)[4],
                               BaPoint<V2> &p)
{
    for (int k = 0; k < 3; k++) p.Y[k] = ((X[0] * R[k * 3] + X[1] * R[k * 3 + 1]) + X[2] * R[k * 3 + 2]) + t[k];
    p.proj = true;
#pragma unroll
    for (int v = 0; v < 2 + V2; v++) p.proj = refine_project(a.c.cam, v & 1, v < 2 ? X : p.Y, o[v], p.r + 2 * v, p.A + 2 * v) && p.proj;
}

template <int V2>
__device__ inline double ba_chi(const BaPoint<V2> &p, double s2)
{
    if (!p.proj) return 0.0;
    double c = p.r[0] * p.r[0];
#pragma unroll
    for (int k = 1; k < 4 + 2 * V2; k++) c += p.r[k] * p.r[k];
    return c / s2;
}

// A point's share of the normal equations at weight ws = w_i / sigma^2 and damping lam, with the point eliminated:
// L the Cholesky factor of V* = V + lam diag V (l00 l10 l11 l20 l21 l22), T = W L^-T, y = L^-1 g_x; ok false when a pivot is
// <= 0 (T = 0, y = 0: the point then contributes U and g_p only and is not moved).  ACC: U - T T^T, g_p - T y and diag U are
// added to acc.
struct BaSys { double L[6], T[6][3], y[3]; bool ok; };

template <int V2, bool ACC>
__device__ inline void ba_system(const BaPoint<V2> &p, const double (&R)[9], double ws, double lam, BaSys &s, double *acc)
{
    constexpr int D = 4 + 2 * V2, D2 = 2 * V2;
    double Jx[D][3], Jp[D2][6];
#pragma unroll
    for (int k = 0; k < 4; k++)
        for (int j = 0; j < 3; j++) Jx[k][j] = p.A[k][j];
#pragma unroll
    for (int m = 0; m < D2; m++) {
        const double *A = p.A[4 + m];
        for (int j = 0; j < 3; j++) Jx[4 + m][j] = (A[0] * R[j] + A[1] * R[3 + j]) + A[2] * R[6 + j];      // a^T R
        refine_pose_row(A, p.Y, Jp[m]);
    }
    double V[6], gx[3], gp[6];                                       // V: 00 10 11 20 21 22
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j <= i; j++) {
            double v = Jx[0][i] * Jx[0][j];
#pragma unroll
            for (int k = 1; k < D; k++) v += Jx[k][i] * Jx[k][j];
            V[i * (i + 1) / 2 + j] = ws * v;
        }
        double g = Jx[0][i] * p.r[0];
#pragma unroll
        for (int k = 1; k < D; k++) g += Jx[k][i] * p.r[k];
        gx[i] = ws * g;
    }
#pragma unroll
    for (int q = 0; q < 6; q++) {
#pragma unroll
        for (int j = 0; j < 3; j++) {
            double v = Jp[0][q] * Jx[4][j];
#pragma unroll
            for (int m = 1; m < D2; m++) v += Jp[m][q] * Jx[4 + m][j];
            s.T[q][j] = ws * v;                                      // W for now
        }
        double g = Jp[0][q] * p.r[4];
#pragma unroll
        for (int m = 1; m < D2; m++) g += Jp[m][q] * p.r[4 + m];
        gp[q] = ws * g;
    }
    s.ok = refine_chol3(V, lam, s.L);
#pragma unroll
    for (int q = 0; q < 6; q++) refine_fwd3(s.L, s.T[q], s.ok, s.T[q]);      // T = W L^-T
    refine_fwd3(s.L, gx, s.ok, s.y);
    if (ACC) {
        int idx = 1;
#pragma unroll
        for (int q = 0; q < 6; q++) {
#pragma unroll
            for (int c = q; c < 6; c++) {
                double u = Jp[0][q] * Jp[0][c];
#pragma unroll
                for (int m = 1; m < D2; m++) u += Jp[m][q] * Jp[m][c];
                u = ws * u;
                acc[idx++] += u - ((s.T[q][0] * s.T[c][0] + s.T[q][1] * s.T[c][1]) + s.T[q][2] * s.T[c][2]);
                if (c == q) acc[kBaDiag + q] += u;
            }
            acc[kBaG + q] += gp[q] - ((s.T[q][0] * s.y[0] + s.T[q][1] * s.y[1]) + s.T[q][2] * s.y[2]);
        }
    }
}

enum { kBaInit = 0, kBaReclass = 1, kBaKeep = 2 };

struct BaItem { const float *X3; const float2 *x1l, *x1r, *x2l, *x2r; uint8_t *flags; int n; };

template <int V2>
__device__ inline void ba_load(const BaItem &it, const double *Xc, int i, double (&X)[3], float2 (&o)[4])
{
    for (int k = 0; k < 3; k++) X[k] = Xc[3 * (int64_t)i + k];
    o[0] = it.x1l[i]; o[1] = it.x1r[i]; o[2] = it.x2l[i];
    o[3] = V2 == 2 ? it.x2r[i] : make_float2(0.f, 0.f);
}

// The reduced system at the accepted estimate (R, t, Xc) and damping lam.
//   kBaInit: the active set becomes every projectable point; kBaReclass: every point is re-classified first -- active iff
//   projectable and c_i <= tau -- and a point that ends inactive returns to its triangulation; kBaKeep: the flags stand.
// S (LDS, complete for every thread on return): cost | H | g | diag sum U | count | cost tail -- H, g with 1 / sigma^2 applied.
template <int V2>
__device__ void ba_build(const BaArgs &a, const BaItem &it, double *Xc, const double (&R)[9], const double (&t)[3], int mode, bool robust,
                         double tau, double s2, double lam, double *red, double *S)
{
    double acc[kBaAcc];
    for (int k = 0; k < kBaAcc; k++) acc[k] = 0.0;
    const double is2 = 1.0 / s2;
    for (int i = threadIdx.x; i < it.n; i += kRefineThreads) {
        double X[3];
        float2 o[4];
        ba_load<V2>(it, Xc, i, X, o);
        BaPoint<V2> p;
        ba_eval<V2>(a, X, R, t, o, p);
        const double c = ba_chi<V2>(p, s2);
        bool act;
        if (mode == kBaInit) act = p.proj;
        else if (mode == kBaReclass) act = p.proj && c <= tau;
        else act = it.flags[i] != 0;
        if (mode != kBaKeep) {
            it.flags[i] = act ? 1 : 0;
            if (!act) for (int k = 0; k < 3; k++) Xc[3 * (int64_t)i + k] = (double)it.X3[3 * i + k];
        }
        if (!act) continue;
        double w, rho;
        refine_huber(robust, c, tau, w, rho);
        refine_dd_add(acc[0], acc[kBaCostLo], rho, 0.0);
        acc[kBaCount] += 1.0;
        BaSys s;
        ba_system<V2, true>(p, R, w * is2, lam, s, acc);
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    __syncthreads();                                        // `red` and S may still be read from the previous pass
    for (int k = 1; k <= kBaCount; k++) {
        const double ws = wave_allsum_f64(acc[k]);
        if (lane == 0) red[wave * kBaAcc + k] = ws;
    }
    refine_wave_cost(acc[0], acc[kBaCostLo]);
    if (lane == 0) { red[wave * kBaAcc] = acc[0]; red[wave * kBaAcc + kBaCostLo] = acc[kBaCostLo]; }
    __syncthreads();
    const int k = threadIdx.x;
    if (k >= 1 && k <= kBaCount) S[k] = ((red[k] + red[kBaAcc + k]) + red[2 * kBaAcc + k]) + red[3 * kBaAcc + k];
    if (k == 0) refine_block_cost(red, kBaAcc, kBaCostLo, 4, S[0], S[kBaCostLo]);
    __syncthreads();
}

// A trial step: dX_i = -L^-T (y + T^T xi) from the system at the accepted estimate, the trial points to Xt (EVERY point of the
// pair: the ones that do not move are copied), the cost at (Rn, tn, Xt) over the standing flags.
// S: cost | cost tail | the count of active points that are not projectable there | the largest |dX_i|^2.
template <int V2>
__device__ void ba_trial(const BaArgs &a, const BaItem &it, const double *Xc, double *Xt, const double (&R)[9], const double (&t)[3],
                         const double (&Rn)[9], const double (&tn)[3], const double (&xi)[6], bool robust, double tau, double s2, double lam,
                         double *red, double *S)
{
    double cs = 0.0, ce = 0.0, bad = 0.0, step = 0.0;
    const double is2 = 1.0 / s2;
    for (int i = threadIdx.x; i < it.n; i += kRefineThreads) {
        double X[3];
        float2 o[4];
        ba_load<V2>(it, Xc, i, X, o);
        const bool act = it.flags[i] != 0;
        if (act) {
            BaPoint<V2> p;
            ba_eval<V2>(a, X, R, t, o, p);                  // (an active point is projectable at the accepted estimate)
            double w, rho;
            refine_huber(robust, ba_chi<V2>(p, s2), tau, w, rho);
            BaSys s;
            ba_system<V2, false>(p, R, w * is2, lam, s, nullptr);
            double z[3];
            for (int j = 0; j < 3; j++) {
                double v = s.T[0][j] * xi[0];
#pragma unroll
                for (int q = 1; q < 6; q++) v += s.T[q][j] * xi[q];
                z[j] = s.y[j] + v;
            }
            double dX[3];
            refine_back3(s.L, z, s.ok, dX);
            for (int k = 0; k < 3; k++) X[k] = X[k] + dX[k];
            step = fmax(step, (dX[0] * dX[0] + dX[1] * dX[1]) + dX[2] * dX[2]);
        }
        for (int k = 0; k < 3; k++) Xt[3 * (int64_t)i + k] = X[k];
        if (!act) continue;
        BaPoint<V2> pn;
        ba_eval<V2>(a, X, Rn, tn, o, pn);
        if (!pn.proj) { bad += 1.0; continue; }
        double w, rho;
        refine_huber(robust, ba_chi<V2>(pn, s2), tau, w, rho);
        refine_dd_add(cs, ce, rho, 0.0);
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    __syncthreads();
    bad = wave_allsum_f64(bad);
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) step = fmax(step, __shfl_xor(step, m, 64));
    if (lane == 0) { red[wave * kBaAcc + kBaBad] = bad; red[wave * kBaAcc + kBaStep] = step; }
    refine_wave_cost(cs, ce);
    if (lane == 0) { red[wave * kBaAcc] = cs; red[wave * kBaAcc + kBaCostLo] = ce; }
    __syncthreads();
    if (threadIdx.x == 0) {
        refine_block_cost(red, kBaAcc, kBaCostLo, 4, S[0], S[kBaCostLo]);
        S[kBaBad] = ((red[kBaBad] + red[kBaAcc + kBaBad]) + red[2 * kBaAcc + kBaBad]) + red[3 * kBaAcc + kBaBad];
        S[kBaStep] = fmax(fmax(red[kBaStep], red[kBaAcc + kBaStep]), fmax(red[2 * kBaAcc + kBaStep], red[3 * kBaAcc + kBaStep]));
    }
    __syncthreads();
}

template <int V2>
__global__ __launch_bounds__(kRefineThreads) __attribute__((amdgpu_waves_per_eu(2, 2))) void pose_ba_kernel(BaArgs a)
{
    __shared__ double red[4 * kBaAcc];
    __shared__ double S[kBaAcc], Sn[kBaAcc];                // the sums at the accepted estimate; the trial's cost, bad count, step
    const int tid = threadIdx.x, b = blockIdx.x;
    svo_refine_result *res = a.c.res + b;
    BaItem it;
    it.flags = a.c.flags + (int64_t)b * a.c.flag_stride;
    it.X3 = a.X3 + (int64_t)b * a.stride * 3;
    it.x1l = a.x1l + (int64_t)b * a.stride; it.x1r = a.x1r + (int64_t)b * a.stride; it.x2l = a.x2l + (int64_t)b * a.stride;
    it.x2r = V2 == 2 ? a.x2r + (int64_t)b * a.stride : nullptr;
    double *const X_out = a.Xa + (int64_t)b * a.x_stride * 3;
    double *Xc = X_out, *Xt = a.Xb + (int64_t)b * a.x_stride * 3;
    double R[9], t[3], rv0[3];
    int n = a.c.n_fixed;
    bool skip = false;
    if (a.c.pnp) {
        const PnpRecord &q = a.c.pnp[b];
        for (int i = 0; i < 9; i++) R[i] = q.R[i];
        for (int i = 0; i < 3; i++) { t[i] = q.tvec[i]; rv0[i] = q.rvec[i]; }
        n = q.n;
        skip = q.ok == 0;                                   // solvePnPRansac failed (no model, or fewer points than one needs)
    } else {
        for (int i = 0; i < 3; i++) { t[i] = a.c.tvec0[i]; rv0[i] = a.c.rvec0[i]; }
        refine_rodrigues(rv0, R);
    }
    n = n < 0 ? 0 : (n > a.c.cap ? a.c.cap : n);
    it.n = n;
    for (int i = tid; i < n; i += kRefineThreads)           // every X_i starts at its triangulation
        for (int k = 0; k < 3; k++) Xc[3 * (int64_t)i + k] = (double)it.X3[3 * i + k];
    if (skip) {
        for (int i = tid; i < n; i += kRefineThreads) it.flags[i] = 0;
        if (tid == 0) {
            for (int i = 0; i < 3; i++) { res->rvec[i] = rv0[i]; res->tvec[i] = t[i]; res->pnp_rvec[i] = rv0[i]; res->pnp_tvec[i] = t[i]; }
            for (int i = 0; i < 9; i++) res->R[i] = R[i];
            for (int i = 0; i < 36; i++) res->info[i] = 0.0;
            res->cost_first = 0.0; res->cost_last = 0.0;
            res->n_points = n; res->n_active = 0; res->iters = 0; res->views = V2; res->status = SVO_REFINE_SKIPPED; res->_pad = 0;
        }
        return;
    }
    const double tau = V2 == 2 ? 11.070 : 7.815;            // chi-square 95 % points, d - 3 = 5 and 3 degrees of freedom
    const double s2 = a.c.sigma * a.c.sigma;
    int total = 0;
    double cost_first = 0.0, cost = 0.0, cost_lo = 0.0;
    for (int rd = 0; rd < a.c.rounds; rd++) {
        const bool robust = rd < 2;
        double lam = 1e-4;
        for (int k = 0; k < a.c.iters; k++) {
            total++;
            ba_build<V2>(a, it, Xc, R, t, k > 0 ? kBaKeep : (rd == 0 ? kBaInit : kBaReclass), robust, tau, s2, lam, red, S);
            if (k == 0) {
                cost = S[0]; cost_lo = S[kBaCostLo];
                if (rd == 0) cost_first = cost;
            }
            double A[36], g[6], xi[6];
            {
                int q = 1;
                for (int p = 0; p < 6; p++)
                    for (int s = p; s < 6; s++) { const double h = S[q++]; A[p * 6 + s] = h; A[s * 6 + p] = h; }
                for (int p = 0; p < 6; p++) { g[p] = -S[kBaG + p]; A[p * 6 + p] = A[p * 6 + p] + lam * S[kBaDiag + p]; }
            }
            bool accepted = false;
            double Rn[9], tn[3];
            if (refine_chol6(A, g, xi)) {
                double E[9], Vr[3], Et[3];
                refine_se3_exp(xi, E, Vr);
                refine_mm3(E, R, Rn);
                refine_mv3(E, t, Et);
                for (int i = 0; i < 3; i++) tn[i] = Et[i] + Vr[i];
                ba_trial<V2>(a, it, Xc, Xt, R, t, Rn, tn, xi, robust, tau, s2, lam, red, Sn);
                accepted = Sn[kBaBad] == 0.0 && (Sn[0] < cost || (Sn[0] == cost && Sn[kBaCostLo] < cost_lo));
            }
            if (accepted) {
                for (int i = 0; i < 9; i++) R[i] = Rn[i];
                for (int i = 0; i < 3; i++) t[i] = tn[i];
                { double *sw = Xc; Xc = Xt; Xt = sw; }       // the trial points are the accepted ones now
                cost = Sn[0]; cost_lo = Sn[kBaCostLo];
                lam = lam / 10.0 > 1e-12 ? lam / 10.0 : 1e-12;
                double nx = xi[0] * xi[0];
                for (int i = 1; i < 6; i++) nx += xi[i] * xi[i];
                if (sqrt(nx) < 1e-10 && sqrt(Sn[kBaStep]) < 1e-9) break;
            } else {
                lam *= 10.0;
                if (lam > 1e10) break;
            }
        }
    }
    // the last re-classification; info = the reduced H at lam = 0 over the active set; the outcome (R7)
    ba_build<V2>(a, it, Xc, R, t, kBaReclass, false, tau, s2, 0.0, red, S);
    double info[36], zero[6] = {0, 0, 0, 0, 0, 0}, dummy[6], rv[3];
    {
        int q = 1;
        for (int p = 0; p < 6; p++)
            for (int s = p; s < 6; s++) { const double h = S[q++]; info[p * 6 + s] = h; info[s * 6 + p] = h; }
    }
    const int n_active = (int)S[kBaCount];
    refine_so3_log(R, rv);
    bool fin = refine_finite(cost_first) && refine_finite(cost);
    for (int i = 0; i < 9; i++) fin = fin && refine_finite(R[i]);
    for (int i = 0; i < 3; i++) fin = fin && refine_finite(t[i]) && refine_finite(rv[i]);
    for (int i = 0; i < 36; i++) fin = fin && refine_finite(info[i]);
    const bool pd = refine_chol6(info, zero, dummy);
    const bool applied = n_active >= a.c.min_inliers && pd && fin;
    // the points that stand, at the front buffer: the accepted ones, or the triangulation again when the PnP pose is kept
    if (!applied) {
        for (int i = tid; i < n; i += kRefineThreads)
            for (int k = 0; k < 3; k++) X_out[3 * (int64_t)i + k] = (double)it.X3[3 * i + k];
    } else if (Xc != X_out) {
        for (int i = tid; i < n; i += kRefineThreads)
            for (int k = 0; k < 3; k++) X_out[3 * (int64_t)i + k] = Xc[3 * (int64_t)i + k];
    }
    if (tid == 0) {
        double R0[9], t0[3];
        if (a.c.pnp) {
            const PnpRecord &q = a.c.pnp[b];
            for (int i = 0; i < 9; i++) R0[i] = q.R[i];
            for (int i = 0; i < 3; i++) { t0[i] = q.tvec[i]; rv0[i] = q.rvec[i]; }
        } else {
            for (int i = 0; i < 3; i++) { t0[i] = a.c.tvec0[i]; rv0[i] = a.c.rvec0[i]; }
            refine_rodrigues(rv0, R0);
        }
        for (int i = 0; i < 3; i++) {
            res->pnp_rvec[i] = rv0[i]; res->pnp_tvec[i] = t0[i];
            res->rvec[i] = applied ? rv[i] : rv0[i]; res->tvec[i] = applied ? t[i] : t0[i];
        }
        for (int i = 0; i < 9; i++) res->R[i] = applied ? R[i] : R0[i];
        for (int i = 0; i < 36; i++) res->info[i] = info[i];
        res->cost_first = cost_first; res->cost_last = cost;
        res->n_points = n; res->n_active = n_active; res->iters = total; res->views = V2;
        res->status = applied ? SVO_REFINE_APPLIED : SVO_REFINE_KEPT_PNP; res->_pad = 0;
        if (applied && a.c.pnp) {
            // the gates, T_rel_inv and the chain (finalize_*_kernel) read the pair's PnP record: they see the adjusted pose
            PnpRecord &q = a.c.pnp[b];
            for (int i = 0; i < 3; i++) { q.rvec[i] = rv[i]; q.tvec[i] = t[i]; }
            for (int i = 0; i < 9; i++) q.R[i] = R[i];
        }
    }
}

// ---- the mode's device block, beside the stage's (refine_cut): [Xa x (B + 1) x cap x 3 doubles][Xb, the same][stage-call t1
// observations, left and right, x cap]; item B is the stage call's.  48 bytes x (max_batch + 1) x max_keypoints + 16 bytes x
// max_keypoints.
struct BaCut { size_t Xb, x1l, x1r, end; };
static BaCut ba_cut(const svo_config &c)
{
    const size_t items = (size_t)c.max_batch + 1, cap = (size_t)c.max_keypoints;
    BlockCut cut;
    cut.add(sizeof(double) * 3 * cap * items);              // Xa, at the front
    BaCut r;
    r.Xb = cut.add(sizeof(double) * 3 * cap * items);
    r.x1l = cut.add(sizeof(float2) * cap); r.x1r = cut.add(sizeof(float2) * cap); r.end = cut.total();
    return r;
}

int ba_alloc(svo_ctx *ctx)
{
    SVO_TRY(refine_alloc(ctx));                             // the records, the flags and the stage call's X / t2 scratch are the stage's
    if (ctx->ba_buf) return SVO_OK;
    SVO_HIP(hipSetDevice(ctx->device));
    uint8_t *p = nullptr;
    if (dev_alloc(ctx, &p, ba_cut(ctx->cfg).end) != SVO_OK) return SVO_ERR_HIP;
    ctx->ba_buf = p;                                        // (written before it is read: the kernel starts every point at its triangulation)
    return SVO_OK;
}

static void ba_fill(const svo_ctx *ctx, BaArgs &a)
{
    a.Xa = (double *)ctx->ba_buf; a.Xb = (double *)(ctx->ba_buf + ba_cut(ctx->cfg).Xb);
    a.x_stride = ctx->cfg.max_keypoints;
}

void launch_ba_batch(svo_ctx *ctx, int n_pairs, hipStream_t st)
{
    BaArgs a{};
    refine_fill(ctx, a.c, ctx->cfg.P1, ctx->cfg.P2);
    ba_fill(ctx, a);
    const bool four = ctx->cfg.track_mode == SVO_MODE_LK;      // ORB mode has no t2_right (zeros): three views
    a.X3 = ctx->X3; a.x1l = ctx->cmp[0]; a.x1r = ctx->cmp[1]; a.x2l = ctx->cmp[3]; a.x2r = four ? ctx->cmp[2] : nullptr;
    a.stride = ctx->cfg.max_keypoints;
    a.c.pnp = (PnpRecord *)ctx->pnp_ws;
    if (four) hipLaunchKernelGGL(pose_ba_kernel<2>, dim3(n_pairs), dim3(kRefineThreads), 0, st, a);
    else hipLaunchKernelGGL(pose_ba_kernel<1>, dim3(n_pairs), dim3(kRefineThreads), 0, st, a);
}

int stage_refine_ba(svo_ctx *ctx, const svo_pt3f *obj, const svo_pt2f *img1_left, const svo_pt2f *img1_right, const svo_pt2f *img2_left,
                    const svo_pt2f *img2_right, int n, const double P1[12], const double P2[12], const double rvec0[3],
                    const double tvec0[3], svo_refine_result *res, uint8_t *active, double *X_out, int mem)
{
    SVO_ARG(P1 && P2 && rvec0 && tvec0 && res, "null pointer");
    SVO_ARG(n >= 0 && n <= ctx->cfg.max_keypoints, "n exceeds max_keypoints");
    SVO_ARG(mem == SVO_MEM_HOST || mem == SVO_MEM_DEVICE, "bad mem");
    SVO_ARG(n == 0 || (obj && img1_left && img1_right && img2_left), "null pointer");
    SVO_TRY(ba_alloc(ctx));
    SVO_HIP(hipSetDevice(ctx->device));
    const bool four = img2_right != nullptr;
    BaArgs a{};
    refine_fill_stage(ctx, a.c, P1, P2, n, rvec0, tvec0);
    ba_fill(ctx, a);
    const size_t own = (size_t)ctx->cfg.max_batch * ctx->cfg.max_keypoints * 3;      // item max_batch is the stage call's
    a.Xa += own; a.Xb += own; a.x_stride = 0;
    const RefineCut o = refine_cut(ctx->cfg);
    const BaCut ob = ba_cut(ctx->cfg);
    SVO_TRY(to_device(ctx, (const float *)obj, (float *)(ctx->refine_buf + o.X), (size_t)3 * n, mem, &a.X3));
    SVO_TRY(to_device(ctx, (const float2 *)img1_left, (float2 *)(ctx->ba_buf + ob.x1l), (size_t)n, mem, &a.x1l));
    SVO_TRY(to_device(ctx, (const float2 *)img1_right, (float2 *)(ctx->ba_buf + ob.x1r), (size_t)n, mem, &a.x1r));
    SVO_TRY(to_device(ctx, (const float2 *)img2_left, (float2 *)(ctx->refine_buf + o.xl), (size_t)n, mem, &a.x2l));
    if (four) SVO_TRY(to_device(ctx, (const float2 *)img2_right, (float2 *)(ctx->refine_buf + o.xr), (size_t)n, mem, &a.x2r));
    if (mem == SVO_MEM_DEVICE && active) a.c.flags = active;
    if (four) hipLaunchKernelGGL(pose_ba_kernel<2>, dim3(1), dim3(kRefineThreads), 0, ctx->stream, a);
    else hipLaunchKernelGGL(pose_ba_kernel<1>, dim3(1), dim3(kRefineThreads), 0, ctx->stream, a);
    SVO_HIP(hipGetLastError());
    SVO_TRY(from_device(ctx, X_out, (const double *)a.Xa, (size_t)3 * n, mem));
    return refine_stage_finish(ctx, a.c, n, res, active, mem);
}

// the points of pair `pair` of the last fused launch, which ran in SVO_REFINE_BA mode; the caller has ordered the pose stage
// before the context's stream
int ba_read_points(svo_ctx *ctx, int pair, double *X, int cap, int *n_out)
{
    svo_refine_result *h;
    SVO_TRY(refine_fetch_record(ctx, pair, X, cap, "point capacity too small", &h, n_out));
    const int n = h->n_points;
    if (!X || n == 0) return SVO_OK;
    SVO_TRY(from_device(ctx, X, (const double *)ctx->ba_buf + (size_t)pair * ctx->cfg.max_keypoints * 3, (size_t)3 * n, SVO_MEM_HOST));
    return io_done(ctx, SVO_MEM_HOST);
}

}  // namespace svo
