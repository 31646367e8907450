// refine.hip -- robust two-view pose refinement after solvePnPRansac for gfx950: what the reference's
// Tracking::G2O_EstimatePose_PnP (src/tracking.cpp:384-426) was prepared to be and never became -- a motion-only bundle
// adjustment in the style of ORB-SLAM2's PoseOptimization.  The arithmetic (rules R1-R7) is stated in include/svo_abi.h and
// DESIGN.md section 5e; tests/_refine_ref.py is its numpy twin, and the expressions below keep its order of operations.
//
// pose_refine_kernel: ONE workgroup of four waves per pair.  Lanes stride the pair's points; every lane keeps 21 + 6 + 1
// double partial sums (upper triangle of H, g, active count) and the cost as a pair; a wave reduction (wave_allsum_f64) and
// a fixed-order sum of the four wave totals through LDS give EVERY thread the same numbers, so the 6 x 6 Cholesky solve, the SE(3) update and all the
// accept / reject / round decisions are computed redundantly in registers and the control flow is workgroup-uniform: three
// barriers per evaluation, none per solve.  The stage is a chain of about rounds x iters dependent evaluate-and-solve steps of
// a few hundred kFLOP each: latency, not arithmetic, so a pair gets the four SIMDs of one CU and no more.
// A point's active flag lives in device memory and is only ever touched by the lane that strides over it.
// The per-view math, the Huber weight and the cost pair are refine_device.h's leaves (all three optimisers use them); the host
// plumbing around a launch (RefineCommon; defined below) is shared with ba.hip.  The kernel keeps its own prologue and epilogue.
#include <cmath>
#include <cstring>
#include "refine_device.h"

namespace svo {

constexpr int kRefAcc = 31;                    // cost, H (21, row-major upper triangle), g (6), active count, cost tail, bad count
constexpr int kRefCount = 28, kRefCostLo = 29, kRefBad = 30;
struct RefineArgs {
    const float *X3; const float2 *xl, *xr; int64_t stride;      // points of item b at + b * stride (xr: two-view launches only)
    RefineCommon c;
};

// One evaluation of a pair's points at (R, t): residuals, c_i, Jacobians (R3, R4), the sums of R5 / R6 over the active set.
//   mode 0: the active set becomes every projectable point (the start of round 0);
//   mode 1: every point is re-classified first -- active iff projectable and c_i <= tau;
//   mode 2: a trial step -- the flags stand; an active point that is no longer projectable is counted (the step is then
//           rejected).
// S (LDS, kRefAcc doubles, complete for every thread when the call returns) receives cost | sum w J^T J (upper triangle) |
// sum w J^T r | the active count | the cost's tail | the count of active points that are not projectable -- H and g NOT yet
// divided by sigma^2.  The totals live in LDS, not in registers: two sets of 31 doubles per thread (the accepted pose's and the
// trial's) on top of the 31 partial sums and the Jacobian rows spilled the two-view kernel to scratch.
enum { kRefInit = 0, kRefReclass = 1, kRefTrial = 2 };
template <int V>
__device__ void refine_pass(const RefineArgs &a, const float *X3, const float2 *xl, const float2 *xr, uint8_t *flags, int n,
                            const double (&R)[9], const double (&t)[3], int mode, bool robust, double tau, double s2, double *red,
                            double *S)
{
    double acc[kRefAcc];
    for (int k = 0; k < kRefAcc; k++) acc[k] = 0.0;
    for (int i = threadIdx.x; i < n; i += kRefineThreads) {
        const double X = (double)X3[3 * i], Yp = (double)X3[3 * i + 1], Z = (double)X3[3 * i + 2];
        double Y[3];
        for (int k = 0; k < 3; k++) Y[k] = ((X * R[k * 3] + Yp * R[k * 3 + 1]) + Z * R[k * 3 + 2]) + t[k];
        double r[2 * V], J[2 * V][6];
        bool proj = true;
#pragma unroll
        for (int v = 0; v < V; v++) {
            double A[2][3];
            proj = refine_project(a.c.cam, v == 1, Y, v == 0 ? xl[i] : xr[i], r + 2 * v, A) && proj;
            refine_pose_row(A[0], Y, J[2 * v]);
            refine_pose_row(A[1], Y, J[2 * v + 1]);
        }
        double c = 0.0;
        if (proj) {
            c = r[0] * r[0];
#pragma unroll
            for (int k = 1; k < 2 * V; k++) c += r[k] * r[k];
            c = c / s2;
        }
        bool act;
        if (mode == kRefInit) act = proj;
        else if (mode == kRefReclass) act = proj && c <= tau;
        else act = flags[i] != 0;
        if (mode != kRefTrial) flags[i] = act ? 1 : 0;
        if (!act) continue;
        if (!proj) { acc[kRefBad] += 1.0; continue; }
        double w, rho;
        refine_huber(robust, c, tau, w, rho);
        refine_dd_add(acc[0], acc[kRefCostLo], rho, 0.0);
        acc[kRefCount] += 1.0;
        int q = 1;
#pragma unroll
        for (int p = 0; p < 6; p++)
#pragma unroll
            for (int s = p; s < 6; s++) {
                double jj = J[0][p] * J[0][s];
#pragma unroll
                for (int k = 1; k < 2 * V; k++) jj += J[k][p] * J[k][s];
                acc[q++] += w * jj;
            }
#pragma unroll
        for (int p = 0; p < 6; p++) {
            double jr = J[0][p] * r[0];
#pragma unroll
            for (int k = 1; k < 2 * V; k++) jr += J[k][p] * r[k];
            acc[q++] += w * jr;
        }
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    __syncthreads();                                        // `red` and S may still be read from the previous pass
    for (int k = 1; k < kRefAcc; k++) {
        if (k == kRefCostLo) continue;
        const double ws = wave_allsum_f64(acc[k]);
        if (lane == 0) red[wave * kRefAcc + k] = ws;
    }
    double cs = acc[0], ce = acc[kRefCostLo];
    refine_wave_cost(cs, ce);
    if (lane == 0) { red[wave * kRefAcc] = cs; red[wave * kRefAcc + kRefCostLo] = ce; }
    __syncthreads();
    const int k = threadIdx.x;
    if (k >= 1 && k < kRefAcc && k != kRefCostLo) S[k] = ((red[k] + red[kRefAcc + k]) + red[2 * kRefAcc + k]) + red[3 * kRefAcc + k];
    if (k == 0) refine_block_cost(red, kRefAcc, kRefCostLo, 4, S[0], S[kRefCostLo]);
    __syncthreads();
}

template <int V>
__global__ __launch_bounds__(kRefineThreads) __attribute__((amdgpu_waves_per_eu(2, 2))) void pose_refine_kernel(RefineArgs a)
{
    __shared__ double red[4 * kRefAcc];
    __shared__ double tot[2][kRefAcc];                      // the sums at the accepted pose and at the trial pose
    const int tid = threadIdx.x, b = blockIdx.x;
    svo_refine_result *res = a.c.res + b;
    uint8_t *flags = a.c.flags + (int64_t)b * a.c.flag_stride;
    const float *X3 = a.X3 + (int64_t)b * a.stride * 3;
    const float2 *xl = a.xl + (int64_t)b * a.stride;
    const float2 *xr = V == 2 ? a.xr + (int64_t)b * a.stride : nullptr;
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
    if (skip) {
        for (int i = tid; i < n; i += kRefineThreads) flags[i] = 0;
        if (tid == 0) {
            for (int i = 0; i < 3; i++) { res->rvec[i] = rv0[i]; res->tvec[i] = t[i]; res->pnp_rvec[i] = rv0[i]; res->pnp_tvec[i] = t[i]; }
            for (int i = 0; i < 9; i++) res->R[i] = R[i];
            for (int i = 0; i < 36; i++) res->info[i] = 0.0;
            res->cost_first = 0.0; res->cost_last = 0.0;
            res->n_points = n; res->n_active = 0; res->iters = 0; res->views = V; res->status = SVO_REFINE_SKIPPED; res->_pad = 0;
        }
        return;
    }
    const double tau = V == 2 ? 9.488 : 5.991;
    const double s2 = a.c.sigma * a.c.sigma, is2 = 1.0 / s2;
    double *S = tot[0], *Sn = tot[1];
    int total = 0;
    double cost_first = 0.0, cost = 0.0, cost_lo = 0.0;
    for (int rd = 0; rd < a.c.rounds; rd++) {
        const bool robust = rd < 2;
        refine_pass<V>(a, X3, xl, xr, flags, n, R, t, rd == 0 ? kRefInit : kRefReclass, robust, tau, s2, red, S);
        cost = S[0]; cost_lo = S[kRefCostLo];
        if (rd == 0) cost_first = cost;
        double lam = 1e-4;
        for (int it = 0; it < a.c.iters; it++) {
            total++;
            double A[36], g[6], xi[6];
            {
                int q = 1;
                for (int p = 0; p < 6; p++)
                    for (int s = p; s < 6; s++) { const double h = S[q++] * is2; A[p * 6 + s] = h; A[s * 6 + p] = h; }
                for (int p = 0; p < 6; p++) { g[p] = -(S[22 + p] * is2); A[p * 6 + p] = A[p * 6 + p] + lam * A[p * 6 + p]; }
            }
            bool accepted = false;
            double Rn[9], tn[3];
            if (refine_chol6(A, g, xi)) {
                double E[9], Vr[3], Et[3];
                refine_se3_exp(xi, E, Vr);
                refine_mm3(E, R, Rn);
                refine_mv3(E, t, Et);
                for (int i = 0; i < 3; i++) tn[i] = Et[i] + Vr[i];
                refine_pass<V>(a, X3, xl, xr, flags, n, Rn, tn, kRefTrial, robust, tau, s2, red, Sn);
                accepted = Sn[kRefBad] == 0.0 && (Sn[0] < cost || (Sn[0] == cost && Sn[kRefCostLo] < cost_lo));
            }
            if (accepted) {
                for (int i = 0; i < 9; i++) R[i] = Rn[i];
                for (int i = 0; i < 3; i++) t[i] = tn[i];
                { double *sw = S; S = Sn; Sn = sw; }         // the trial's sums are the accepted pose's now
                cost = S[0]; cost_lo = S[kRefCostLo];
                lam = lam / 10.0 > 1e-12 ? lam / 10.0 : 1e-12;
                double nx = xi[0] * xi[0];
                for (int i = 1; i < 6; i++) nx += xi[i] * xi[i];
                if (sqrt(nx) < 1e-10) break;
            } else {
                lam *= 10.0;
                if (lam > 1e10) break;
            }
        }
    }
    // R7: the last re-classification, the information matrix over the active set, the outcome
    refine_pass<V>(a, X3, xl, xr, flags, n, R, t, kRefReclass, false, tau, s2, red, S);
    double info[36], zero[6] = {0, 0, 0, 0, 0, 0}, dummy[6], rv[3];
    {
        int q = 1;
        for (int p = 0; p < 6; p++)
            for (int s = p; s < 6; s++) { const double h = S[q++] / s2; info[p * 6 + s] = h; info[s * 6 + p] = h; }
    }
    const int n_active = (int)S[kRefCount];
    refine_so3_log(R, rv);
    bool fin = refine_finite(cost_first) && refine_finite(cost);
    for (int i = 0; i < 9; i++) fin = fin && refine_finite(R[i]);
    for (int i = 0; i < 3; i++) fin = fin && refine_finite(t[i]) && refine_finite(rv[i]);
    for (int i = 0; i < 36; i++) fin = fin && refine_finite(info[i]);
    const bool pd = refine_chol6(info, zero, dummy);
    const bool applied = n_active >= a.c.min_inliers && pd && fin;
    if (tid == 0) {
        // the start pose again, from where it came (kept in registers through the rounds it cost the two-view kernel its second wave per SIMD)
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
        res->n_points = n; res->n_active = n_active; res->iters = total; res->views = V;
        res->status = applied ? SVO_REFINE_APPLIED : SVO_REFINE_KEPT_PNP; res->_pad = 0;
        if (applied && a.c.pnp) {
            // the gates, T_rel_inv and the chain (finalize_*_kernel) read the pair's PnP record: they see the refined pose
            PnpRecord &q = a.c.pnp[b];
            for (int i = 0; i < 3; i++) { q.rvec[i] = rv[i]; q.tvec[i] = t[i]; }
            for (int i = 0; i < 9; i++) q.R[i] = R[i];
        }
    }
}


int refine_alloc(svo_ctx *ctx)
{
    if (ctx->refine_buf) return SVO_OK;
    SVO_HIP(hipSetDevice(ctx->device));
    const size_t bytes = refine_cut(ctx->cfg).end;
    uint8_t *p = nullptr;
    if (dev_alloc(ctx, &p, bytes) != SVO_OK) return SVO_ERR_HIP;
    // (a block that could not be cleared is not used: it stays the context's, to be freed with it)
    // Cleared ON THE CONTEXT'S STREAM and waited for: hipMemset runs on the null stream and may return before the fill has run,
    // and the context's streams are non-blocking, so a stage call's first input copy into this block could be overtaken by it.
    if (hipMemsetAsync(p, 0, bytes, ctx->stream) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) {
        ctx->err = "hipMemset of the refinement block failed";
        return SVO_ERR_HIP;
    }
    ctx->refine_buf = p;
    return SVO_OK;
}

void refine_fill(const svo_ctx *ctx, RefineCommon &c, const double P1[12], const double P2[12])
{
    c.cam = stereo_cam(P1, P2);
    c.rounds = ctx->refine_rounds; c.iters = ctx->refine_iters; c.min_inliers = ctx->refine_min_inliers; c.sigma = ctx->refine_sigma;
    c.cap = ctx->cfg.max_keypoints;
    c.res = (svo_refine_result *)ctx->refine_buf;
    c.flags = ctx->refine_buf + refine_cut(ctx->cfg).flags;
    c.flag_stride = ctx->cfg.max_keypoints;
}

void refine_fill_stage(const svo_ctx *ctx, RefineCommon &c, const double P1[12], const double P2[12], int n, const double rvec0[3],
                       const double tvec0[3])
{
    refine_fill(ctx, c, P1, P2);
    const int B = ctx->cfg.max_batch;                        // item B of the block is the stage call's
    c.res += B;
    c.flags += (size_t)B * ctx->cfg.max_keypoints; c.flag_stride = 0;
    c.n_fixed = n; c.pnp = nullptr;
    for (int i = 0; i < 3; i++) { c.rvec0[i] = rvec0[i]; c.tvec0[i] = tvec0[i]; }
}

int refine_stage_finish(svo_ctx *ctx, const RefineCommon &c, int n, svo_refine_result *res, uint8_t *active, int mem)
{
    svo_refine_result *h;                                    // the record comes back to the host in both memory kinds
    SVO_TRY(pinned_block(ctx, sizeof(*h), &h));
    SVO_TRY(from_device(ctx, h, (const svo_refine_result *)c.res, 1, SVO_MEM_HOST));
    SVO_TRY(from_device(ctx, active, (const uint8_t *)c.flags, (size_t)n, mem));                         // (device: the kernel wrote them)
    SVO_TRY(io_done(ctx, SVO_MEM_HOST));
    memcpy(res, h, sizeof(*res));
    return SVO_OK;
}

int refine_fetch_record(svo_ctx *ctx, int pair, const void *dst, int cap, const char *too_small, svo_refine_result **h, int *n_out)
{
    SVO_TRY(pinned_block(ctx, sizeof(**h), h));
    SVO_TRY(from_device(ctx, *h, (const svo_refine_result *)ctx->refine_buf + pair, 1, SVO_MEM_HOST));
    SVO_TRY(io_done(ctx, SVO_MEM_HOST));
    const int n = (*h)->n_points;
    SVO_ARG(n >= 0 && n <= ctx->cfg.max_keypoints, "corrupt point count");
    if (n_out) *n_out = n;                                  // also when the capacity is too small: what to size dst for
    SVO_ARG(dst == nullptr || n <= cap, too_small);         // nothing else has been written
    return SVO_OK;
}

void launch_refine_batch(svo_ctx *ctx, int n_pairs, hipStream_t st)
{
    RefineArgs a{};
    refine_fill(ctx, a.c, ctx->cfg.P1, ctx->cfg.P2);
    const bool two = ctx->cfg.track_mode == SVO_MODE_LK;       // ORB mode has no t2_right (zeros): view L only
    a.X3 = ctx->X3; a.xl = ctx->cmp[3]; a.xr = two ? ctx->cmp[2] : nullptr; a.stride = ctx->cfg.max_keypoints;
    a.c.pnp = (PnpRecord *)ctx->pnp_ws;
    if (two) hipLaunchKernelGGL(pose_refine_kernel<2>, dim3(n_pairs), dim3(kRefineThreads), 0, st, a);
    else hipLaunchKernelGGL(pose_refine_kernel<1>, dim3(n_pairs), dim3(kRefineThreads), 0, st, a);
}

int stage_refine_pose(svo_ctx *ctx, const svo_pt3f *obj, const svo_pt2f *img_left, const svo_pt2f *img_right, int n, const double P1[12],
                      const double P2[12], const double rvec0[3], const double tvec0[3], svo_refine_result *res, uint8_t *active, int mem)
{
    SVO_ARG(P1 && rvec0 && tvec0 && res, "null pointer");
    SVO_ARG(img_right == nullptr || P2 != nullptr, "img_right without P2");
    SVO_ARG(n >= 0 && n <= ctx->cfg.max_keypoints, "n exceeds max_keypoints");
    SVO_ARG(mem == SVO_MEM_HOST || mem == SVO_MEM_DEVICE, "bad mem");
    SVO_ARG(n == 0 || (obj && img_left), "null pointer");
    SVO_TRY(refine_alloc(ctx));
    SVO_HIP(hipSetDevice(ctx->device));
    const bool two = img_right != nullptr;
    RefineArgs a{};
    refine_fill_stage(ctx, a.c, P1, two ? P2 : nullptr, n, rvec0, tvec0);
    const RefineCut o = refine_cut(ctx->cfg);
    SVO_TRY(to_device(ctx, (const float *)obj, (float *)(ctx->refine_buf + o.X), (size_t)3 * n, mem, &a.X3));
    SVO_TRY(to_device(ctx, (const float2 *)img_left, (float2 *)(ctx->refine_buf + o.xl), (size_t)n, mem, &a.xl));
    if (two) SVO_TRY(to_device(ctx, (const float2 *)img_right, (float2 *)(ctx->refine_buf + o.xr), (size_t)n, mem, &a.xr));
    if (mem == SVO_MEM_DEVICE && active) a.c.flags = active;
    if (two) hipLaunchKernelGGL(pose_refine_kernel<2>, dim3(1), dim3(kRefineThreads), 0, ctx->stream, a);
    else hipLaunchKernelGGL(pose_refine_kernel<1>, dim3(1), dim3(kRefineThreads), 0, ctx->stream, a);
    SVO_HIP(hipGetLastError());
    return refine_stage_finish(ctx, a.c, n, res, active, mem);
}

// the record and the flags of pair `pair` of the last fused launch; the caller has ordered the pose stage before the context's stream
int refine_read_result(svo_ctx *ctx, int pair, svo_refine_result *res, uint8_t *active, int cap, int *n_out)
{
    const svo_config &c = ctx->cfg;
    svo_refine_result *h;
    SVO_TRY(refine_fetch_record(ctx, pair, active, cap, "flag capacity too small", &h, n_out));
    const int n = h->n_points;
    if (res) memcpy(res, h, sizeof(*res));
    if (!active || n == 0) return SVO_OK;
    SVO_TRY(from_device(ctx, active, (const uint8_t *)ctx->refine_buf + refine_cut(c).flags + (size_t)pair * c.max_keypoints, (size_t)n, SVO_MEM_HOST));
    return io_done(ctx, SVO_MEM_HOST);
}

}  // namespace svo
