// keyframe.hip -- keyframe-relative pose on the online chain over carried LK tracks (svo_set_keyframe / svo_keyframe_join).
// The chain keeps a table (id, X) of the points triangulated at a keyframe; every step joins the table with the pair's tracks
// by id, solves solvePnPRansac on the joined lists and, where the solve passes the pair's own gates, reports the pose it gives
// instead of the chained one.  The rules (K1-K8 of include/svo_abi.h):
//
//   join    : tracks in ascending order whose id has a table row -> (X[row], t2_left[track]), (track, row)
//   solve   : n_join >= min_tracks: the pair's solvePnPRansac on the joined lists (item 1 of the pose workspace)
//   accept  : r.ok, solve ok, inlier rate, and F = ([R t] inv_K) pose_a passes the rotation gate and the upper motion gate
//   apply   : r.pose = pose_K inverse([R t])
//   switch  : r.ok and (no keyframe, or not applied, or gap >= max_gap): frame a becomes the keyframe, the table the pair's
//             finite triangulations
//
// Two kernels, one workgroup of 1024 lanes each; they run once per step on a few thousand points and nothing here is tuned.
#include <cmath>
#include <cstring>
#include "abi_io.h"
#include "keyframe.h"
#include "pose_device.h"
#include "svo_device.h"

namespace svo {

// K2.  A lane takes a track and binary-searches the id column, which goes through LDS kKfTrip rows at a time (a table that
// fits one trip is staged once); the hits leave in track order through block1024_ballot_rank (a ballot per wave and the waves' totals).
__global__ __launch_bounds__(1024) void keyframe_join_kernel(KeyframeJoinArgs a)
{
    __shared__ long long s_ids[kKfTrip];
    __shared__ int wave_tot[16];
    const int tid = threadIdx.x;
    const bool valid = !a.clear && (!a.valid || *a.valid != 0);
    int n_rows = a.tab_n ? *a.tab_n : a.n_rows;
    n_rows = !valid || n_rows < 0 ? 0 : (n_rows > a.rows_cap ? a.rows_cap : n_rows);
    int n_trk = a.trk_n ? *a.trk_n : a.n_trk;
    n_trk = n_trk < 0 ? 0 : (n_trk > a.trk_cap ? a.trk_cap : n_trk);
    const bool one_trip = n_rows <= kKfTrip;
    if (one_trip) {
        for (int k = tid; k < n_rows; k += 1024) s_ids[k] = a.tab_ids[k];
        __syncthreads();
    }
    int n_out = 0;
    for (int start = 0; start < n_trk; start += 1024) {
        const int i = start + tid;
        const bool in = i < n_trk;
        const long long id = in ? a.trk_ids[i] : 0;
        int row = -1;
        for (int r0 = 0; r0 < n_rows; r0 += kKfTrip) {
            const int cnt = min(kKfTrip, n_rows - r0);
            if (!one_trip) {
                __syncthreads();                           // the previous trip has been searched
                for (int k = tid; k < cnt; k += 1024) s_ids[k] = a.tab_ids[r0 + k];
                __syncthreads();
            }
            if (in && row < 0 && id >= s_ids[0] && id <= s_ids[cnt - 1]) {
                int lo = 0, hi = cnt - 1;                  // the first entry >= id
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (s_ids[mid] < id) lo = mid + 1; else hi = mid;
                }
                if (s_ids[lo] == id) row = r0 + lo;
            }
        }
        const bool hit = row >= 0;
        int tot;
        const int dst = n_out + block1024_ballot_rank(hit, wave_tot, tot);
        if (hit && dst < a.out_cap) {
            a.o_X[3 * (int64_t)dst] = a.tab_X[3 * (int64_t)row];
            a.o_X[3 * (int64_t)dst + 1] = a.tab_X[3 * (int64_t)row + 1];
            a.o_X[3 * (int64_t)dst + 2] = a.tab_X[3 * (int64_t)row + 2];
            a.o_xy[dst] = a.trk_xy[i];
            a.o_trk[dst] = i; a.o_row[dst] = row;
            if (a.o_id) a.o_id[dst] = id;
        }
        n_out += tot;
    }
    if (tid == 0) {
        const int n_join = min(n_out, a.out_cap);
        a.counts[0] = n_join;
        if (a.min_tracks > 0) a.counts[1] = valid && n_join >= a.min_tracks ? n_join : 0;
    }
}

void launch_keyframe_join(const KeyframeJoinArgs &a, hipStream_t st)
{
    hipLaunchKernelGGL(keyframe_join_kernel, dim3(1), dim3(1024), 0, st, a);
}

// K4-K6.  Lane 0 decides -- the gates on the implied motion, the composition, the switch (pose_device.h) -- and writes the result record; on a
// switch all lanes rebuild the table from the pair's lists (the same ballot rank keeps the list order).
__global__ __launch_bounds__(1024) void keyframe_update_kernel(KeyframeUpdateArgs a)
{
    __shared__ int wave_tot[16];
    __shared__ int s_switch;
    const int tid = threadIdx.x;
    KfState *S = a.state;
    if (tid == 0) {
        const bool valid = !a.clear && S->valid != 0;
        svo_step_result *r = a.rec;
        const PnpRecord &q = *a.pnp;
        const int n_join = a.counts[0];
        const bool solved = valid && n_join >= a.min_tracks;
        svo_keyframe_result out;
        out.switched = 0; out._pad = 0;
        out.kf_index = valid ? S->kf_index : -1;
        out.gap = valid ? a.index_b - S->kf_index : 0;
        out.n_rows = valid ? S->n_rows : 0;
        out.n_join = n_join;
        out.n_inliers = solved ? q.n_inliers : 0; out.ransac_iters = solved ? q.ransac_iters : 0; out.lm_iters = solved ? q.lm_iters : 0;
        for (int i = 0; i < 3; i++) { out.rvec[i] = solved ? q.rvec[i] : 0.0; out.tvec[i] = solved ? q.tvec[i] : 0.0; }
        for (int i = 0; i < 16; i++) { out.pose_K[i] = valid ? S->pose_K[i] : 0.0; out.pose_pair[i] = r->pose[i]; }
        int status;
        if (!valid) status = SVO_KF_NONE;
        else if (!solved) status = SVO_KF_SHORT;
        else if (!r->ok) status = SVO_KF_PAIR_FAILED;
        else {
            status = SVO_KF_REJECTED;
            if (q.ok && !((double)q.n_inliers / (double)n_join < a.inlier_rate)) {
                double M[16], A[16], F[16];
                for (int i = 0; i < 3; i++) {
                    for (int j = 0; j < 3; j++) M[i * 4 + j] = q.R[i * 3 + j];
                    M[i * 4 + 3] = q.tvec[i];
                }
                M[12] = 0; M[13] = 0; M[14] = 0; M[15] = 1;
                pose_mul4(M, S->inv_K, A);
                pose_mul4(A, a.pose_a, F);
                if (pose_euler_gate(F, 4) && pose_norm2_t(F + 3, 4) < a.max_move2) {
                    status = SVO_KF_APPLIED;
                    double Ti[16], P[16];
                    pose_inv_rt(q.R, q.tvec, Ti);
                    pose_mul4(S->pose_K, Ti, P);
                    for (int i = 0; i < 16; i++) r->pose[i] = P[i];
                }
            }
        }
        out.status = status;
        const bool sw = r->ok && (!valid || status != SVO_KF_APPLIED || (a.max_gap > 0 && out.gap >= a.max_gap));
        out.switched = sw ? 1 : 0;
        *a.res = out;
        if (sw) {
            S->valid = 1; S->kf_index = a.index_b - 1;
            for (int i = 0; i < 16; i++) S->pose_K[i] = a.pose_a[i];
            pose_inv_t4(a.pose_a, S->inv_K);
        } else if (!valid) {
            S->valid = 0; S->kf_index = -1; S->n_rows = 0;    // K1: the host's clear, made to last
        }
        s_switch = sw ? 1 : 0;
    }
    __syncthreads();
    if (!s_switch) return;
    int n_trk = *a.trk_n;
    n_trk = n_trk < 0 ? 0 : (n_trk > a.cap ? a.cap : n_trk);
    int n_rows = 0;
    for (int start = 0; start < n_trk; start += 1024) {
        const int i = start + tid;
        float x = 0.f, y = 0.f, z = 0.f;
        bool fin = false;
        if (i < n_trk) {
            x = a.tri[3 * (int64_t)i]; y = a.tri[3 * (int64_t)i + 1]; z = a.tri[3 * (int64_t)i + 2];
            fin = isfinite(x) && isfinite(y) && isfinite(z);
        }
        int tot;
        const int rk = block1024_ballot_rank(fin, wave_tot, tot);
        if (fin) {
            const int dst = n_rows + rk;                      // <= i < cap
            a.tab_ids[dst] = a.trk_ids[i];
            a.tab_X[3 * (int64_t)dst] = x; a.tab_X[3 * (int64_t)dst + 1] = y; a.tab_X[3 * (int64_t)dst + 2] = z;
        }
        n_rows += tot;
    }
    if (tid == 0) S->n_rows = n_rows;
}

void launch_keyframe_update(const KeyframeUpdateArgs &a, hipStream_t st)
{
    hipLaunchKernelGGL(keyframe_update_kernel, dim3(1), dim3(1024), 0, st, a);
}

// ---- the fused step (svo_set_keyframe): the chain's state, its table, the joined lists and the result, ONE block
struct KfCut { size_t state, ids, X, j_X, j_xy, j_trk, j_row, j_id, counts, res, end; };
static KfCut keyframe_cut(int kcap)
{
    const size_t K = (size_t)kcap;
    BlockCut cut;
    KfCut c;
    c.state = cut.add(sizeof(KfState));
    c.ids = cut.add(sizeof(long long) * K); c.X = cut.add(sizeof(float) * 3 * K);
    c.j_X = cut.add(sizeof(float) * 3 * K); c.j_xy = cut.add(sizeof(float2) * K); c.j_trk = cut.add(sizeof(int) * K);
    c.j_row = cut.add(sizeof(int) * K); c.j_id = cut.add(sizeof(long long) * K);
    c.counts = cut.add(sizeof(int) * 2); c.res = cut.add(sizeof(svo_keyframe_result));
    c.end = cut.total();
    return c;
}

int keyframe_alloc(svo_ctx *ctx)
{
    if (ctx->kf.buf) return SVO_OK;
    SVO_HIP(hipSetDevice(ctx->device));
    const KfCut c = keyframe_cut(ctx->cfg.max_keypoints);
    uint8_t *p = nullptr;
    if (dev_alloc(ctx, &p, c.end) != SVO_OK) return SVO_ERR_HIP;
    SVO_HIP(hipMemsetAsync(p, 0, c.end, ctx->stream));
    SVO_HIP(hipStreamSynchronize(ctx->stream));
    ctx->kf.buf = p;
    return SVO_OK;
}

// after launch_finalize_chain (and the refinement stage) of an online step, on its stream: join, solve, update
int keyframe_fused_step(svo_ctx *ctx, const double *pose0_host, hipStream_t st)
{
    const int K = ctx->cfg.max_keypoints;
    const KfCut c = keyframe_cut(K);
    uint8_t *s = ctx->kf.buf;
    KfState *state = (KfState *)(s + c.state);
    int *counts = (int *)(s + c.counts);
    KeyframeJoinArgs j{};
    j.tab_ids = (const long long *)(s + c.ids); j.tab_X = (const float *)(s + c.X); j.tab_n = &state->n_rows; j.rows_cap = K;
    j.trk_ids = ctx->carry.trk_id; j.trk_xy = ctx->cmp[3]; j.trk_n = ctx->m_out; j.trk_cap = K;
    j.valid = &state->valid; j.clear = ctx->kf.clear ? 1 : 0;
    j.min_tracks = ctx->kf.min_tracks;
    j.o_X = (float *)(s + c.j_X); j.o_xy = (float2 *)(s + c.j_xy); j.o_trk = (int *)(s + c.j_trk); j.o_row = (int *)(s + c.j_row);
    j.o_id = (long long *)(s + c.j_id);
    j.out_cap = K; j.counts = counts;
    launch_keyframe_join(j, st);
    timing_mark(ctx, "kf_join");
    launch_pnp_item(ctx, 1, j.o_X, j.o_xy, counts + 1, st);
    timing_mark(ctx, "kf_pnp");
    KeyframeUpdateArgs u{};
    u.state = state; u.tab_ids = (long long *)(s + c.ids); u.tab_X = (float *)(s + c.X);
    u.clear = j.clear; u.index_b = ctx->online_frames; u.min_tracks = ctx->kf.min_tracks; u.max_gap = ctx->kf.max_gap; u.cap = K;
    memcpy(u.pose_a, pose_from_host(pose0_host).m, sizeof(u.pose_a));
    u.inlier_rate = ctx->cfg.inlier_rate; u.max_move2 = ctx->cfg.max_move2;
    u.rec = ctx->d_results; u.pnp = pnp_record(ctx, 1); u.counts = counts;
    u.trk_ids = ctx->carry.trk_id; u.tri = ctx->X3; u.trk_n = ctx->m_out;
    u.res = (svo_keyframe_result *)(s + c.res);
    launch_keyframe_update(u, st);
    timing_mark(ctx, "kf_update");
    ctx->kf.clear = false;
    return SVO_OK;
}

// read-backs of the last step (HOST)
int keyframe_read_result(svo_ctx *ctx, svo_keyframe_result *res)
{
    const KfCut c = keyframe_cut(ctx->cfg.max_keypoints);
    SVO_TRY(from_device(ctx, res, (const svo_keyframe_result *)(ctx->kf.buf + c.res), (size_t)1, SVO_MEM_HOST));
    return io_done(ctx, SVO_MEM_HOST);
}

int keyframe_read_matches(svo_ctx *ctx, int64_t *ids, svo_pt3f *X, svo_pt2f *xy, int32_t *trk_index, uint8_t *mask, int cap, int *n_out)
{
    const int K = ctx->cfg.max_keypoints;
    const KfCut c = keyframe_cut(K);
    const uint8_t *s = ctx->kf.buf;
    const int *h;
    SVO_TRY(count_fetch(ctx, 0, s + c.counts, 2));
    SVO_TRY(counts_wait(ctx, &h));
    const int n = h[0], n_solve = h[1];
    SVO_ARG(n >= 0 && n <= K, "corrupt join count");
    *n_out = n;
    if (!ids && !X && !xy && !trk_index && !mask) return SVO_OK;
    SVO_ARG(n <= cap, "match capacity too small");
    SVO_TRY(from_device(ctx, (long long *)ids, (const long long *)(s + c.j_id), (size_t)n, SVO_MEM_HOST));
    SVO_TRY(from_device(ctx, (float *)X, (const float *)(s + c.j_X), (size_t)3 * n, SVO_MEM_HOST));
    SVO_TRY(from_device(ctx, (float2 *)xy, (const float2 *)(s + c.j_xy), (size_t)n, SVO_MEM_HOST));
    SVO_TRY(from_device(ctx, (int *)trk_index, (const int *)(s + c.j_trk), (size_t)n, SVO_MEM_HOST));
    if (mask && n_solve == n) SVO_TRY(from_device(ctx, mask, pnp_inlier_mask(ctx) + (size_t)K, (size_t)n, SVO_MEM_HOST));
    SVO_TRY(io_done(ctx, SVO_MEM_HOST));
    if (mask && n_solve != n) memset(mask, 0, (size_t)n);     // nothing was solved: the workspace holds an older solve's flags
    return SVO_OK;
}

int keyframe_read_table(svo_ctx *ctx, int64_t *ids, svo_pt3f *X, int cap, int *n_out)
{
    const int K = ctx->cfg.max_keypoints;
    const KfCut c = keyframe_cut(K);
    const uint8_t *s = ctx->kf.buf;
    const KfState *state = (const KfState *)(s + c.state);
    const int *h;
    SVO_TRY(count_fetch(ctx, 0, &state->valid, 1));
    SVO_TRY(count_fetch(ctx, 1, &state->n_rows, 1));
    SVO_TRY(counts_wait(ctx, &h));
    const int n = h[0] ? h[1] : 0;
    SVO_ARG(n >= 0 && n <= K, "corrupt table count");
    *n_out = n;
    if (!ids && !X) return SVO_OK;
    SVO_ARG(n <= cap, "table capacity too small");
    SVO_TRY(from_device(ctx, (long long *)ids, (const long long *)(s + c.ids), (size_t)n, SVO_MEM_HOST));
    SVO_TRY(from_device(ctx, (float *)X, (const float *)(s + c.X), (size_t)3 * n, SVO_MEM_HOST));
    return io_done(ctx, SVO_MEM_HOST);
}

// ---- svo_keyframe_join: the join kernel on a caller's arrays
int stage_keyframe_join(svo_ctx *ctx, const int64_t *tab_ids, const svo_pt3f *tab_X, int n_rows, const int64_t *trk_ids,
                        const svo_pt2f *trk_xy, int n_trk, svo_pt3f *out_X, svo_pt2f *out_xy, int32_t *out_trk, int32_t *out_row,
                        int cap, int *n_out, int mem)
{
    SVO_ARG(n_rows >= 0 && n_rows <= (1 << 20) && n_trk >= 0 && n_trk <= (1 << 20), "n_rows / n_trk outside 0..2^20");
    SVO_ARG(n_rows == 0 || (tab_ids && tab_X), "null table");
    SVO_ARG(n_trk == 0 || (trk_ids && trk_xy), "null track list");
    SVO_ARG(cap >= (n_rows < n_trk ? n_rows : n_trk) && cap <= (1 << 20), "cap < min(n_rows, n_trk)");
    SVO_ARG(n_out && (cap == 0 || (out_X && out_xy && out_trk && out_row)), "null output");
    SVO_ARG(mem == SVO_MEM_HOST || mem == SVO_MEM_DEVICE, "mem must be SVO_MEM_HOST or SVO_MEM_DEVICE");
    SVO_HIP(hipSetDevice(ctx->device));
    KeyframeJoinArgs a{};
    a.n_rows = n_rows; a.rows_cap = n_rows; a.n_trk = n_trk; a.trk_cap = n_trk; a.out_cap = cap;
    if (mem == SVO_MEM_DEVICE) {                                  // the caller's arrays and count as they are: no scratch, nothing allocated
        a.tab_ids = (const long long *)tab_ids; a.tab_X = (const float *)tab_X;
        a.trk_ids = (const long long *)trk_ids; a.trk_xy = (const float2 *)trk_xy;
        a.o_X = (float *)out_X; a.o_xy = (float2 *)out_xy; a.o_trk = (int *)out_trk; a.o_row = (int *)out_row;
        a.counts = n_out;
        launch_keyframe_join(a, ctx->stream);
        SVO_HIP(hipGetLastError());
        return SVO_OK;
    }
    const size_t nr = (size_t)n_rows, nt = (size_t)n_trk, nc = (size_t)cap;
    BlockCut cut;
    const size_t o_cnt = cut.add(256);
    const size_t i_ids = cut.add(sizeof(long long) * nr), i_X = cut.add(sizeof(float) * 3 * nr), i_tid = cut.add(sizeof(long long) * nt),
                 i_xy = cut.add(sizeof(float2) * nt);
    const size_t r_X = cut.add(sizeof(float) * 3 * nc), r_xy = cut.add(sizeof(float2) * nc), r_trk = cut.add(sizeof(int) * nc),
                 r_row = cut.add(sizeof(int) * nc);
    if (dev_reserve(ctx, &ctx->kf.stage, cut.total()) != SVO_OK) return SVO_ERR_HIP;
    uint8_t *s = ctx->kf.stage.base;
    SVO_TRY(to_device(ctx, (const long long *)tab_ids, (long long *)(s + i_ids), nr, mem, &a.tab_ids));
    SVO_TRY(to_device(ctx, (const float *)tab_X, (float *)(s + i_X), 3 * nr, mem, &a.tab_X));
    SVO_TRY(to_device(ctx, (const long long *)trk_ids, (long long *)(s + i_tid), nt, mem, &a.trk_ids));
    SVO_TRY(to_device(ctx, (const float2 *)trk_xy, (float2 *)(s + i_xy), nt, mem, &a.trk_xy));
    a.o_X = (float *)(s + r_X); a.o_xy = (float2 *)(s + r_xy); a.o_trk = (int *)(s + r_trk); a.o_row = (int *)(s + r_row);
    a.counts = (int *)(s + o_cnt);
    launch_keyframe_join(a, ctx->stream);
    SVO_HIP(hipGetLastError());
    SVO_TRY(count_read(ctx, a.counts, n_out));
    const size_t n = (size_t)*n_out;
    SVO_TRY(from_device(ctx, (float *)out_X, (const float *)a.o_X, 3 * n, mem));
    SVO_TRY(from_device(ctx, (float2 *)out_xy, (const float2 *)a.o_xy, n, mem));
    SVO_TRY(from_device(ctx, (int *)out_trk, (const int *)a.o_trk, n, mem));
    SVO_TRY(from_device(ctx, (int *)out_row, (const int *)a.o_row, n, mem));
    return io_done(ctx, mem);
}

}  // namespace svo
