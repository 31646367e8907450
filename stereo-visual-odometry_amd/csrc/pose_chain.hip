// pose_chain.hip -- the tail of the pose stage, what follows solvePnPRansac (geometry.hip) and the refinement stage on a
// pair's record: the gating / accumulation code of the reference (src/tracking.cpp:305-329, 440-463, :59-68).  The algebra
// -- gates, inverses, products, the cleared record, the one-wave chain -- is pose_device.h's.
//   finalize_chain_kernel   : per pair failure staging, Euler / translation gates, inv([R t; 0 1]); then frame_pose_ *= T^-1
//                             over the batch, skipping failed steps.  One launch of one wave.
//   finalize_streams_kernel : the same gates for the pairs of a stream-set step, pose_s *= T^-1 per stream in the stream store
//   chain_relative_kernel   : the chain alone, on relative motions gathered elsewhere (svo_chain_relative)
#include "abi_io.h"
#include "pose_device.h"

namespace svo {
struct FinalizeArgs {
    const PnpRecord *pnp; const int *n_prev, *n_cur, *n_tracked;   // per pair
    const int *ovf;                // per pair (ORB mode): an image of the pair overflowed a capacity; may be null
    int n_pairs;
    int mode;                      // SVO_MODE_LK checks "< 30 FAST corners" first (src/tracking.cpp:261)
    int cap;                       // max_keypoints: a frame with more corners was truncated -> SVO_FAIL_CAPACITY
    int num_features_tracking; double inlier_rate, min_move2, max_move2;
    svo_step_result *res;
};
__device__ inline void finalize_pair(const FinalizeArgs &a, int p)
{
    svo_step_result r;
    const PnpRecord &q = a.pnp[p];
    step_record_clear(r);
    r.n_prev_kps = a.n_prev[p]; r.n_cur_kps = a.n_cur[p];
    int fail = 0;
    if (r.n_prev_kps > a.cap || r.n_cur_kps > a.cap || (a.ovf && a.ovf[p])) fail = SVO_FAIL_CAPACITY;   // never silently track a truncated set
    else if (a.mode == SVO_MODE_LK && r.n_cur_kps < 30) fail = SVO_FAIL_FEW_KEYPOINTS;     // src/tracking.cpp:261
    else {
        const int m = a.n_tracked[p];
        r.n_tracked = m;
        if (m < a.num_features_tracking) fail = SVO_FAIL_FEW_TRACKS;         // :274
        else {
            r.n_inliers = q.n_inliers; r.ransac_iters = q.ransac_iters; r.lm_iters = q.lm_iters;
            for (int i = 0; i < 3; i++) { r.rvec[i] = q.rvec[i]; r.tvec[i] = q.tvec[i]; }
            for (int i = 0; i < 9; i++) r.R[i] = q.R[i];
            if ((double)q.n_inliers / (double)m < a.inlier_rate) fail = SVO_FAIL_INLIER_RATIO;   // :491
            else if (!pose_euler_gate(q.R, 3)) fail = SVO_FAIL_ROTATION_GATE;                    // :308
            else {
                const double n2 = pose_norm2_t(q.tvec, 1);
                if (!(n2 < a.max_move2 && n2 > a.min_move2)) fail = SVO_FAIL_TRANSL_GATE;        // :311
                else pose_inv_rt(q.R, q.tvec, r.T_rel_inv);
            }
        }
    }
    r.fail_stage = fail;
    r.ok = fail == 0;
    a.res[p] = r;
}

// frame_pose_ = frame_pose_ * T^-1 over consecutive pairs; failed steps are skipped (:59-68).  The seed pose travels BY VALUE
// (callers of svo_track_batch with device results never synchronise).  The gates of every pair, then the chain, in ONE launch of one workgroup (the pose stage ends with it: two launches were
// 10 us of a lone pair's 750).  ONE WAVE (round 6): the launch is queued on the side stream while the NEXT batch's LK grid
// fills the chip; behind lk_sse2_kernel's single-wave workgroups (two a SIMD, all 160 KB of LDS) wave slots come free one at
// a time, and a four-wave workgroup never found four at once until that grid drained -- the poses of a batch arrived up to a
// whole LK launch (20 ms) late (profiles/r06_sse2_timeline_before.csv).  A lone wave takes the first slot that frees; the 256
// pairs of a batch are four trips of finalize_pair instead of one.  The chain is chain_wave_step's, 64 staged records a trip.
constexpr int kFinThreads = 64;
__global__ __launch_bounds__(kFinThreads) void finalize_chain_kernel(FinalizeArgs a, Pose16 pose0, const double *seed_dev)
{
    __shared__ double sT[64 * 16];
    __shared__ int sOk[64];
    for (int p = threadIdx.x; p < a.n_pairs; p += kFinThreads) finalize_pair(a, p);
    __threadfence_block();
    svo_step_result *res = a.res;
    const int n_pairs = a.n_pairs, lane = threadIdx.x & 63, i = (lane >> 2) & 3, j = lane & 3;
    double P = seed_dev ? seed_dev[i * 4 + j] : pose0.m[i * 4 + j];     // device seed: the previous batch's last pose
    for (int base = 0; base < n_pairs; base += 64) {
        const int cnt = min(64, n_pairs - base);
        __syncthreads();
        for (int e = lane; e < cnt * 16; e += 64) sT[e] = res[base + (e >> 4)].T_rel_inv[e & 15];
        if (lane < cnt) sOk[lane] = res[base + lane].ok;
        __syncthreads();
        P = chain_wave_step(P, sT, sOk, cnt, [&](int p) { return res[base + p].pose; });
    }
}

// The pose stage of a stream-set step (svo_streams_step): the pairs of one launch belong to DIFFERENT streams, so nothing is
// chained along the batch.  finalize_pair decides the gates exactly as for a batch; then pose_s = pose_s * T_rel_inv per stream,
// read from and written to the stream store on the device (a queued step depends on no host memory), 16 lanes per stream, four
// streams per wave, one wave per workgroup; each lane's element is pose_mul4_elem, the chain's association order.
// A stream whose first frame this is gets the StereoInit_f2f record (src/tracking.cpp:78-92) instead: detect only, ok = 1.
constexpr int kFinStreams = 4;                          // streams per workgroup
__global__ __launch_bounds__(64) void finalize_streams_kernel(FinalizeArgs a, int item0, StreamTable tab, double *pose_store)
{
    const int g = threadIdx.x >> 4, e = threadIdx.x & 15, i = e >> 2, j = e & 3;
    const int t = blockIdx.x * kFinStreams + g;         // entry of this launch's table
    const int p = item0 + t;                            // item of the step
    const bool live = t < kStreamChunk && p < a.n_pairs;
    const bool init = live && tab.init[t] != 0;
    if (live && e == 0) {
        if (!init) finalize_pair(a, p);
        else {
            svo_step_result r;
            step_record_clear(r);
            r.ok = 1; r.n_cur_kps = a.n_cur[p];
            a.res[p] = r;
        }
    }
    __threadfence_block();
    __syncthreads();                                    // the record lane 0 wrote is visible to the 16 lanes of its stream
    double out = 0;
    if (live) {
        const svo_step_result *r = a.res + p;
        const double *P = pose_store + (size_t)tab.id[t] * 16;
        out = P[e];
        if (!init && r->ok) out = pose_mul4_elem(P[i * 4 + 0], P[i * 4 + 1], P[i * 4 + 2], P[i * 4 + 3], r->T_rel_inv + j);
    }
    __syncthreads();                                    // every lane has read the old pose before any writes the new one
    if (live) {
        a.res[p].pose[e] = out;
        pose_store[(size_t)tab.id[t] * 16 + e] = out;
    }
}

__global__ __launch_bounds__(256) void streams_set_pose_kernel(double *pose_store, int n, Pose16 pose)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k < n * 16) pose_store[k] = pose.m[k & 15];
}

// The same product for relative motions gathered from independently tracked chunks (other launches, contexts or GPUs)
__global__ __launch_bounds__(64) void chain_relative_kernel(const double *T, const int *ok, int n, Pose16 pose0, double *out)
{
    __shared__ double sT[64 * 16];
    __shared__ int sOk[64];
    const int lane = threadIdx.x, i = (lane >> 2) & 3, j = lane & 3;
    double P = pose0.m[i * 4 + j];
    for (int base = 0; base < n; base += 64) {
        const int cnt = min(64, n - base);
        __syncthreads();
        for (int e = lane; e < cnt * 16; e += 64) sT[e] = T[(int64_t)base * 16 + e];
        if (lane < cnt) sOk[lane] = ok[base + lane];
        __syncthreads();
        P = chain_wave_step(P, sT, sOk, cnt, [&](int p) { return out + (int64_t)(base + p) * 16; });
    }
}

int stage_chain_relative(svo_ctx *ctx, const double *T, const int32_t *ok, int n, const double *pose0_host, double *out, int mem)
{
    SVO_ARG(T && ok && out && n >= 0, "null pointer / negative count");
    SVO_ARG(mem == SVO_MEM_HOST || mem == SVO_MEM_DEVICE, "bad mem");
    if (n == 0) return SVO_OK;
    // host operands: one scratch block of the context (device operands: stream-ordered, nothing allocated or waited for)
    const bool host = mem == SVO_MEM_HOST;
    const size_t hn = host ? (size_t)n : 0;
    BlockCut cut;
    const size_t i_T = cut.add(sizeof(double) * 16 * hn), i_ok = cut.add(sizeof(int) * hn), o_P = cut.add(sizeof(double) * 16 * hn);
    if (host && dev_reserve(ctx, &ctx->chain_stage, cut.total()) != SVO_OK) return SVO_ERR_HIP;
    uint8_t *s = ctx->chain_stage.base;
    const double *dT; const int *dOk;
    SVO_TRY(to_device(ctx, T, (double *)(s + i_T), (size_t)16 * n, mem, &dT));
    SVO_TRY(to_device(ctx, (const int *)ok, (int *)(s + i_ok), (size_t)n, mem, &dOk));
    double *dOut = host ? (double *)(s + o_P) : out;
    hipLaunchKernelGGL(chain_relative_kernel, dim3(1), dim3(64), 0, ctx->stream, dT, dOk, n, pose_from_host(pose0_host), dOut);
    SVO_HIP(hipGetLastError());
    SVO_TRY(from_device(ctx, out, (const double *)dOut, (size_t)16 * n, mem));
    return io_done(ctx, mem);
}

// the gates' inputs and settings, from the context: the records solvePnPRansac left, the tracks' counts, the step records
static FinalizeArgs finalize_args_from_ctx(svo_ctx *ctx, int n_pairs, const int *n_prev, const int *n_cur, const int *ovf)
{
    FinalizeArgs f{};
    f.pnp = pnp_record(ctx, 0); f.n_prev = n_prev; f.n_cur = n_cur; f.n_tracked = ctx->m_out; f.ovf = ovf;
    f.cap = ctx->cfg.max_keypoints; f.n_pairs = n_pairs; f.mode = ctx->cfg.track_mode; f.num_features_tracking = ctx->cfg.num_features_tracking;
    f.inlier_rate = ctx->cfg.inlier_rate; f.min_move2 = ctx->cfg.min_move2; f.max_move2 = ctx->cfg.max_move2; f.res = ctx->d_results;
    return f;
}

void launch_finalize_chain(svo_ctx *ctx, int n_pairs, const int *n_prev, const int *n_cur, const int *ovf, const double *pose0_host, hipStream_t st)
{
    hipLaunchKernelGGL(finalize_chain_kernel, dim3(1), dim3(kFinThreads), 0, st, finalize_args_from_ctx(ctx, n_pairs, n_prev, n_cur, ovf),
                       pose_from_host(pose0_host), ctx->seed_dev);
}

void launch_finalize_streams(svo_ctx *ctx, int item0, int n_items, int n_pairs, const int *n_prev, const int *n_cur, const int *ovf,
                             const StreamTable &tab, hipStream_t st)
{
    const int end = item0 + n_items < n_pairs ? item0 + n_items : n_pairs;
    hipLaunchKernelGGL(finalize_streams_kernel, dim3((n_items + kFinStreams - 1) / kFinStreams), dim3(64), 0, st,
                       finalize_args_from_ctx(ctx, end, n_prev, n_cur, ovf), item0, tab, ctx->streams.pose);
}

void launch_streams_set_pose(svo_ctx *ctx, int id0, int n, const double *pose_host)
{
    hipLaunchKernelGGL(streams_set_pose_kernel, dim3((n * 16 + 255) / 256), dim3(256), 0, ctx->stream,
                       ctx->streams.pose + (size_t)id0 * 16, n, pose_from_host(pose_host));
}
}  // namespace svo
