// pipeline.hip -- the fused LK-mode frame step (Tracking::AddFrame -> LK_StereoF2F_PnP_Track,
// reference src/tracking.cpp:49-77, 258-344) as a fixed sequence of batched launches:
//
//   pyramids (L,R of every new frame) -> FAST on every left image -> circular LK chain per point
//   -> stable compaction -> triangulation -> RANSAC-EPnP + LM -> gates -> pose chain
//
// Every consecutive frame pair is independent, so a batch of F frames is
// F-1 pairs processed by ONE launch of each kernel (grid.y / grid.x = pair), with frame f's
// pyramids at bslots[2f], bslots[2f+1] and its keypoints at kp[f]; only the 4x4 pose product is
// sequential.  The online entry point (svo_add_frame) runs the same kernels with one pair on a
// two-frame ring.
#include <cstring>
#include "abi_io.h"
#include "carry.h"
#include "pose_device.h"

namespace svo {

void timing_mark(svo_ctx *ctx, const char *name)
{
    if (!ctx->timing) return;
    if (ctx->ev_used >= 16384) return;                 // bounded log
    if (ctx->ev_used == ctx->ev_pool.size()) {
        hipEvent_t ev = nullptr;
        if (dev_event(ctx, &ev, hipEventDefault) != SVO_OK) return;      // (timing-enabled, unlike every other event of the context)
        ctx->ev_pool.push_back(ev);
    }
    hipEvent_t ev = ctx->ev_pool[ctx->ev_used++];
    (void)hipEventRecord(ev, ctx->stream);
    ctx->marks.emplace_back(name, ev);
}
static inline void mark(svo_ctx *ctx, const char *name) { timing_mark(ctx, name); }

static const char *kTMatch = "orb_match";
static const char *kT0 = "start", *kTPyr = "pyramid", *kTFast = "fast", *kTLk = "lk", *kTCompact = "compact",
                  *kTTri = "triangulate", *kTPnp = "pnp", *kTRefine = "refine", *kTFin = "finalize";

// Builds pyramids of `n_new` frames into frame slots [f0, f0+n_new) and runs FAST on their left
// images.  L/R: device pointers to the first new frame.
static int ingest_frames(svo_ctx *ctx, const uint8_t *L, const uint8_t *R, int pitch, int64_t frame_stride,
                         int f0, int n_new)
{
    if (ctx->cfg.track_mode == SVO_MODE_ORB) {
        // Detect_MyORBFeatures (src/tracking.cpp:502-532): ORBextractor on the left AND right image;
        // frame f -> feature slots 2f (left), 2f+1 (right)
        // (orb_extract_batch records its own stage marks: orb_pyramid, orb_cellfast, orb_quadtree, orb_describe)
        // (level 0 read in place: the frames belong to the caller's batch / the context's staging until the step is done)
        const int rc = orb_extract_batch(ctx, L, R, pitch, frame_stride, 2 * f0, 2 * n_new, ctx->stream, /*in_place*/ true);
        // svo_set_orb_matcher: stage S of the guided matcher while the levels are in the slots and the caller's frames are valid
        if (rc == SVO_OK && ctx->orbm_mode == SVO_ORB_MATCHER_GUIDED) return orbm_stereo_frames(ctx, 2 * f0, n_new, ctx->stream);
        return rc;
    }
    const PyrGeom &g = ctx->geom;
    PyrArgs p{};
    // left and right images interleave into consecutive slots 2f, 2f+1: one launch set for both
    p.g = g; p.pitch = pitch; p.img_stride = frame_stride; p.slot_stride = g.slot_bytes;
    p.img = L; p.img2 = R; p.slots = ctx->bslots + (size_t)(2 * f0) * g.slot_bytes;
    launch_pyramid(p, 2 * n_new, ctx->stream);
    mark(ctx, kTPyr);
    if (ctx->lk_detector == SVO_DETECTOR_GFTT) {
        // svo_set_lk_detector: cv::goodFeaturesToTrack instead of cv::FAST (the buckets and fast_keep_strongest are excluded with it)
        const int rc = gftt_detect_frames(ctx, L, pitch, frame_stride, f0, n_new);
        mark(ctx, kTFast);
        return rc;
    }
    FastArgs a{};
    a.img = L; a.pitch = pitch; a.img_stride = frame_stride;
    a.w = ctx->cfg.width; a.h = ctx->cfg.height; a.thr = ctx->cfg.fast_threshold; a.nms = 1;
    a.score = ctx->score + (size_t)f0 * ctx->score_stride; a.spitch = ctx->spitch; a.score_stride = ctx->score_stride;
    a.rowcount = ctx->rowcount + (size_t)f0 * ctx->rowcount_stride; a.rowcount_stride = ctx->rowcount_stride;
    a.kp_xy = ctx->kp_xy + (size_t)f0 * ctx->cfg.max_keypoints;
    a.kp_resp = ctx->kp_resp + (size_t)f0 * ctx->cfg.max_keypoints;
    a.kp_stride = ctx->cfg.max_keypoints;
    a.n_out = ctx->kp_n + f0; a.cap = ctx->cfg.max_keypoints;
    launch_fast(a, n_new, ctx->stream);
    if (ctx->bucket_keep > 0) {
        // svo_set_fast_buckets: the strongest corners per grid cell, before the global top-N
        BucketArgs k{};
        k.kp_xy = a.kp_xy; k.kp_resp = a.kp_resp; k.kp_stride = a.kp_stride; k.n_out = a.n_out; k.cap = a.cap;
        k.w = a.w; k.h = a.h; k.cw = ctx->bucket_w; k.ch = ctx->bucket_h; k.per_cell = ctx->bucket_keep;
        k.cols = (a.w + k.cw - 1) / k.cw; k.ncells = k.cols * ((a.h + k.ch - 1) / k.ch);
        k.cells_stride = (int64_t)4 * k.ncells;
        k.cells = ctx->bucket_cells.base ? (int *)ctx->bucket_cells.base + (size_t)f0 * k.cells_stride : nullptr;
        launch_fast_buckets(k, n_new, ctx->stream);
    }
    launch_fast_keep_strongest(a, n_new, ctx->cfg.fast_keep_strongest, ctx->stream);
    mark(ctx, kTFast);
    return SVO_OK;
}

// A stream-set step: item i of the launch set works for stream ids[i]; init[i]: that stream has no previous frame.
struct StreamStep { const int32_t *ids; const uint8_t *init; };
// The pose stage of a launch set.  carried: track carry ran on its pairs; os: an online step and the followers it runs.
static int run_back(svo_ctx *ctx, int n_pairs, const double *pose0_host, svo_step_result *results_dev, bool carried,
                    bool triangulate_first = false, const StreamStep *ss = nullptr, const OnlineStep *os = nullptr);
static const char *kTGather = "stream_gather", *kTScatter = "stream_scatter";

// What a frame carries from one step to the next -- the list exists here only.  work[k]: the working array behind segment k (frame
// slot f at work[k] + f * bytes[k]); is_count[k]: a count segment.  carry_last_frame moves them between frame slots, a stream
// set keeps them per stream, in this order (streams_create sizes the store by them).
static int stream_segments(svo_ctx *ctx, uint8_t *work[kMaxSeg], size_t bytes[kMaxSeg], int is_count[kMaxSeg])
{
    const size_t cap = (size_t)ctx->cfg.max_keypoints;
    if (ctx->cfg.track_mode == SVO_MODE_ORB) {
        const size_t kcap = (size_t)ctx->orb_kp_cap;
        work[0] = (uint8_t *)ctx->orb_kps;      bytes[0] = 2 * kcap * sizeof(svo_keypoint); is_count[0] = 0;
        work[1] = ctx->orb_desc;                bytes[1] = 2 * kcap * 32;                   is_count[1] = 0;
        work[2] = (uint8_t *)ctx->orb_n;        bytes[2] = 2 * sizeof(int);                 is_count[2] = 1;
        work[3] = (uint8_t *)ctx->orb_overflow; bytes[3] = 2 * sizeof(int);                 is_count[3] = 1;
        if (ctx->orbm_mode == SVO_ORB_MATCHER_GUIDED) {
            // the guided matcher's frame block: stage S's uR / sad and the patches stage T compares against the next frame
            work[4] = ctx->orbm_frames;         bytes[4] = ctx->orbm_frame_bytes;           is_count[4] = 0;
            return 5;
        }
    } else {
        work[0] = ctx->bslots;                  bytes[0] = (size_t)2 * ctx->geom.slot_bytes; is_count[0] = 0;
        work[1] = (uint8_t *)ctx->kp_xy;        bytes[1] = cap * sizeof(float2);            is_count[1] = 0;
        work[2] = (uint8_t *)ctx->kp_resp;      bytes[2] = cap * sizeof(float);             is_count[2] = 0;
        work[3] = (uint8_t *)ctx->kp_n;         bytes[3] = sizeof(int);                     is_count[3] = 1;
        if (ctx->carry.on) {
            // svo_set_track_carry: the list's ids and ages travel with it
            work[4] = (uint8_t *)ctx->carry.kp_id;    bytes[4] = cap * sizeof(long long);         is_count[4] = 0;
            work[5] = (uint8_t *)ctx->carry.kp_age;   bytes[5] = cap * sizeof(int);               is_count[5] = 0;
            return 6;
        }
    }
    return 4;
}

// ---- track carry (svo_set_track_carry; the kernel and its rules: carry.hip) -------------------------------------------------
static const char *kTCarry = "carry";

int carry_alloc(svo_ctx *ctx)
{
    const size_t cap = (size_t)ctx->cfg.max_keypoints, nf = (size_t)ctx->n_img, np = (size_t)ctx->cfg.max_batch;
    if (!ctx->carry.buf) {
        BlockCut cut;
        const size_t o_next = cut.add(sizeof(long long)), o_id = cut.add(sizeof(long long) * cap * nf), o_age = cut.add(sizeof(int) * cap * nf),
                     o_tid = cut.add(sizeof(long long) * cap * np), o_tage = cut.add(sizeof(int) * cap * np),
                     o_sorted = cut.add(sizeof(int) * cap * np), o_flag = cut.add(cap * np), o_dflag = cut.add(cap * np),
                     o_dxy = cut.add(sizeof(float2) * cap * np), o_dresp = cut.add(sizeof(float) * cap * np);
        uint8_t *s = nullptr;
        if (dev_alloc(ctx, &s, cut.total()) != SVO_OK) return SVO_ERR_HIP;
        SVO_HIP(hipMemsetAsync(s, 0, cut.total(), ctx->stream));
        ctx->carry.next = (long long *)(s + o_next);
        ctx->carry.kp_id = (long long *)(s + o_id); ctx->carry.kp_age = (int *)(s + o_age);
        ctx->carry.trk_id = (long long *)(s + o_tid); ctx->carry.trk_age = (int *)(s + o_tage);
        ctx->carry.sorted = (int *)(s + o_sorted); ctx->carry.flag = s + o_flag; ctx->carry.dflag = s + o_dflag;
        ctx->carry.dxy = (float2 *)(s + o_dxy); ctx->carry.dresp = (float *)(s + o_dresp);
        ctx->carry.buf = s;
    }
    StreamSet &ss = ctx->streams;
    if (ss.n > 0) {
        // the store's share, in whichever order the set and the switch came (a call that failed half way finds what it made)
        const size_t bytes[3] = {cap * sizeof(long long) * (size_t)ss.n + 16, cap * sizeof(int) * (size_t)ss.n + 16, sizeof(long long) * (size_t)ss.n};
        uint8_t **at[3] = {&ss.seg[4], &ss.seg[5], (uint8_t **)&ss.next_id};
        for (int k = 0; k < 3; k++) {
            if (*at[k]) continue;
            if (dev_alloc(ctx, at[k], bytes[k]) != SVO_OK) return SVO_ERR_HIP;
            SVO_HIP(hipMemsetAsync(*at[k], 0, bytes[k], ctx->stream));
        }
        ss.seg_bytes[4] = cap * sizeof(long long); ss.seg_bytes[5] = cap * sizeof(int);
    }
    return SVO_OK;
}

// The carry step of n_pairs pairs (frame slot fp0 + p*fstep -> fc0 + p*fstep), behind the compaction and the count snapshot:
// the new frames' detections become their merged lists, in place.  no_prev: a chain's first frame, which only gets its ids.
static void launch_carry_pairs(svo_ctx *ctx, int n_pairs, int fp0, int fc0, int fstep, const StreamStep *ss, bool no_prev)
{
    const size_t cap = (size_t)ctx->cfg.max_keypoints;
    CarryMergeArgs a{};
    a.w = ctx->cfg.width; a.h = ctx->cfg.height;
    carry_grid(a.w, a.h, ctx->carry.min_distance, &a.cell, &a.cols, &a.rows);
    a.min_d2 = ctx->carry.min_distance * ctx->carry.min_distance;
    a.max_age = ctx->carry.max_age;
    a.cap = a.out_cap = (int)cap;
    a.stride = (int64_t)fstep * (int64_t)cap; a.n_stride = fstep;
    a.q = ctx->pts_out[2]; a.keep = ctx->keep;
    a.p_resp = ctx->kp_resp + (size_t)fp0 * cap; a.p_id = ctx->carry.kp_id + (size_t)fp0 * cap; a.p_age = ctx->carry.kp_age + (size_t)fp0 * cap;
    a.p_n = no_prev ? nullptr : ctx->kp_n + fp0; a.n_trk = 0;
    a.d_xy = ctx->kp_xy + (size_t)fc0 * cap; a.d_resp = ctx->kp_resp + (size_t)fc0 * cap; a.d_n = ctx->kp_n + fc0;
    a.o_xy = ctx->kp_xy + (size_t)fc0 * cap; a.o_resp = ctx->kp_resp + (size_t)fc0 * cap;
    a.o_id = ctx->carry.kp_id + (size_t)fc0 * cap; a.o_age = ctx->carry.kp_age + (size_t)fc0 * cap;
    a.o_n = ctx->kp_n + fc0;
    a.trk_id = ctx->carry.trk_id; a.trk_age = ctx->carry.trk_age;
    a.sorted = ctx->carry.sorted; a.flag = ctx->carry.flag; a.dflag = ctx->carry.dflag; a.s_dxy = ctx->carry.dxy; a.s_dresp = ctx->carry.dresp;
    if (!ss) {
        // the online ring: one pair, one counter
        a.next_id = ctx->carry.next;
        a.fresh[0] = !no_prev && !ctx->carry.ids[fp0 & 1];
        a.restart[0] = ctx->carry.restart;
        ctx->carry.restart = false;
        launch_carry_merge(a, 1, ctx->stream);
        return;
    }
    StreamSet &set = ctx->streams;
    a.next_id = set.next_id;
    for (int i0 = 0; i0 < n_pairs; i0 += kCarryChunk) {
        const int n = n_pairs - i0 < kCarryChunk ? n_pairs - i0 : kCarryChunk;
        a.item0 = i0;
        for (int t = 0; t < n; t++) {
            const size_t id = (size_t)ss->ids[i0 + t];
            a.cnt[t] = (int32_t)id;
            a.fresh[t] = !ss->init[i0 + t] && !set.has_ids[id];     // (an init item has no previous list: the gather left its count 0)
            a.restart[t] = set.restart[id];
            set.restart[id] = 0; set.has_ids[id] = 1;
        }
        launch_carry_merge(a, n, ctx->stream);
    }
}

// A micro-batch of a stream starts with the frame the previous one ended with: instead of building that frame's
// pyramids and detecting its features again, what the pair needs of it is carried from frame slot `last` to slot 0
// (LK mode: the two pyramid slots, the FAST keypoints + responses + count; ORB mode: both images' keypoints, descriptors,
// counts and capacity flags, and with the guided matcher the frame's stereo block) -- ONE launch, 16 bytes per thread.
struct CarryArgs { uint8_t *dst[kMaxSeg]; const uint8_t *src[kMaxSeg]; size_t bytes[kMaxSeg]; int n; };
__global__ __launch_bounds__(256) void carry_frame_kernel(CarryArgs a)
{
    const int seg = blockIdx.y;
    if (seg >= a.n) return;
    const size_t n16 = a.bytes[seg] / 16, rest = a.bytes[seg] - n16 * 16;
    const uint4 *s = (const uint4 *)a.src[seg];
    uint4 *d = (uint4 *)a.dst[seg];
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (size_t)gridDim.x * 256) d[i] = s[i];
    if (blockIdx.x == 0 && threadIdx.x < rest) a.dst[seg][n16 * 16 + threadIdx.x] = a.src[seg][n16 * 16 + threadIdx.x];
}

static void carry_last_frame(svo_ctx *ctx, int last)
{
    CarryArgs c{};
    uint8_t *work[kMaxSeg];
    int is_count[kMaxSeg];
    c.n = stream_segments(ctx, work, c.bytes, is_count);
    for (int k = 0; k < c.n; k++) { c.dst[k] = work[k]; c.src[k] = work[k] + (size_t)last * c.bytes[k]; }
    hipLaunchKernelGGL(carry_frame_kernel, dim3(64, c.n), dim3(256), 0, ctx->stream, c);
}

// The same copy for the streams of a stream set, table-driven: ONE launch moves every carried segment of up to kStreamChunk
// streams between the stream store (segment k of stream s at store[k] + s * bytes[k]) and the working frame slots (segment k of
// frame slot f at work[k] + f * bytes[k]).  Item t of the launch is stream tab.id[t] <-> frame slot slot0 + t.
// Gather (to_store = 0): store -> slot; a stream WITHOUT a previous frame (tab.init[t]) leaves a hole -- its count segments are
// zeroed (no keypoints: the pair tracks nothing and the pose stage writes the init record), the others are not touched.
// Scatter (to_store = 1): slot -> store, every item.  16 bytes per lane where both ends are 16-byte aligned, else 4, else 1.
struct StreamCopyArgs {
    uint8_t *store[kMaxSeg], *work[kMaxSeg];
    size_t bytes[kMaxSeg];
    int is_count[kMaxSeg];
    int n_seg, n_items, slot0, to_store;
    StreamTable tab;
};
__global__ __launch_bounds__(256) void stream_copy_kernel(StreamCopyArgs a)
{
    const int seg = blockIdx.y, t = blockIdx.z;
    if (seg >= a.n_seg || t >= a.n_items || t >= kStreamChunk) return;
    const size_t bytes = a.bytes[seg];
    uint8_t *st = a.store[seg] + (size_t)a.tab.id[t] * bytes;
    uint8_t *wk = a.work[seg] + (size_t)(a.slot0 + t) * bytes;
    const bool hole = !a.to_store && a.tab.init[t];
    if (hole && !a.is_count[seg]) return;
    uint8_t *d = a.to_store ? st : wk;
    const uint8_t *s = a.to_store ? wk : st;
    const size_t tid = (size_t)blockIdx.x * 256 + threadIdx.x, nthr = (size_t)gridDim.x * 256;
    if (hole) {
        for (size_t i = tid; i < bytes; i += nthr) d[i] = 0;
        return;
    }
    const uintptr_t al = (uintptr_t)d | (uintptr_t)s;
    size_t done = 0;
    if ((al & 15) == 0) {
        const size_t n16 = bytes / 16;
        for (size_t i = tid; i < n16; i += nthr) ((uint4 *)d)[i] = ((const uint4 *)s)[i];
        done = n16 * 16;
    } else if ((al & 3) == 0) {
        const size_t n4 = bytes / 4;
        for (size_t i = tid; i < n4; i += nthr) ((uint32_t *)d)[i] = ((const uint32_t *)s)[i];
        done = n4 * 4;
    }
    for (size_t i = done + tid; i < bytes; i += nthr) d[i] = s[i];
}

static void launch_stream_copy(svo_ctx *ctx, const StreamTable &tab, int n_items, int slot0, bool to_store)
{
    StreamCopyArgs a{};
    a.n_seg = stream_segments(ctx, a.work, a.bytes, a.is_count);
    for (int k = 0; k < a.n_seg; k++) a.store[k] = ctx->streams.seg[k];
    a.n_items = n_items; a.slot0 = slot0; a.to_store = to_store ? 1 : 0;
    a.tab = tab;
    // the largest segment (two pyramid slots, ~1.2 MB at KITTI size) in 4 KB workgroup trips: 64 workgroups for a lone stream,
    // fewer per stream as the launch widens (the grid is items x segments x this)
    int gx = 2048 / n_items;
    gx = gx > 64 ? 64 : (gx < 8 ? 8 : gx);
    hipLaunchKernelGGL(stream_copy_kernel, dim3(gx, a.n_seg, n_items), dim3(256), 0, ctx->stream, a);
}

// launch(tab, i0, n) for every chunk of up to kStreamChunk items of a step: tab.id[t] / tab.init[t] are those of item i0 + t
// (init null: none is an init item).
template <class F>
static void for_stream_chunks(const int32_t *ids, const uint8_t *init, int m, F launch)
{
    for (int i0 = 0; i0 < m; i0 += kStreamChunk) {
        const int n = m - i0 < kStreamChunk ? m - i0 : kStreamChunk;
        StreamTable tab{};
        for (int t = 0; t < n; t++) { tab.id[t] = ids[i0 + t]; tab.init[t] = init ? init[i0 + t] : 0; }
        launch(tab, i0, n);
    }
}

// Tracks `n_pairs` pairs; pair p = (frame slot fp0 + p*fstep, frame slot fc0 + p*fstep).
// Front half on the context's stream: circular LK, compaction, triangulation.  Back half (pose
// solver, gates, chain, optional copy of the records to `results_dev`) on `back_stream`, which is
// the context's stream, or -- overlap mode -- the side stream, ordered after the front by an event.
static int run_pairs(svo_ctx *ctx, int n_pairs, int fp0, int fc0, int fstep, const double *pose0_host,
                     svo_step_result *results_dev, const StreamStep *ss = nullptr, const OnlineStep *os = nullptr)
{
    const PyrGeom &g = ctx->geom;
    const int cap = ctx->cfg.max_keypoints;
    if (ctx->cfg.track_mode == SVO_MODE_ORB) {
        // ORB_StereoF2F_PnP_Track (src/tracking.cpp:168-249): Hamming matches + filter instead of LK
        if (ctx->back_pending) {
            SVO_HIP(hipStreamWaitEvent(ctx->stream, ctx->ev_back, 0));
            ctx->back_pending = false;
        }
        if (ctx->orbm_mode == SVO_ORB_MATCHER_GUIDED) {          // svo_set_orb_matcher: stage T writes the same lists
            const int rc = orbm_track_pairs(ctx, n_pairs, fp0, fc0, fstep, ctx->stream);
            if (rc) return rc;
        } else
            orb_match_pairs(ctx, n_pairs, fp0, fc0, fstep, ctx->stream);
        mark(ctx, kTMatch);
        // + n_prev / n_cur = left keypoint counts of the two frames (feature slots 2f) and the capacity flags, frozen for the
        // pose stage by the pairs' begin workgroups
        const SnapSpec snap{(const int *)ctx->orb_n, (const int *)ctx->orb_overflow, fp0, fc0, fstep, 2};
        launch_triangulate_batch(ctx, n_pairs, cap, ctx->cmp[0], ctx->cmp[1], ctx->m_out, 0, &snap);
        mark(ctx, kTTri);
        return run_back(ctx, n_pairs, pose0_host, results_dev, /*carried*/ false, false, ss, os);
    }
    auto S = [&](int slot) { return ctx->bslots + (size_t)slot * g.slot_bytes; };
    LkArgs a{};
    a.g = g; a.ncalls = 4;
    a.slot_stride = (int64_t)fstep * 2 * g.slot_bytes;
    // L1 -> R1 -> R2 -> L2 -> L1'  (src/tracking.cpp:593-618)
    a.prev[0] = S(2 * fp0);     a.next[0] = S(2 * fp0 + 1);
    a.prev[1] = S(2 * fp0 + 1); a.next[1] = S(2 * fc0 + 1);
    a.prev[2] = S(2 * fc0 + 1); a.next[2] = S(2 * fc0);
    a.prev[3] = S(2 * fc0);     a.next[3] = S(2 * fp0);
    // matched_t1_left = the previous frame's FAST keypoints (:268-271), read in place.  Outputs use
    // the same per-item stride (po = b * pts_stride + idx); n_pts is indexed by the batch item, so
    // fstep must be 1 when n_pairs > 1.
    a.pts_in = ctx->kp_xy + (size_t)fp0 * cap; a.pts_stride = (int64_t)fstep * cap;
    a.n_pts = ctx->kp_n + fp0;
    a.n_fixed = 0; a.cap = cap;
    for (int i = 0; i < 4; i++) { a.pts_out[i] = ctx->pts_out[i]; a.status[i] = ctx->status[i]; }
    a.keep = ctx->keep;
    a.match_err = ctx->cfg.feature_match_error;
    a.accum = ctx->cfg.lk_accum;
    launch_lk(a, n_pairs, cap, ctx->stream);
    mark(ctx, kTLk);
    // the previous batch's pose stage (overlap mode) still reads the compacted lists / 3-D points
    if (ctx->back_pending) {
        SVO_HIP(hipStreamWaitEvent(ctx->stream, ctx->ev_back, 0));
        ctx->back_pending = false;
    }
    CompactArgs c{};
    c.keep = ctx->keep; c.n_pts = ctx->kp_n + fp0; c.n_fixed = 0; c.pts_stride = (int64_t)fstep * cap; c.cap = cap;
    c.in[0] = a.pts_in; c.in[1] = ctx->pts_out[0]; c.in[2] = ctx->pts_out[1]; c.in[3] = ctx->pts_out[2];
    for (int i = 0; i < 4; i++) c.out[i] = ctx->cmp[i];
    c.m_out = ctx->m_out;
    launch_compact(c, n_pairs, ctx->stream);
    mark(ctx, kTCompact);
    // triangulatePoints(P1, P2, t1_left, t1_right) (:292-294); the pairs' begin workgroups also freeze the keypoint counts
    // of the frames involved for the pose stage (FAST of the next batch overwrites kp_n): snap[p] = n_prev of pair p,
    // snap[n_pairs + p] = n_cur of pair p
    const SnapSpec snap{ctx->kp_n, nullptr, fp0, fc0, fstep, 1};
    // Overlap mode: the triangulation belongs to the pose stage (nothing of the front end reads its points), so it goes to the
    // side stream with it -- 0.14 ms per 256 pairs, 50 us of a micro-batch's front-end chain --; only the count snapshot stays in
    // front-end order (SVO_TRI_SIDE=0: the round-5 order, for A/B runs)
    static const bool tri_side = !(getenv("SVO_TRI_SIDE") && getenv("SVO_TRI_SIDE")[0] == '0');
    if (tri_side && ctx->overlap && results_dev != nullptr && !ss) {
        launch_snap_counts(ctx, n_pairs, snap, ctx->stream);
        mark(ctx, kTTri);
        return run_back(ctx, n_pairs, pose0_host, results_dev, /*carried*/ false, /*triangulate_first*/ true);
    }
    launch_triangulate_batch(ctx, n_pairs, cap, ctx->cmp[0], ctx->cmp[1], ctx->m_out, 0, &snap);
    mark(ctx, kTTri);
    if (ctx->carry.on) {
        // svo_set_track_carry: the new frames' lists = what was just tracked into them + their detections; the counts the
        // pose stage reports are already frozen.  A stream set stores the new frames only now.
        launch_carry_pairs(ctx, n_pairs, fp0, fc0, fstep, ss, false);
        mark(ctx, kTCarry);
        if (ss) {
            for_stream_chunks(ss->ids, nullptr, n_pairs, [&](const StreamTable &tab, int i0, int n) { launch_stream_copy(ctx, tab, n, fc0 + i0, /*to_store*/ true); });
            mark(ctx, kTScatter);
        }
    }
    return run_back(ctx, n_pairs, pose0_host, results_dev, ctx->carry.on, false, ss, os);
}

// Pose stage: solvePnPRansac(X, t2_left) (:299 / :200), gates, frame_pose_ chain, optional copy of the
// records; on the side stream in overlap mode.
static int run_back(svo_ctx *ctx, int n_pairs, const double *pose0_host, svo_step_result *results_dev, bool carried,
                    bool triangulate_first, const StreamStep *ss, const OnlineStep *os)
{
    hipStream_t bs = ctx->stream;
    const bool side = ctx->overlap && results_dev != nullptr && !ss;      // a stream-set step is ordered on the context's stream
    if (side) {
        SVO_HIP(hipEventRecord(ctx->ev_front, ctx->stream));
        SVO_HIP(hipStreamWaitEvent(ctx->side_stream, ctx->ev_front, 0));
        bs = ctx->side_stream;
    }
    if (triangulate_first)       // LK mode, overlap: triangulatePoints + the RANSAC start-up of every pair, on the pose stage's stream
        launch_triangulate_batch(ctx, n_pairs, ctx->cfg.max_keypoints, ctx->cmp[0], ctx->cmp[1], ctx->m_out, 0, nullptr, bs);
    launch_pnp_batch(ctx, n_pairs, ctx->cmp[3], ctx->m_out, 0, bs);
    if (!side) mark(ctx, kTPnp);
    // svo_set_pose_refine: robust two-view refinement of every pair's PnP record in place, before the gates read it
    if (ctx->refine_mode != SVO_REFINE_OFF) {
        if (ctx->refine_mode == SVO_REFINE_BA) launch_ba_batch(ctx, n_pairs, bs);
        else launch_refine_batch(ctx, n_pairs, bs);
        if (!side) mark(ctx, kTRefine);
    }
    const int *ovf = ctx->cfg.track_mode == SVO_MODE_ORB ? ctx->kp_n_snap + 2 * n_pairs : nullptr;
    if (ss) {
        // gates per pair, pose_s = pose_s * T_rel_inv per stream (no chain along the launch), init records
        for_stream_chunks(ss->ids, ss->init, n_pairs, [&](const StreamTable &tab, int i0, int n) {
            launch_finalize_streams(ctx, i0, n, n_pairs, ctx->kp_n_snap, ctx->kp_n_snap + n_pairs, ovf, tab, bs);
        });
    } else {
        launch_finalize_chain(ctx, n_pairs, ctx->kp_n_snap, ctx->kp_n_snap + n_pairs, ovf, pose0_host, bs);
    }
    // svo_set_window_ba: the online chain's landmark table moves on by this pair and is adjusted; an applied result rewrites the record's pose
    if (os && os->window) SVO_TRY(window_fused_step(ctx, pose0_host, bs));
    // svo_set_keyframe: the pair's tracks joined with the keyframe's table, one more solve, and where it is accepted its pose in the record
    if (os && os->keyframe) SVO_TRY(keyframe_fused_step(ctx, pose0_host, bs));
    // everything is queued: what this launch ran (the followers belong to online steps; other launches leave theirs alone)
    LastLaunch &last = ctx->last;
    last.pairs = n_pairs; last.carry = carried; last.refine_mode = ctx->refine_mode;
    if (os) { last.window_frames = os->window ? ctx->win.frames : 0; last.keyframe = os->keyframe; }
    const int rc = deliver_records(ctx, ctx->d_results, n_pairs, results_dev, SVO_MEM_DEVICE, bs);
    if (rc) return rc;
    if (side) {
        SVO_HIP(hipEventRecord(ctx->ev_back, ctx->side_stream));
        ctx->back_pending = true;
    } else {
        mark(ctx, kTFin);
    }
    return SVO_OK;
}

// When the online chain breaks -- the ONE statement of it.  Every entry point that starts, re-seats or reconfigures the chain
// calls this; nothing else sets a "start fresh" flag, and only the fused step that honours one clears it (launch_carry_pairs,
// window_fused_step, keyframe_fused_step).
//
//   event                                                   track ids     window table   keyframe
//   kChainNew          svo_reset, a chain's first frame      start at 0    cleared        dropped
//   kChainPoseSet      svo_set_pose                          run on        cleared        dropped    their poses belong to the chain that was
//   kChainCarrySet     svo_set_track_carry, switched on      run on        cleared        dropped    (a list without ids is fresh: carry.ids[])
//   kChainWindowSet    svo_set_window_ba, on or off          run on        cleared        kept
//   kChainKeyframeSet  svo_set_keyframe, on or off           run on        kept           dropped
//
// A failed step is no event of the host's: the kernels read the record's `ok` (the window clears its table, the keyframe stays).
void chain_event(svo_ctx *ctx, ChainEvent ev)
{
    if (ev == kChainNew) ctx->carry.restart = true;
    if (ev != kChainKeyframeSet) ctx->win.clear = true;
    if (ev != kChainWindowSet) ctx->kf.clear = true;
}

int deliver_records(svo_ctx *ctx, const svo_step_result *d_src, int n, svo_step_result *out, int mem, hipStream_t st)
{
    if (mem == SVO_MEM_DEVICE) return from_device(ctx, out, d_src, (size_t)n, mem, st);
    svo_step_result *h;
    SVO_TRY(pinned_records(ctx, sizeof(svo_step_result) * (size_t)n, &h));
    SVO_TRY(from_device(ctx, h, d_src, (size_t)n, mem, st));
    SVO_TRY(io_done(ctx, mem, st));
    memcpy(out, h, sizeof(svo_step_result) * (size_t)n);
    return SVO_OK;
}

int pipeline_track_batch(svo_ctx *ctx, const uint8_t *left_frames, const uint8_t *right_frames, int pitch,
                         int64_t frame_stride, int n_frames, const double *pose0,
                         svo_step_result *results, int results_mem, int carry_first)
{
    const int n_pairs = n_frames - 1;
    // carry_first: frame 0 of this batch IS the last frame of the previous batch on this context (a stream's halo frame):
    // its features are carried over instead of being computed again
    SVO_ARG(!carry_first || ctx->carry_slot > 0, "SVO_CONTINUE_CARRY_FRAME: frame slot of the previous async batch's last frame is no longer valid "
                                                 "(no such batch, a failed launch, or svo_add_frame / a synchronous batch ran in between)");
    const int carry_from = carry_first ? ctx->carry_slot : 0;
    ctx->carry_slot = -1;                        // whatever happens below overwrites frame slots
    ctx->last_batch_pairs = n_pairs;
    mark(ctx, kT0);
    int rc;
    if (carry_from > 0) {
        carry_last_frame(ctx, carry_from);
        rc = ingest_frames(ctx, left_frames + frame_stride, right_frames + frame_stride, pitch, frame_stride, 1, n_frames - 1);
    } else {
        rc = ingest_frames(ctx, left_frames, right_frames, pitch, frame_stride, 0, n_frames);
    }
    if (rc) return rc;
    // the LK outputs use the keypoint stride (cap) per item: frame slots are consecutive (fstep 1)
    // (device records -- results null: they stay in the context for svo_collect_results -- are the pose stage's last copy, on its stream)
    rc = run_pairs(ctx, n_pairs, 0, 1, 1, pose0, results_mem == SVO_MEM_DEVICE ? results : nullptr);
    if (rc) return rc;
    SVO_HIP(hipGetLastError());
    if (results_mem == SVO_MEM_DEVICE) return SVO_OK;
    return deliver_records(ctx, ctx->d_results, n_pairs, results, SVO_MEM_HOST, ctx->stream);
}

// Host image -> device staging: the rows are gathered into a pinned mirror with the staging pitch
// and go over PCIe as ONE copy (a pitched 2-D copy from pageable memory is issued row by row and
// costs ~5 ms per KITTI pair).
int stage_host_image(svo_ctx *ctx, const uint8_t *img, int pitch, int stage_idx, const uint8_t **dptr, int *dpitch)
{
    const int w = ctx->cfg.width, h = ctx->cfg.height, sp = ctx->stage_pitch;
    const size_t bytes = (size_t)sp * h;
    uint8_t *hs = ctx->h_stage + (size_t)stage_idx * bytes;
    uint8_t *dst = ctx->stage_img + (size_t)stage_idx * bytes;
    if (ctx->h_stage_busy[stage_idx]) {
        SVO_HIP(hipEventSynchronize(ctx->ev_stage[stage_idx]));
        ctx->h_stage_busy[stage_idx] = false;
    }
    for (int y = 0; y < h; y++) memcpy(hs + (size_t)y * sp, img + (size_t)y * pitch, (size_t)w);
    SVO_HIP(hipMemcpyAsync(dst, hs, bytes, hipMemcpyHostToDevice, ctx->stream));
    SVO_HIP(hipEventRecord(ctx->ev_stage[stage_idx], ctx->stream));
    ctx->h_stage_busy[stage_idx] = true;
    *dptr = dst; *dpitch = sp;
    return SVO_OK;
}

int pipeline_add_frame(svo_ctx *ctx, const uint8_t *left, const uint8_t *right, int pitch, svo_step_result *res)
{
    ctx->carry_slot = -1;                        // the online ring lives in frame slots 0 / 1
    // two-frame ring in frame slots 0 / 1
    const int cur = ctx->online_frames == 0 ? 0 : (ctx->online_cur ^ 1);
    const int prev = cur ^ 1;
    mark(ctx, kT0);
    int rc = ingest_frames(ctx, left, right, pitch, 0, cur, 1);
    if (rc) return rc;
    memset(res, 0, sizeof(*res));
    ctx->carry.ids[cur] = ctx->carry.on;
    if (ctx->online_frames == 0) {
        chain_event(ctx, kChainNew);
        ctx->last.window_frames = 0; ctx->last.keyframe = false;      // no pair, no follower ran
        // StereoInit_f2f (:78-92): detect only
        int n_cur;
        SVO_TRY(count_read(ctx, ctx->cfg.track_mode == SVO_MODE_ORB ? ctx->orb_n + 2 * cur : ctx->kp_n + cur, &n_cur));
        if (ctx->carry.on) {                     // svo_set_track_carry: the chain's first list gets its ids (the count above stays the detector's)
            launch_carry_pairs(ctx, 1, prev, cur, 0, nullptr, /*no_prev*/ true);
            mark(ctx, kTCarry);
            SVO_HIP(hipGetLastError());
        }
        step_record_clear(*res);
        res->ok = 1; res->n_cur_kps = n_cur;
        memcpy(res->pose, ctx->pose, sizeof(res->pose));
        ctx->online_frames = 1; ctx->online_cur = cur; ctx->online_tracked = 0;
        return SVO_OK;
    }
    const OnlineStep step{ctx->win.frames > 0 && ctx->carry.on, ctx->kf.on && ctx->carry.on};
    rc = run_pairs(ctx, 1, prev, cur, 0, ctx->pose, nullptr, nullptr, &step);
    if (rc) return rc;
    SVO_HIP(hipGetLastError());
    rc = deliver_records(ctx, ctx->d_results, 1, res, SVO_MEM_HOST, ctx->stream);
    if (rc) return rc;
    ctx->online_tracked = res->n_tracked;
    memcpy(ctx->pose, res->pose, sizeof(ctx->pose));
    ctx->online_frames++; ctx->online_cur = cur;       // last_frame_ = current_frame_ on both outcomes (:59-68)
    return res->ok ? SVO_OK : res->fail_stage;
}

// ---- stream sets: many independent live streams through one launch set -----------------------------------------------

int pipeline_streams_create(svo_ctx *ctx, int n_streams)
{
    StreamSet &ss = ctx->streams;
    SVO_ARG(ss.n == 0, "the context already has a stream set");
    SVO_ARG(n_streams >= 1 && n_streams <= (1 << 20), "n_streams must be >= 1");
    SVO_HIP(hipSetDevice(ctx->device));
    if (ctx->cfg.track_mode == SVO_MODE_ORB) { const int rc = orb_alloc(ctx); if (rc) return rc; }
    uint8_t *work[kMaxSeg]; int is_count[kMaxSeg];
    ss.n_seg = stream_segments(ctx, work, ss.seg_bytes, is_count);
    for (int k = 0; k < ss.n_seg; k++) {
        // + 16: a segment whose size is not a multiple of 16 still ends inside its allocation for every access width
        if (dev_alloc(ctx, &ss.seg[k], ss.seg_bytes[k] * (size_t)n_streams + 16) != SVO_OK) return SVO_ERR_HIP;
        SVO_HIP(hipMemsetAsync(ss.seg[k], 0, ss.seg_bytes[k] * (size_t)n_streams + 16, ctx->stream));
    }
    if (dev_alloc(ctx, &ss.pose, sizeof(double) * 16 * (size_t)n_streams) != SVO_OK) return SVO_ERR_HIP;
    ss.n_frames.assign((size_t)n_streams, 0);
    ss.seen.assign((size_t)n_streams, 0);
    ss.has_ids.assign((size_t)n_streams, 0);
    ss.restart.assign((size_t)n_streams, 1);
    ss.call = 0;
    ss.n = n_streams;                                  // the set exists from here on
    if (ctx->carry.buf) SVO_TRY(carry_alloc(ctx));     // svo_set_track_carry came first: the store's ids, ages and counters
    launch_streams_set_pose(ctx, 0, n_streams, nullptr);
    SVO_HIP(hipGetLastError());
    return SVO_OK;
}

int pipeline_streams_reset(svo_ctx *ctx, int id)
{
    StreamSet &ss = ctx->streams;
    SVO_ARG(ss.n > 0, "no stream set (svo_streams_create)");
    SVO_ARG(id >= -1 && id < ss.n, "stream id out of range");
    SVO_HIP(hipSetDevice(ctx->device));
    const int id0 = id < 0 ? 0 : id, n = id < 0 ? ss.n : 1;
    for (int s = id0; s < id0 + n; s++) { ss.n_frames[(size_t)s] = 0; ss.restart[(size_t)s] = 1; }
    launch_streams_set_pose(ctx, id0, n, nullptr);     // in stream order: steps queued before it keep their poses
    SVO_HIP(hipGetLastError());
    return SVO_OK;
}

int pipeline_streams_set_pose(svo_ctx *ctx, int id, const double *pose)
{
    StreamSet &ss = ctx->streams;
    SVO_ARG(ss.n > 0, "no stream set (svo_streams_create)");
    SVO_ARG(id >= 0 && id < ss.n && pose, "stream id out of range / null pose");
    SVO_HIP(hipSetDevice(ctx->device));
    launch_streams_set_pose(ctx, id, 1, pose);         // the pose travels by value in the argument block
    SVO_HIP(hipGetLastError());
    return SVO_OK;
}

int pipeline_streams_get_pose(svo_ctx *ctx, int id, double *pose)
{
    StreamSet &ss = ctx->streams;
    SVO_ARG(ss.n > 0, "no stream set (svo_streams_create)");
    SVO_ARG(id >= 0 && id < ss.n && pose, "stream id out of range / null pose");
    SVO_HIP(hipSetDevice(ctx->device));
    double *h;
    SVO_TRY(pinned_block(ctx, sizeof(double) * 16, &h));
    SVO_TRY(from_device(ctx, h, (const double *)ss.pose + (size_t)id * 16, 16, SVO_MEM_HOST));
    SVO_TRY(io_done(ctx, SVO_MEM_HOST));
    memcpy(pose, h, sizeof(double) * 16);
    return SVO_OK;
}

// The m ids of one step: each names a stream of the set, none twice (a stream remembers the last call that named it).
int pipeline_streams_check_ids(svo_ctx *ctx, const int32_t *ids, int m)
{
    StreamSet &ss = ctx->streams;
    for (int i = 0; i < m; i++) SVO_ARG(ids[i] >= 0 && ids[i] < ss.n, "stream id out of range");
    ss.call++;
    for (int i = 0; i < m; i++) {
        SVO_ARG(ss.seen[(size_t)ids[i]] != ss.call, "the same stream id twice in one step");
        ss.seen[(size_t)ids[i]] = ss.call;
    }
    return SVO_OK;
}

// Frame i at base + i * frame_stride.  Working frame slots 0 .. m-1 hold the streams' previous frames, m .. 2m-1 the new ones:
// 2m of the context's max_batch + 1.
int pipeline_streams_step(svo_ctx *ctx, const int32_t *ids, int m, const uint8_t *L, const uint8_t *R, int pitch,
                          int64_t frame_stride, svo_step_result *results, int results_mem)
{
    StreamSet &ss = ctx->streams;
    // one more writer of the working frame slots and the pair buffers, like svo_track_batch: a pending side-stream pose stage
    // still reads them, and neither a carried frame nor the online ring survives
    if (ctx->back_pending) {
        SVO_HIP(hipStreamWaitEvent(ctx->stream, ctx->ev_back, 0));
        ctx->back_pending = false;
    }
    ctx->carry_slot = -1;
    ctx->last_batch_pairs = m;
    std::vector<uint8_t> init((size_t)m);
    for (int i = 0; i < m; i++) init[(size_t)i] = ss.n_frames[(size_t)ids[i]] == 0;
    mark(ctx, kT0);
    for_stream_chunks(ids, init.data(), m, [&](const StreamTable &tab, int i0, int n) { launch_stream_copy(ctx, tab, n, i0, /*to_store*/ false); });
    mark(ctx, kTGather);
    int rc = ingest_frames(ctx, L, R, pitch, m == 1 ? 0 : frame_stride, m, m);
    if (rc) return rc;
    if (!ctx->carry.on) {                               // (with track carry the lists are still to be merged: run_pairs stores the frames)
        for_stream_chunks(ids, nullptr, m, [&](const StreamTable &tab, int i0, int n) { launch_stream_copy(ctx, tab, n, m + i0, /*to_store*/ true); });
        mark(ctx, kTScatter);
        for (int i = 0; i < m; i++) ss.has_ids[(size_t)ids[i]] = 0;
    }
    // last_frame_ = current_frame_ on every outcome (src/tracking.cpp:59-68): the store already holds the new frames
    for (int i = 0; i < m; i++) ss.n_frames[(size_t)ids[i]]++;
    const StreamStep step{ids, init.data()};
    rc = run_pairs(ctx, m, 0, m, 1, nullptr, nullptr, &step);
    if (rc) return rc;
    SVO_HIP(hipGetLastError());
    return deliver_records(ctx, ctx->d_results, m, results, results_mem, ctx->stream);
}

}  // namespace svo
