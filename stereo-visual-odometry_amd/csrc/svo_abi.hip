// svo_abi.hip -- host side of the C-ABI declared in include/svo_abi.h: context lifecycle, buffer
// ownership (ctx owns every device buffer; no allocation in the steady state) and the stage /
// fused entry points that launch the HIP kernels.  There is NO CPU fallback in this library.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <ctime>
#include <new>
#include <vector>
#include "abi_io.h"
#include "carry.h"
#include "fast_scratch.h"
#include "pose_device.h"

using namespace svo;

namespace svo {
int dev_alloc_raw(svo_ctx *ctx, void **out, size_t bytes)
{
    *out = nullptr;
    if (bytes == 0) bytes = 1;
    if (ctx->arena.planning) {
        ctx->arena.plan.emplace_back(out, ctx->arena.planned);
        ctx->arena.planned += align_up(bytes, kDevAlign);
        return SVO_OK;
    }
    SVO_HIP(hipMalloc(out, bytes));
    ctx->arena.extra.push_back(*out);
    return SVO_OK;
}

int dev_defer(svo_ctx *ctx, std::function<int()> fn)
{
    if (!ctx->arena.planning) return fn();
    ctx->arena.after.push_back(std::move(fn));
    return SVO_OK;
}

static int dev_commit(svo_ctx *ctx)
{
    DevArena &a = ctx->arena;
    a.planning = false;
    SVO_HIP(hipMalloc((void **)&a.base, a.planned + 256));
    for (auto &e : a.plan) *e.first = a.base + e.second;
    a.plan.clear();
    for (auto &fn : a.after) { const int rc = fn(); if (rc != SVO_OK) return rc; }
    a.after.clear();
    return SVO_OK;
}

int dev_reserve(svo_ctx *ctx, DevScratch *s, size_t bytes)
{
    if (s->base && bytes <= s->bytes) return SVO_OK;
    uint8_t *grown = nullptr;
    SVO_HIP(hipMalloc((void **)&grown, bytes ? bytes : 1));
    uint8_t *old = s->base;
    if (!old) ctx->arena.scratch.push_back(s);                 // its first block: the context frees it from now on
    s->base = grown; s->bytes = bytes;
    if (old) (void)hipFree(old);
    return SVO_OK;
}

int dev_event(svo_ctx *ctx, hipEvent_t *ev, unsigned flags)
{
    if (*ev) return SVO_OK;
    SVO_HIP(hipEventCreateWithFlags(ev, flags));
    ctx->arena.events.push_back(*ev);
    return SVO_OK;
}

int dev_stream(svo_ctx *ctx, hipStream_t *st)
{
    if (*st) return SVO_OK;
    SVO_HIP(hipStreamCreateWithFlags(st, hipStreamNonBlocking));
    ctx->arena.streams.push_back(*st);
    return SVO_OK;
}

static void dev_release(svo_ctx *ctx)
{
    DevArena &a = ctx->arena;
    for (DevScratch *s : a.scratch) { (void)hipFree(s->base); *s = DevScratch(); }
    a.scratch.clear();
    for (void *p : a.extra) if (p) (void)hipFree(p);
    a.extra.clear();
    if (a.base) (void)hipFree(a.base);
    a.base = nullptr;
}
}  // namespace svo

static int frame_buffers(svo_ctx *ctx);              // the lazily made sets of an online-sized context, which svo_create makes
static int async_ring(svo_ctx *ctx);                 // for a batch context

constexpr int kMaxFrameSide = 16384;                // svo_create refuses larger frames
// the LK kernels form tile offsets with 24-bit multiplies (lk_common.h, stage_src): the widest accepted pitch fits
static_assert(kMaxFrameSide + 2 * kPad + 63 <= kMaxLkPitch, "pitch of the widest accepted frame exceeds the LK kernels' 24-bit multiply");

// Pyramid geometry: buildOpticalFlowPyramid stops adding levels once the next one would not
// exceed the 21-pixel window ("if (sz.width <= winSize.width || sz.height <= winSize.height)").
static void make_geom(int w, int h, PyrGeom *g)
{
    memset(g, 0, sizeof(*g));
    int64_t off = 0;
    int lw = w, lh = h;
    for (int l = 0; l < kMaxLevels; l++) {
        if (l > 0) {
            int nw = (lw + 1) / 2, nh = (lh + 1) / 2;
            if (nw <= kWin || nh <= kWin) break;
            lw = nw; lh = nh;
        }
        g->w[l] = lw; g->h[l] = lh;
        g->pitch[l] = align_up(lw + 2 * kPad, 64);
        g->origin[l] = off + (int64_t)kPad * g->pitch[l] + kPad;
        off += (int64_t)g->pitch[l] * (lh + 2 * kPad);
        off = (int64_t)align_up((size_t)off, kDevAlign);
        g->nlevels = l + 1;
    }
    g->slot_bytes = off;
}

extern "C" int svo_abi_version(void) { return SVO_ABI_VERSION; }
extern "C" int svo_config_bytes(void) { return (int)sizeof(svo_config); }

extern "C" int svo_device_count(int *n)
{
    if (!n) return SVO_ERR_ARG;
    *n = 0;
    int c = 0;
    if (hipGetDeviceCount(&c) != hipSuccess || c <= 0) return SVO_ERR_HIP;
    *n = c;
    return SVO_OK;
}

extern "C" void svo_default_config(svo_config *cfg, int width, int height)
{
    memset(cfg, 0, sizeof(*cfg));
    cfg->width = width; cfg->height = height;
    cfg->max_keypoints = 8192;
    cfg->max_batch = 1;
    cfg->num_slots = 4;
    cfg->fast_threshold = 20;               // src/tracking.cpp:99
    cfg->num_features_tracking = 5;         // config/default.yaml:69
    cfg->iterations = 500;                  // :80
    cfg->reproj_err = 0.5f;                 // :81
    cfg->confidence = 0.99f;                // :82
    cfg->feature_match_error = 3.0;         // :66
    cfg->inlier_rate = 0.01;                // :77
    cfg->min_move2 = 0.0005 * 0.0005;       // LK mode, src/tracking.cpp:311
    cfg->max_move2 = 100.0;
    const double fx = 718.856, fy = 718.856, cx = 607.193, cy = 185.216, tx = -0.537;   // default.yaml:33-47
    const double P1[12] = {fx, 0, cx, 0, 0, fy, cy, 0, 0, 0, 1, 0};
    const double P2[12] = {fx, 0, cx, fx * tx, 0, fy, cy, 0, 0, 0, 1, 0};
    memcpy(cfg->P1, P1, sizeof(P1));
    memcpy(cfg->P2, P2, sizeof(P2));
    cfg->track_mode = SVO_MODE_LK;
    cfg->orb_nfeatures = 2000;              // config/default.yaml:93
    cfg->orb_scale_factor = 1.2f;           // :92
    cfg->orb_nlevels = 8;                   // :91
    cfg->orb_ini_th = 20;                   // :90
    cfg->orb_min_th = 7;                    // :89
    cfg->fast_keep_strongest = 0;           // every cv::FAST corner, as the reference tracks them
    cfg->lk_accum = SVO_LK_ACCUM_EXACT;     // the canonical recipe; SVO_LK_ACCUM_SSE2 = an x86 OpenCV build's float order
}

static void free_all(svo_ctx *c)
{
    dev_release(c);                                   // every device buffer: the arena, the lazy extras, the growable scratch
    if (c->h_pinned) (void)hipHostFree(c->h_pinned);
    if (c->h_stage) (void)hipHostFree(c->h_stage);
    DevArena &a = c->arena;
    for (hipEvent_t e : a.events) (void)hipEventDestroy(e);
    for (size_t k = a.streams.size(); k-- > 0;) (void)hipStreamDestroy(a.streams[k]);      // the context's own stream last
    a.events.clear(); a.streams.clear();
}

// SVO_TIMING=1: milliseconds of svo_create's phases on stderr (where a short run's start-up goes)
static double now_ms()
{
    timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6;
}
#define PHASE(name) do { if (timing_on) { const double t__ = now_ms(); fprintf(stderr, "[svo_create] %8.2f ms  %s\n", t__ - t_phase, name); t_phase = t__; } } while (0)

extern "C" int svo_create(const svo_config *cfg, int device, svo_ctx **out)
{
    if (!cfg || !out) return SVO_ERR_ARG;
    const bool timing_on = getenv("SVO_TIMING") != nullptr;
    double t_phase = now_ms();
    *out = nullptr;
    if (cfg->width < 32 || cfg->height < 32 || cfg->max_keypoints < 64 || cfg->max_batch < 1 ||
        cfg->num_slots < 4 || cfg->width > kMaxFrameSide || cfg->height > kMaxFrameSide)
        return SVO_ERR_ARG;
    if (cfg->lk_accum != SVO_LK_ACCUM_EXACT && cfg->lk_accum != SVO_LK_ACCUM_SSE2 && cfg->lk_accum != SVO_LK_ACCUM_SIMD128 &&
        cfg->lk_accum != SVO_LK_ACCUM_SSE2_LEGACY) {
        fprintf(stderr, "svo_create: lk_accum = %d is none of SVO_LK_ACCUM_EXACT / _SSE2 / _SIMD128 / _SSE2_LEGACY\n", cfg->lk_accum);
        return SVO_ERR_ARG;
    }
    if (cfg->fast_keep_strongest < 0) return SVO_ERR_ARG;
    if (cfg->num_features_tracking < 4) {
        // a pair with exactly 4 tracks takes cv::solvePnPRansac's npoints == 4 branch (the P3P kernel: geometry.hip); with
        // fewer than 4 the reference's call asserts (CV_Assert(npoints >= 4)) and the process dies: refuse the configuration
        fprintf(stderr, "svo_create: num_features_tracking = %d < 4 is not supported (cv::solvePnPRansac asserts npoints >= 4)\n",
                cfg->num_features_tracking);
        return SVO_ERR_ARG;
    }
    svo_ctx *ctx = new (std::nothrow) svo_ctx();
    if (!ctx) return SVO_ERR_NOMEM;
    ctx->cfg = *cfg;
    ctx->device = device;
    pose_identity16(ctx->pose);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) {
        // fail loudly: this library has no CPU path
        fprintf(stderr, "svo_create: no usable HIP device (count=%d, requested %d)\n", ndev, device);
        delete ctx;
        return SVO_ERR_HIP;
    }
    PHASE("hipGetDeviceCount (HIP runtime start)");
    auto fail = [&](int code) { free_all(ctx); delete ctx; return code; };
    // (HIP calls and the context's own helpers alike: hipSuccess and SVO_OK are both 0)
#define CK(call) do { if ((call) != 0) { fprintf(stderr, "svo_create: %s failed\n", #call); return fail(SVO_ERR_HIP); } } while (0)
    CK(hipSetDevice(device));
    CK(dev_stream(ctx, &ctx->own_stream));
    ctx->stream = ctx->own_stream;
    PHASE("hipSetDevice + stream");
    make_geom(cfg->width, cfg->height, &ctx->geom);

    const int w = cfg->width, h = cfg->height, cap = cfg->max_keypoints, B = cfg->max_batch;
    const int n_img = B + 1;
    ctx->n_img = n_img;
    const bool orb = cfg->track_mode == SVO_MODE_ORB;
    if (!orb && cfg->track_mode != SVO_MODE_LK) return fail(SVO_ERR_ARG);
    // What only the LK pipeline touches is sized for ONE item in an ORB context (the stage API -- svo_fast_detect,
    // svo_lk_track, svo_circular_match -- stays usable there); the ORB buffers of an LK context are allocated on first use.
    const int n_fast = orb ? 1 : n_img, B_lk = orb ? 1 : B;
    ctx->arena.planning = true;
#define DA(ptr, bytes) do { if (dev_alloc(ctx, &(ptr), (bytes)) != SVO_OK) return fail(SVO_ERR_HIP); } while (0)
    DA(ctx->slots, (size_t)cfg->num_slots * ctx->geom.slot_bytes);
    dev_defer(ctx, [ctx]() { SVO_HIP(hipMemsetAsync(ctx->slots, 0, (size_t)ctx->cfg.num_slots * ctx->geom.slot_bytes, ctx->stream)); return SVO_OK; });
    ctx->slot_built.assign(cfg->num_slots, 0);
    ctx->stage_pitch = align_up(w, 256);
    DA(ctx->stage_img, (size_t)ctx->stage_pitch * h * 2);
    // FAST scratch: corner records and per-(row, tile column) counts, sized by the bounds in fast_scratch.h
    ctx->spitch = fast_record_pitch(w);
    ctx->score_stride = (int64_t)ctx->spitch * h;
    DA(ctx->score, (size_t)ctx->score_stride * n_fast);
    ctx->rowcount_stride = fast_count_words(w, h);
    DA(ctx->rowcount, sizeof(int) * (size_t)ctx->rowcount_stride * n_fast);
    DA(ctx->kp_xy, sizeof(float2) * (size_t)cap * n_fast);
    DA(ctx->kp_resp, sizeof(float) * (size_t)cap * n_fast);
    DA(ctx->kp_n, sizeof(int) * (size_t)n_fast);
    DA(ctx->pts_in, sizeof(float2) * (size_t)cap * B_lk);
    for (int i = 0; i < 4; i++) {
        DA(ctx->pts_out[i], sizeof(float2) * (size_t)cap * B_lk);
        DA(ctx->status[i], (size_t)cap * B_lk);
        DA(ctx->cmp[i], sizeof(float2) * (size_t)cap * B);
    }
    DA(ctx->keep, (size_t)cap * B_lk);
    DA(ctx->m_out, sizeof(int) * (size_t)B);
    DA(ctx->X3, sizeof(float) * 3 * (size_t)cap * B);
    if (geom_workspace_bytes(*cfg, B, &ctx->pnp_ws_bytes) != SVO_OK) return fail(SVO_ERR_ARG);
    PHASE("plan + kernel attributes (code object load)");
    DA(ctx->pnp_ws, ctx->pnp_ws_bytes);
    dev_defer(ctx, [ctx]() { return geom_workspace_init(ctx); });
    DA(ctx->d_results, sizeof(svo_step_result) * (size_t)B);
    DA(ctx->bslots, orb ? 256 : (size_t)2 * n_img * ctx->geom.slot_bytes);
    DA(ctx->kp_n_snap, sizeof(int) * (size_t)(3 * n_img));
    if (B > 1) {
        // a batch context is what the runner and the stream create: their frame buffers and record rings come with it
        const size_t per_cam = (size_t)ctx->stage_pitch * h * (size_t)(B + 1);
        for (int k = 0; k < 2; k++) {
            DA(ctx->fb[k], 2 * per_cam);
            DA(ctx->d_async[k], sizeof(svo_step_result) * (size_t)B);
        }
    }
    if (orb) {
        int rc = orb_alloc(ctx);
        if (rc != SVO_OK) { fprintf(stderr, "svo_create: %s\n", ctx->err.c_str()); return fail(rc); }
    }
#undef DA
    if (dev_commit(ctx) != SVO_OK) { fprintf(stderr, "svo_create: device memory (%zu MB): %s\n", ctx->arena.planned >> 20, ctx->err.c_str()); return fail(SVO_ERR_HIP); }
    PHASE("one device allocation + deferred initialisation");
    CK(hipHostMalloc(&ctx->h_stage, (size_t)ctx->stage_pitch * h * 2, hipHostMallocDefault));
    for (int k = 0; k < 2; k++) CK(dev_event(ctx, &ctx->ev_stage[k]));
    // (a high-priority side stream was measured in round 6: no difference, 5.80 against 5.80 ms per ORB step and 14.32 against
    // 14.34 per LK step -- what holds a pose-stage kernel back beside the next front end is free LDS and wave slots on a CU, not
    // the queue's place at the dispatcher)
    CK(dev_stream(ctx, &ctx->side_stream));
    CK(dev_event(ctx, &ctx->ev_front));
    CK(dev_event(ctx, &ctx->ev_back));
    if (B > 1) {                                      // (their device memory came with the arena)
        CK(frame_buffers(ctx));
        CK(async_ring(ctx));
    }
    // (the fixed records read back through the block: PnpRecord, svo_refine_result, a stream's pose)
    ctx->pinned = pinned_layout((size_t)cap, (size_t)B, sizeof(svo_keypoint), sizeof(svo_step_result),
                                std::max({sizeof(PnpRecord), sizeof(svo_refine_result), sizeof(double) * 16}));
    CK(hipHostMalloc(&ctx->h_pinned, ctx->pinned.total, hipHostMallocDefault));
    PHASE("events, streams, page-locked scratch");
    CK(hipStreamSynchronize(ctx->stream));
    PHASE("stream sync");
#undef CK
    *out = ctx;
    return SVO_OK;
}

extern "C" void svo_destroy(svo_ctx *ctx)
{
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    if (ctx->side_stream) (void)hipStreamSynchronize(ctx->side_stream);
    free_all(ctx);
    delete ctx;
}

extern "C" const char *svo_last_error(const svo_ctx *ctx) { return ctx ? ctx->err.c_str() : "null context"; }

extern "C" int svo_set_stream(svo_ctx *ctx, void *hip_stream)
{
    if (!ctx) return SVO_ERR_ARG;
    if (svo_wait_results(ctx) != SVO_OK) return SVO_ERR_HIP;
    ctx->stream = hip_stream ? (hipStream_t)hip_stream : ctx->own_stream;
    return SVO_OK;
}

extern "C" int svo_sync(svo_ctx *ctx)
{
    if (!ctx) return SVO_ERR_ARG;
    SVO_HIP(hipStreamSynchronize(ctx->stream));
    if (ctx->back_pending) { SVO_HIP(hipStreamSynchronize(ctx->side_stream)); ctx->back_pending = false; }
    return SVO_OK;
}

extern "C" int svo_set_overlap(svo_ctx *ctx, int on)
{
    if (!ctx) return SVO_ERR_ARG;
    int rc = svo_wait_results(ctx);
    if (rc) return rc;
    ctx->overlap = on != 0;
    return SVO_OK;
}

// Makes the context's stream wait (on the device, no host sync) for the pose stage of the last
// svo_track_batch when overlap mode runs it on the side stream.
extern "C" int svo_wait_results(svo_ctx *ctx)
{
    if (!ctx) return SVO_ERR_ARG;
    if (ctx->back_pending) {
        SVO_HIP(hipStreamWaitEvent(ctx->stream, ctx->ev_back, 0));
        ctx->back_pending = false;
    }
    return SVO_OK;
}

// The read-backs' common start: what is asked for exists (`ran`, else the ARG error `why_not`), the context's device is current
// and a pose stage still on the side stream is ordered before the context's stream.
static int read_back_ready(svo_ctx *ctx, bool ran, const char *why_not)
{
    SVO_ARG(ran, why_not);
    SVO_HIP(hipSetDevice(ctx->device));
    return svo_wait_results(ctx) == SVO_OK ? SVO_OK : SVO_ERR_HIP;
}

// What a follower stage of the online chain (`name`) needs before it is switched on: an LK-mode context, track carry on, and
// the other stage that rewrites the step's pose off.
static int follower_may_start(svo_ctx *ctx, const std::string &name, bool other_on, const std::string &other, const char *other_off)
{
    SVO_ARG(ctx->cfg.track_mode == SVO_MODE_LK, name + " is an LK-mode option");
    if (!ctx->carry.on) { ctx->err = name + " needs track carry (svo_set_track_carry) on"; return SVO_ERR_STATE; }
    if (other_on) { ctx->err = other + " is on and rewrites the step's pose too (" + other_off + " first)"; return SVO_ERR_STATE; }
    return SVO_OK;
}

// ABI v7: ordering against work on OTHER streams on the device, without a host synchronisation.
extern "C" int svo_wait_stream(svo_ctx *ctx, void *hip_stream)
{
    if (!ctx) return SVO_ERR_ARG;
    hipStream_t other = (hipStream_t)hip_stream;
    if (other == ctx->stream) return SVO_OK;                     // same queue: already ordered
    SVO_HIP(hipSetDevice(ctx->device));
    if (dev_event(ctx, &ctx->ev_order) != SVO_OK) return SVO_ERR_HIP;
    SVO_HIP(hipEventRecord(ctx->ev_order, other));
    SVO_HIP(hipStreamWaitEvent(ctx->stream, ctx->ev_order, 0));
    return SVO_OK;
}

extern "C" int svo_signal_stream(svo_ctx *ctx, void *hip_stream)
{
    if (!ctx) return SVO_ERR_ARG;
    hipStream_t other = (hipStream_t)hip_stream;
    SVO_HIP(hipSetDevice(ctx->device));
    // the pose stage of an overlap-mode batch ends on the side stream: its event first (kept pending for the context's own waits)
    if (ctx->back_pending && other != ctx->side_stream) SVO_HIP(hipStreamWaitEvent(other, ctx->ev_back, 0));
    if (other == ctx->stream) return SVO_OK;
    if (dev_event(ctx, &ctx->ev_order) != SVO_OK) return SVO_ERR_HIP;
    SVO_HIP(hipEventRecord(ctx->ev_order, ctx->stream));
    SVO_HIP(hipStreamWaitEvent(other, ctx->ev_order, 0));
    return SVO_OK;
}

// ABI v9: the front end only (everything that reads the caller's frames is on ctx->stream; the pose stage of an overlap-mode
// batch, which reads context memory only, is on the side stream and is not waited for).
extern "C" int svo_signal_stream_inputs(svo_ctx *ctx, void *hip_stream)
{
    if (!ctx) return SVO_ERR_ARG;
    hipStream_t other = (hipStream_t)hip_stream;
    if (other == ctx->stream) return SVO_OK;
    SVO_HIP(hipSetDevice(ctx->device));
    if (dev_event(ctx, &ctx->ev_order) != SVO_OK) return SVO_ERR_HIP;
    SVO_HIP(hipEventRecord(ctx->ev_order, ctx->stream));
    SVO_HIP(hipStreamWaitEvent(other, ctx->ev_order, 0));
    return SVO_OK;
}

extern "C" int svo_num_levels(const svo_ctx *ctx) { return ctx ? ctx->geom.nlevels : 0; }

extern "C" int svo_enable_timing(svo_ctx *ctx, int on)
{
    if (!ctx) return SVO_ERR_ARG;
    ctx->timing = on != 0;
    return SVO_OK;
}

// Resolves the stage marks logged since the last query: synchronises the stream, averages the
// elapsed time of each stage over the logged steps ("start" opens a step), clears the log.
extern "C" int svo_get_timing(svo_ctx *ctx, const char **names, float *ms, int cap)
{
    if (!ctx) return SVO_ERR_ARG;
    SVO_HIP(hipStreamSynchronize(ctx->stream));
    std::vector<std::pair<const char *, double>> acc;
    std::vector<int> cnt;
    for (size_t i = 1; i < ctx->marks.size(); i++) {
        const char *nm = ctx->marks[i].first;
        if (strcmp(nm, "start") == 0) continue;
        float t = 0.f;
        if (hipEventElapsedTime(&t, ctx->marks[i - 1].second, ctx->marks[i].second) != hipSuccess) continue;
        size_t k = 0;
        for (; k < acc.size(); k++) if (acc[k].first == nm) break;
        if (k == acc.size()) { acc.emplace_back(nm, 0.0); cnt.push_back(0); }
        acc[k].second += t; cnt[k]++;
    }
    ctx->marks.clear();
    ctx->ev_used = 0;
    ctx->last_times.clear();
    for (size_t k = 0; k < acc.size(); k++) ctx->last_times.emplace_back(acc[k].first, (float)(acc[k].second / cnt[k]));
    int n = 0;
    for (auto &t : ctx->last_times) {
        if (n >= cap) break;
        if (names) names[n] = t.first;
        if (ms) ms[n] = t.second;
        n++;
    }
    return n;
}

// Host images are copied into the context's staging buffer (aligned pitch); device images are
// used in place.
static int resolve_image(svo_ctx *ctx, const uint8_t *img, int pitch, int mem, int stage_idx,
                         const uint8_t **dptr, int *dpitch)
{
    SVO_ARG(img != nullptr, "null image");
    SVO_ARG(pitch >= ctx->cfg.width, "pitch < width");
    if (mem == SVO_MEM_DEVICE) { *dptr = img; *dpitch = pitch; return SVO_OK; }
    SVO_ARG(mem == SVO_MEM_HOST, "mem must be SVO_MEM_HOST or SVO_MEM_DEVICE");
    return svo::stage_host_image(ctx, img, pitch, stage_idx, dptr, dpitch);
}

extern "C" int svo_fast_detect(svo_ctx *ctx, const uint8_t *img, int pitch, int mem, int threshold,
                               int nonmax, svo_keypoint *out, int cap, int *n_out)
{
    if (!ctx) return SVO_ERR_ARG;
    SVO_ARG(out && n_out && cap >= 0, "null output");
    SVO_HIP(hipSetDevice(ctx->device));
    const uint8_t *d; int dp;
    int rc = resolve_image(ctx, img, pitch, mem, 0, &d, &dp);
    if (rc) return rc;
    FastArgs a{};
    a.img = d; a.pitch = dp; a.img_stride = 0;
    a.w = ctx->cfg.width; a.h = ctx->cfg.height;
    a.thr = threshold < 0 ? 0 : (threshold > 255 ? 255 : threshold);
    a.nms = nonmax != 0;
    a.score = ctx->score; a.spitch = ctx->spitch; a.score_stride = ctx->score_stride;
    a.rowcount = ctx->rowcount; a.rowcount_stride = ctx->rowcount_stride;
    a.kp_xy = ctx->kp_xy; a.kp_resp = ctx->kp_resp; a.kp_stride = ctx->cfg.max_keypoints;
    a.n_out = ctx->kp_n; a.cap = ctx->cfg.max_keypoints;
    launch_fast(a, 1, ctx->stream);
    SVO_HIP(hipGetLastError());
    // D2H through pinned scratch: count, then xy + response
    int n;
    SVO_TRY(count_read(ctx, ctx->kp_n, &n));
    *n_out = n;
    if (n > ctx->cfg.max_keypoints) { ctx->err = "FAST: keypoints exceed max_keypoints"; return SVO_ERR_ARG; }
    if (n > cap) { ctx->err = "FAST: keypoints exceed caller capacity"; return SVO_ERR_ARG; }
    if (n == 0) return SVO_OK;
    float2 *h_xy;
    SVO_TRY(pinned_block(ctx, (sizeof(float2) + sizeof(float)) * (size_t)ctx->cfg.max_keypoints, &h_xy));
    float *h_r = (float *)(h_xy + ctx->cfg.max_keypoints);
    SVO_TRY(from_device(ctx, h_xy, (const float2 *)ctx->kp_xy, (size_t)n, SVO_MEM_HOST));
    SVO_TRY(from_device(ctx, h_r, (const float *)ctx->kp_resp, (size_t)n, SVO_MEM_HOST));
    SVO_TRY(io_done(ctx, SVO_MEM_HOST));
    // always a HOST array (it is an array of structs for the caller's std::vector<cv::KeyPoint>)
    format_keypoints(h_xy, h_r, n, out);
    return SVO_OK;
}

extern "C" int svo_build_pyramid(svo_ctx *ctx, int slot, const uint8_t *img, int pitch, int mem)
{
    if (!ctx) return SVO_ERR_ARG;
    SVO_ARG(slot >= 0 && slot < ctx->cfg.num_slots, "slot out of range");
    SVO_HIP(hipSetDevice(ctx->device));
    const uint8_t *d; int dp;
    int rc = resolve_image(ctx, img, pitch, mem, 0, &d, &dp);
    if (rc) return rc;
    PyrArgs a{};
    a.g = ctx->geom; a.img = d; a.pitch = dp; a.img_stride = 0;
    a.slots = ctx->slots + (size_t)slot * ctx->geom.slot_bytes; a.slot_stride = 0;
    launch_pyramid(a, 1, ctx->stream);
    SVO_HIP(hipGetLastError());
    if (mem == SVO_MEM_HOST) SVO_HIP(hipStreamSynchronize(ctx->stream));   // staging buffer is reused
    ctx->slot_built[slot] = 1;
    return SVO_OK;
}

extern "C" int svo_read_pyramid_level(svo_ctx *ctx, int slot, int level, uint8_t *out, int out_pitch,
                                      int mem, int *w, int *h)
{
    if (!ctx) return SVO_ERR_ARG;
    SVO_ARG(slot >= 0 && slot < ctx->cfg.num_slots, "slot out of range");
    SVO_ARG(level >= 0 && level < ctx->geom.nlevels, "level out of range");
    if (!ctx->slot_built[slot]) { ctx->err = "pyramid slot not built"; return SVO_ERR_STATE; }
    const int lw = ctx->geom.w[level], lh = ctx->geom.h[level];
    if (w) *w = lw;
    if (h) *h = lh;
    if (!out) return SVO_OK;
    SVO_ARG(out_pitch >= lw, "out_pitch < level width");
    SVO_HIP(hipSetDevice(ctx->device));
    const uint8_t *s = ctx->slots + (size_t)slot * ctx->geom.slot_bytes;
    if (mem == SVO_MEM_DEVICE) {
        launch_pyr_read_level(ctx->geom, s, level, out, out_pitch, ctx->stream);
        SVO_HIP(hipGetLastError());
        return SVO_OK;
    }
    SVO_HIP(hipMemcpy2DAsync(out, out_pitch, s + ctx->geom.origin[level], ctx->geom.pitch[level], lw, lh,
                             hipMemcpyDeviceToHost, ctx->stream));
    SVO_HIP(hipStreamSynchronize(ctx->stream));
    return SVO_OK;
}

static void fill_lk_common(svo_ctx *ctx, LkArgs &a, int n)
{
    a.g = ctx->geom;
    a.slot_stride = 0;
    a.pts_stride = 0;
    a.n_pts = nullptr; a.n_fixed = n; a.cap = n;
    a.match_err = ctx->cfg.feature_match_error;
    a.accum = ctx->cfg.lk_accum;
}

extern "C" int svo_lk_track(svo_ctx *ctx, int slot_prev, int slot_next, const svo_pt2f *prev_pts, int n,
                            svo_pt2f *next_pts, uint8_t *status, int mem)
{
    if (!ctx) return SVO_ERR_ARG;
    SVO_ARG(slot_prev >= 0 && slot_prev < ctx->cfg.num_slots && slot_next >= 0 &&
            slot_next < ctx->cfg.num_slots, "slot out of range");
    SVO_ARG(n >= 0 && n <= ctx->cfg.max_keypoints, "n exceeds max_keypoints");
    SVO_ARG(mem == SVO_MEM_HOST || mem == SVO_MEM_DEVICE, "bad mem");
    if (!ctx->slot_built[slot_prev] || !ctx->slot_built[slot_next]) { ctx->err = "pyramid slot not built"; return SVO_ERR_STATE; }
    if (n == 0) return SVO_OK;
    SVO_ARG(prev_pts && next_pts && status, "null pointer");
    SVO_HIP(hipSetDevice(ctx->device));
    const float2 *d_in;
    SVO_TRY(to_device(ctx, (const float2 *)prev_pts, ctx->pts_in, (size_t)n, mem, &d_in));
    LkArgs a{};
    fill_lk_common(ctx, a, n);
    a.ncalls = 1;
    a.prev[0] = ctx->slots + (size_t)slot_prev * ctx->geom.slot_bytes;
    a.next[0] = ctx->slots + (size_t)slot_next * ctx->geom.slot_bytes;
    a.pts_in = d_in;
    a.pts_out[0] = mem == SVO_MEM_DEVICE ? (float2 *)next_pts : ctx->pts_out[0];
    a.status[0] = mem == SVO_MEM_DEVICE ? status : ctx->status[0];
    launch_lk(a, 1, n, ctx->stream);
    SVO_HIP(hipGetLastError());
    SVO_TRY(from_device(ctx, (float2 *)next_pts, (const float2 *)a.pts_out[0], (size_t)n, mem));      // (device: the kernel wrote them)
    SVO_TRY(from_device(ctx, status, (const uint8_t *)a.status[0], (size_t)n, mem));
    return io_done(ctx, mem);
}

extern "C" int svo_circular_match(svo_ctx *ctx, int slot_prevL, int slot_prevR, int slot_curL, int slot_curR,
                                  const svo_pt2f *t1_left, int n, svo_pt2f *out_t1_left,
                                  svo_pt2f *out_t1_right, svo_pt2f *out_t2_right, svo_pt2f *out_t2_left,
                                  int *m_out, int mem)
{
    if (!ctx) return SVO_ERR_ARG;
    const int sl[4] = {slot_prevL, slot_prevR, slot_curL, slot_curR};
    for (int i = 0; i < 4; i++) {
        SVO_ARG(sl[i] >= 0 && sl[i] < ctx->cfg.num_slots, "slot out of range");
        if (!ctx->slot_built[sl[i]]) { ctx->err = "pyramid slot not built"; return SVO_ERR_STATE; }
    }
    SVO_ARG(n >= 0 && n <= ctx->cfg.max_keypoints, "n exceeds max_keypoints");
    SVO_ARG(mem == SVO_MEM_HOST || mem == SVO_MEM_DEVICE, "bad mem");
    SVO_ARG(m_out != nullptr, "null m_out");
    if (svo_wait_results(ctx) != SVO_OK) return SVO_ERR_HIP;
    *m_out = 0;
    if (n == 0) return SVO_OK;
    SVO_ARG(t1_left && out_t1_left && out_t1_right && out_t2_right && out_t2_left, "null pointer");
    SVO_HIP(hipSetDevice(ctx->device));
    const float2 *d_in;
    SVO_TRY(to_device(ctx, (const float2 *)t1_left, ctx->pts_in, (size_t)n, mem, &d_in));
    auto S = [&](int s) { return ctx->slots + (size_t)s * ctx->geom.slot_bytes; };
    LkArgs a{};
    fill_lk_common(ctx, a, n);
    a.ncalls = 4;
    // L1 -> R1 -> R2 -> L2 -> L1'   (src/tracking.cpp:593-618)
    a.prev[0] = S(slot_prevL); a.next[0] = S(slot_prevR);
    a.prev[1] = S(slot_prevR); a.next[1] = S(slot_curR);
    a.prev[2] = S(slot_curR);  a.next[2] = S(slot_curL);
    a.prev[3] = S(slot_curL);  a.next[3] = S(slot_prevL);
    a.pts_in = d_in;
    for (int i = 0; i < 4; i++) { a.pts_out[i] = ctx->pts_out[i]; a.status[i] = ctx->status[i]; }
    a.keep = ctx->keep;
    launch_lk(a, 1, n, ctx->stream);
    CompactArgs c{};
    c.keep = ctx->keep; c.n_pts = nullptr; c.n_fixed = n; c.pts_stride = 0; c.cap = n;
    c.in[0] = d_in; c.in[1] = ctx->pts_out[0]; c.in[2] = ctx->pts_out[1]; c.in[3] = ctx->pts_out[2];
    svo_pt2f *outs[4] = {out_t1_left, out_t1_right, out_t2_right, out_t2_left};
    for (int i = 0; i < 4; i++) c.out[i] = mem == SVO_MEM_DEVICE ? (float2 *)outs[i] : ctx->cmp[i];
    c.m_out = ctx->m_out;
    launch_compact(c, 1, ctx->stream);
    SVO_HIP(hipGetLastError());
    SVO_TRY(count_read(ctx, ctx->m_out, m_out));
    if (*m_out <= 0) return SVO_OK;
    for (int i = 0; i < 4; i++) SVO_TRY(from_device(ctx, (float2 *)outs[i], (const float2 *)c.out[i], (size_t)*m_out, mem));
    return io_done(ctx, mem);
}

extern "C" int svo_orb_extract(svo_ctx *ctx, const uint8_t *img, int pitch, int mem, svo_keypoint *kps, uint8_t *desc,
                               int cap, int *n_out, int *per_level)
{
    if (!ctx) return SVO_ERR_ARG;
    SVO_ARG(kps && desc && n_out && cap >= 0, "null output");
    SVO_HIP(hipSetDevice(ctx->device));
    int rc = orb_alloc(ctx);
    if (rc) return rc;
    const uint8_t *d; int dp;
    rc = resolve_image(ctx, img, pitch, mem, 0, &d, &dp);
    if (rc) return rc;
    rc = orb_extract_batch(ctx, d, nullptr, dp, 0, 0, 1, ctx->stream);
    if (rc) return rc;
    SVO_HIP(hipGetLastError());
    enum { kN = 0, kOverflow = 1, kPerLevel = 8 };           // positions in the pinned ints
    const int *h;
    SVO_TRY(count_fetch(ctx, kN, ctx->orb_n));
    SVO_TRY(count_fetch(ctx, kOverflow, ctx->orb_overflow));
    SVO_TRY(count_fetch(ctx, kPerLevel, ctx->orb_sel_cnt, ctx->orb_geom.nlevels));
    SVO_TRY(counts_wait(ctx, &h));
    const int n = h[kN];
    *n_out = n;
    if (h[kOverflow]) {
        ctx->err = (h[kOverflow] & 2) ? "ORB: FAST candidates exceed the per-cell (256) or per-level (4 * max_keypoints) capacity"
                   : (h[kOverflow] & 1) ? "ORB quadtree node pool overflow" : "ORB: keypoints exceed max_keypoints";
        return SVO_ERR_ARG;
    }
    if (per_level) for (int l = 0; l < 8; l++) per_level[l] = l < ctx->orb_geom.nlevels ? h[kPerLevel + l] : 0;
    if (n > cap) { ctx->err = "ORB: keypoints exceed caller capacity"; return SVO_ERR_ARG; }
    if (n == 0) return SVO_OK;
    svo_keypoint *hk;
    SVO_TRY(pinned_block(ctx, (sizeof(svo_keypoint) + 32) * (size_t)ctx->orb_kp_cap, &hk));
    uint8_t *hd = (uint8_t *)(hk + ctx->orb_kp_cap);
    SVO_TRY(from_device(ctx, hk, (const svo_keypoint *)ctx->orb_kps, (size_t)n, SVO_MEM_HOST));
    SVO_TRY(from_device(ctx, hd, (const uint8_t *)ctx->orb_desc, (size_t)32 * n, SVO_MEM_HOST));
    SVO_TRY(io_done(ctx, SVO_MEM_HOST));
    memcpy(kps, hk, sizeof(svo_keypoint) * (size_t)n);
    memcpy(desc, hd, (size_t)32 * n);
    return SVO_OK;
}

extern "C" int svo_orb_read_level(svo_ctx *ctx, int level, uint8_t *out, int *w, int *h)
{
    if (!ctx) return SVO_ERR_ARG;
    SVO_HIP(hipSetDevice(ctx->device));
    int rc = orb_alloc(ctx);
    if (rc) return rc;
    SVO_ARG(level >= 0 && level < ctx->orb_geom.nlevels, "level out of range");
    const OrbGeom &g = ctx->orb_geom;
    if (w) *w = g.w[level];
    if (h) *h = g.h[level];
    if (!out) return SVO_OK;
    // (svo_add_frame / the batch calls read level 0 in place from the caller's frames: image slot 0 then holds levels >= 1 only)
    SVO_ARG(level > 0 || ctx->orb_level0_in_slot, "level 0 was read in place from the input frame by the last extraction (svo_add_frame / batch): "
                                                  "it is the input image; svo_orb_extract copies it");
    SVO_HIP(hipMemcpy2DAsync(out, g.w[level], ctx->orb_slots + g.origin[level], g.pitch[level], g.w[level], g.h[level],
                             hipMemcpyDeviceToHost, ctx->stream));
    SVO_HIP(hipStreamSynchronize(ctx->stream));
    return SVO_OK;
}

extern "C" int svo_orb_read_candidates(svo_ctx *ctx, int level, float *out4, int cap, int *n_out)
{
    if (!ctx) return SVO_ERR_ARG;
    SVO_HIP(hipSetDevice(ctx->device));
    int rc = orb_alloc(ctx);
    if (rc) return rc;
    SVO_ARG(level >= 0 && level < ctx->orb_geom.nlevels && out4 && n_out, "bad argument");
    int n = 0;
    SVO_TRY(count_read(ctx, ctx->orb_lvl_cnt + level, &n));
    *n_out = n;
    if (n > cap) n = cap;
    if (n <= 0) return SVO_OK;
    SVO_TRY(from_device(ctx, (float4 *)out4, (const float4 *)ctx->orb_lvl_cand + (size_t)level * ctx->orb_cand_cap, (size_t)n, SVO_MEM_HOST));
    return io_done(ctx, SVO_MEM_HOST);
}

extern "C" int svo_match_hamming(svo_ctx *ctx, const uint8_t *query, int nq, const uint8_t *train, int nt,
                                 int32_t *train_idx, float *distance, int mem)
{
    if (!ctx) return SVO_ERR_ARG;
    SVO_ARG(mem == SVO_MEM_HOST || mem == SVO_MEM_DEVICE, "bad mem");
    SVO_HIP(hipSetDevice(ctx->device));
    int rc = orb_alloc(ctx);
    if (rc) return rc;
    SVO_ARG(nq >= 0 && nt >= 0 && nq <= ctx->orb_kp_cap && nt <= ctx->orb_kp_cap, "descriptor count exceeds max_keypoints");
    if (nq == 0) return SVO_OK;
    SVO_ARG(query && train_idx && distance && (train || nt == 0), "null pointer");
    if (svo_wait_results(ctx) != SVO_OK) return SVO_ERR_HIP;
    const uint8_t *dq, *dt;                                  // host descriptors: staged through the descriptor slots of image 0 / 1
    SVO_TRY(to_device(ctx, query, ctx->orb_desc, (size_t)32 * nq, mem, &dq));
    SVO_TRY(to_device(ctx, train, ctx->orb_desc + (size_t)32 * ctx->orb_kp_cap, (size_t)32 * nt, mem, &dt));
    orb_launch_match_fixed(ctx, dq, nq, dt, nt, ctx->stream);
    SVO_HIP(hipGetLastError());
    SVO_TRY(from_device(ctx, train_idx, (const int32_t *)ctx->orb_midx[0], (size_t)nq, mem));
    SVO_TRY(from_device(ctx, distance, (const float *)ctx->orb_mdist[0], (size_t)nq, mem));
    return io_done(ctx, mem);
}

extern "C" int svo_triangulate(svo_ctx *ctx, const double P1[12], const double P2[12], const svo_pt2f *x1,
                               const svo_pt2f *x2, int n, svo_pt3f *out, int mem)
{
    if (!ctx) return SVO_ERR_ARG;
    if (svo_wait_results(ctx) != SVO_OK) return SVO_ERR_HIP;     // shares X3 / cmp with a pending pose stage
    return stage_triangulate(ctx, P1, P2, x1, x2, n, out, mem);
}

extern "C" int svo_pnp_ransac(svo_ctx *ctx, const svo_pt3f *obj, const svo_pt2f *img, int n, const double K[9],
                              int iterations, float reproj_err, double confidence, svo_pnp_result *res,
                              uint8_t *inlier_mask, int mem)
{
    if (!ctx) return SVO_ERR_ARG;
    if (svo_wait_results(ctx) != SVO_OK) return SVO_ERR_HIP;
    return stage_pnp_ransac(ctx, obj, img, n, K, iterations, reproj_err, confidence, res, inlier_mask, mem);
}

extern "C" int svo_reset(svo_ctx *ctx)
{
    if (!ctx) return SVO_ERR_ARG;
    ctx->online_frames = 0; ctx->online_cur = 0;
    chain_event(ctx, kChainNew);
    pose_identity16(ctx->pose);
    return SVO_OK;
}

extern "C" int svo_get_pose(svo_ctx *ctx, double pose[16])
{
    if (!ctx || !pose) return SVO_ERR_ARG;
    memcpy(pose, ctx->pose, sizeof(double) * 16);
    return SVO_OK;
}

extern "C" int svo_set_pose(svo_ctx *ctx, const double pose[16])
{
    if (!ctx || !pose) return SVO_ERR_ARG;
    memcpy(ctx->pose, pose, sizeof(double) * 16);
    chain_event(ctx, kChainPoseSet);
    return SVO_OK;
}

// ---- host-resident frame batches ---------------------------------------------------------------
// ctx may be NULL (ABI v6): page-locked memory does not belong to a context or a device (hipHostMallocPortable), so a
// runner can pin its frame buffers on one thread WHILE svo_create builds the context on another -- on a short run
// page-locking half a gigabyte (0.25 ms per MB) and context creation are each a quarter of the wall time.
extern "C" int svo_host_alloc(svo_ctx *ctx, size_t bytes, void **out)
{
    if (!out || bytes == 0) { if (ctx) ctx->err = "bad argument: null output / zero size"; return SVO_ERR_ARG; }
    *out = nullptr;
    if (ctx && hipSetDevice(ctx->device) != hipSuccess) { ctx->err = "hipSetDevice failed"; return SVO_ERR_HIP; }
    const hipError_t e = hipHostMalloc(out, bytes, hipHostMallocPortable);
    if (e != hipSuccess) {
        if (ctx) ctx->err = std::string("hipHostMalloc: ") + hipGetErrorString(e);
        return SVO_ERR_HIP;
    }
    return SVO_OK;
}

extern "C" int svo_host_free(svo_ctx *ctx, void *p)
{
    if (p && hipHostFree(p) != hipSuccess) { if (ctx) ctx->err = "hipHostFree failed"; return SVO_ERR_HIP; }
    return SVO_OK;
}

// ---- the frame input path: every entry point that takes frames, plain (frames of the context's size) or ingest (source-size
// frames, resized on the device first), goes through one function per family.  That function takes the frame size (w x h) to
// check against and whether a resize goes in front, states the family's argument rules once -- pointers, counts, pitch / stride,
// mem / results_mem, stream ids -- and runs them before anything is copied or launched.
#define SVO_INGEST_ON() do { if (!ctx->ingest.on) { ctx->err = "no ingest stage (svo_ingest_create)"; return SVO_ERR_STATE; } } while (0)

static size_t work_frame_bytes(const svo_ctx *ctx) { return (size_t)ctx->stage_pitch * ctx->cfg.height; }
static size_t src_frame_bytes(const svo_ctx *ctx) { return (size_t)ctx->ingest.spitch * ctx->ingest.sh; }
// Frames per eye of a frame buffer, of the ingest stage's working frames and of the staging behind them.
static size_t frame_slots(const svo_ctx *ctx) { return (size_t)ctx->cfg.max_batch + 1; }

// n HOST frames of w x h (frame f at src + f * sstride) -> DEVICE frames (frame f at dst + f * dstride), on `st`.  The device frames are dense
// (dstride = dpitch * h): a source laid out the same way goes as one copy.
static int copy_host_frames(svo_ctx *ctx, uint8_t *dst, int dpitch, int64_t dstride, const uint8_t *src, int spitch, int64_t sstride,
                            int w, int h, int n, hipStream_t st)
{
    if (spitch == dpitch && (n == 1 || sstride == dstride)) {
        SVO_HIP(hipMemcpyAsync(dst, src, (size_t)dstride * (size_t)n, hipMemcpyHostToDevice, st));
        return SVO_OK;
    }
    for (int f = 0; f < n; f++)
        SVO_HIP(hipMemcpy2DAsync(dst + f * dstride, (size_t)dpitch, src + f * sstride, (size_t)spitch, (size_t)w, (size_t)h,
                                 hipMemcpyHostToDevice, st));
    return SVO_OK;
}

// One HOST frame pair of the context's size -> the pinned staging of the online step.
static int stage_host_pair(svo_ctx *ctx, const uint8_t **left, const uint8_t **right, int *pitch)
{
    const int hp = *pitch;
    int rc = svo::stage_host_image(ctx, *left, hp, 0, left, pitch);
    if (rc) return rc;
    return svo::stage_host_image(ctx, *right, hp, 1, right, pitch);
}

// n source-size HOST frames per eye -> the ingest stage's device staging, on the context's stream; the caller's memory is free
// again when this returns.
static int ingest_stage_host(svo_ctx *ctx, const uint8_t **left, const uint8_t **right, int *pitch, int64_t *frame_stride, int n)
{
    Ingest &g = ctx->ingest;
    const size_t fbytes = src_frame_bytes(ctx);
    if (dev_reserve(ctx, &g.src_stage, 2 * fbytes * (size_t)n) != SVO_OK) return SVO_ERR_HIP;
    const uint8_t *src[2] = {*left, *right};
    for (int eye = 0; eye < 2; eye++) {
        const int rc = copy_host_frames(ctx, g.src_stage.base + (size_t)eye * fbytes * (size_t)n, g.spitch, (int64_t)fbytes, src[eye], *pitch,
                                        *frame_stride, g.sw, g.sh, n, ctx->stream);
        if (rc) return rc;
    }
    SVO_HIP(hipStreamSynchronize(ctx->stream));
    *left = g.src_stage.base; *right = g.src_stage.base + fbytes * (size_t)n;
    *pitch = g.spitch; *frame_stride = (int64_t)fbytes;
    return SVO_OK;
}

// n source-size DEVICE frames per eye -> working frame slots 0 .. n-1 of the ingest stage, on the context's stream.
static int ingest_resize(svo_ctx *ctx, const uint8_t **left, const uint8_t **right, int *pitch, int64_t *frame_stride, int n)
{
    uint8_t *wL = ctx->ingest.work, *wR = wL + frame_slots(ctx) * work_frame_bytes(ctx);
    const int rc = resize_launch(ctx, ctx->ingest.tab, *left, *right, *pitch, *frame_stride, wL, wR, ctx->stage_pitch,
                                 (int64_t)work_frame_bytes(ctx), n, ctx->stream);
    *left = wL; *right = wR;
    *pitch = ctx->stage_pitch; *frame_stride = (int64_t)work_frame_bytes(ctx);
    return rc;
}

// ---- svo_add_frame / svo_ingest_add_frame
static int add_frame(svo_ctx *ctx, int w, bool resize, const uint8_t *left, const uint8_t *right, int pitch, int mem,
                     svo_step_result *res)
{
    SVO_ARG(left && right && res, "null pointer");
    SVO_ARG(pitch >= w, (resize ? "pitch < source width" : "pitch < width"));
    SVO_ARG(mem == SVO_MEM_HOST || mem == SVO_MEM_DEVICE, "bad mem");
    SVO_HIP(hipSetDevice(ctx->device));
    int64_t frame_stride = 0;                               // one frame per eye
    int rc = SVO_OK;
    if (mem == SVO_MEM_HOST)
        rc = resize ? ingest_stage_host(ctx, &left, &right, &pitch, &frame_stride, 1) : stage_host_pair(ctx, &left, &right, &pitch);
    if (rc == SVO_OK && resize) rc = ingest_resize(ctx, &left, &right, &pitch, &frame_stride, 1);
    if (rc) return rc;
    return pipeline_add_frame(ctx, left, right, pitch, res);
}

extern "C" int svo_add_frame(svo_ctx *ctx, const uint8_t *left, const uint8_t *right, int pitch, int mem,
                             svo_step_result *res)
{
    if (!ctx) return SVO_ERR_ARG;
    return add_frame(ctx, ctx->cfg.width, false, left, right, pitch, mem, res);
}

extern "C" int svo_ingest_add_frame(svo_ctx *ctx, const uint8_t *left, const uint8_t *right, int pitch, int mem, svo_step_result *res)
{
    if (!ctx) return SVO_ERR_ARG;
    SVO_INGEST_ON();
    return add_frame(ctx, ctx->ingest.sw, true, left, right, pitch, mem, res);
}

// ---- svo_track_batch / svo_ingest_track_batch (DEVICE frames), and the batches of a frame buffer (svo_track_uploaded*)
// results == NULL with SVO_MEM_DEVICE: the records stay in the context (svo_collect_results)
static int track_batch(svo_ctx *ctx, int w, int h, bool resize, const uint8_t *lefts, const uint8_t *rights, int pitch,
                       int64_t frame_stride, int n_frames, const double *pose0, svo_step_result *results, int results_mem,
                       int carry_first = 0)
{
    SVO_ARG(lefts && rights && (results || results_mem == SVO_MEM_DEVICE), "null pointer");
    SVO_ARG(n_frames >= 2 && n_frames - 1 <= ctx->cfg.max_batch, "n_frames - 1 must be in [1, max_batch]");
    SVO_ARG(pitch >= w && frame_stride >= (int64_t)pitch * h, "bad pitch / frame_stride");
    SVO_ARG(results_mem == SVO_MEM_HOST || results_mem == SVO_MEM_DEVICE, "bad results_mem");
    if (ctx->carry.on) {
        ctx->err = "track carry is on (svo_set_track_carry): a batch treats its pairs as independent; use svo_add_frame / svo_streams_step";
        return SVO_ERR_STATE;
    }
    SVO_HIP(hipSetDevice(ctx->device));
    if (resize) {
        const int rc = ingest_resize(ctx, &lefts, &rights, &pitch, &frame_stride, n_frames);
        if (rc) return rc;
    }
    return pipeline_track_batch(ctx, lefts, rights, pitch, frame_stride, n_frames, pose0, results, results_mem, carry_first);
}

extern "C" int svo_track_batch(svo_ctx *ctx, const uint8_t *left_frames, const uint8_t *right_frames,
                               int pitch, int64_t frame_stride, int n_frames, const double *pose0,
                               svo_step_result *results, int results_mem)
{
    if (!ctx) return SVO_ERR_ARG;
    return track_batch(ctx, ctx->cfg.width, ctx->cfg.height, false, left_frames, right_frames, pitch, frame_stride, n_frames, pose0,
                       results, results_mem);
}

extern "C" int svo_ingest_track_batch(svo_ctx *ctx, const uint8_t *lefts, const uint8_t *rights, int pitch, int64_t frame_stride,
                                      int n_frames, const double *pose0, svo_step_result *results, int results_mem)
{
    if (!ctx) return SVO_ERR_ARG;
    SVO_INGEST_ON();
    return track_batch(ctx, ctx->ingest.sw, ctx->ingest.sh, true, lefts, rights, pitch, frame_stride, n_frames, pose0, results,
                       results_mem);
}

// ---- svo_upload_frames_at / svo_ingest_upload_frames_at: HOST frames -> frame buffer `buf`, everything on the copy stream.
// With an ingest stage the copy lands in source-size staging and the resize fills the frame buffer, so everything behind
// ev_up[buf] works unchanged.
static int frame_buffers(svo_ctx *ctx)
{
    if (ctx->copy_stream) return SVO_OK;
    const size_t per_cam = work_frame_bytes(ctx) * frame_slots(ctx);
    // a call that failed half way leaves what it made for the next attempt (copy_stream, made last, is what marks the set complete)
    for (int k = 0; k < 2; k++) {
        if (!ctx->fb[k] && dev_alloc(ctx, &ctx->fb[k], 2 * per_cam) != SVO_OK) return SVO_ERR_HIP;
        if (dev_event(ctx, &ctx->ev_up[k]) != SVO_OK || dev_event(ctx, &ctx->ev_fb_free[k]) != SVO_OK) return SVO_ERR_HIP;
    }
    return dev_stream(ctx, &ctx->copy_stream);
}

// svo_track_uploaded_async's two record buffers, their events and the stream that fetches them
static int async_ring(svo_ctx *ctx)
{
    if (ctx->async_ready) return SVO_OK;
    for (int k = 0; k < 2; k++) {
        if (!ctx->d_async[k] && dev_alloc(ctx, &ctx->d_async[k], sizeof(svo_step_result) * (size_t)ctx->cfg.max_batch) != SVO_OK) return SVO_ERR_HIP;
        if (dev_event(ctx, &ctx->ev_async[k]) != SVO_OK) return SVO_ERR_HIP;
    }
    if (dev_stream(ctx, &ctx->fetch_stream) != SVO_OK) return SVO_ERR_HIP;
    ctx->async_ready = true;
    return SVO_OK;
}

static int upload_frames_at(svo_ctx *ctx, int w, int h, bool resize, int buf, int first_slot, const uint8_t *lefts, const uint8_t *rights,
                            int pitch, int64_t frame_stride, int n_frames)
{
    SVO_ARG(buf == 0 || buf == 1, "buf must be 0 or 1");
    SVO_ARG(lefts && rights, "null frames");
    SVO_ARG(first_slot >= 0 && n_frames >= 1 && first_slot + n_frames <= ctx->cfg.max_batch + 1, "first_slot + n_frames must be in [1, max_batch + 1]");
    // slot 0 is either uploaded or carried on the device (SVO_CONTINUE_CARRY_FRAME): nothing else may be left out
    SVO_ARG(first_slot <= 1, "first_slot must be 0 (a whole batch) or 1 (frame 0 is carried on the device)");
    SVO_ARG(pitch >= w && frame_stride >= (int64_t)pitch * h, "bad pitch / frame_stride");
    SVO_HIP(hipSetDevice(ctx->device));
    int rc = frame_buffers(ctx);
    if (rc) return rc;
    Ingest &g = ctx->ingest;
    const size_t sbytes = src_frame_bytes(ctx), fbytes = work_frame_bytes(ctx);
    if (resize && !g.up_stage[buf] && dev_alloc(ctx, &g.up_stage[buf], 2 * sbytes * frame_slots(ctx)) != SVO_OK) return SVO_ERR_HIP;
    // where the copy lands: the frame buffer itself, or the staging behind it
    uint8_t *base = resize ? g.up_stage[buf] : ctx->fb[buf];
    const size_t dbytes = resize ? sbytes : fbytes;
    const int dpitch = resize ? g.spitch : ctx->stage_pitch;
    // the batch that last read this buffer must have been ingested (the staging behind it is reused in copy-stream order)
    if (ctx->fb_used[buf]) SVO_HIP(hipStreamWaitEvent(ctx->copy_stream, ctx->ev_fb_free[buf], 0));
    const uint8_t *src[2] = {lefts, rights};
    uint8_t *dst[2];
    for (int cam = 0; cam < 2; cam++) {
        dst[cam] = base + ((size_t)cam * frame_slots(ctx) + (size_t)first_slot) * dbytes;
        rc = copy_host_frames(ctx, dst[cam], dpitch, (int64_t)dbytes, src[cam], pitch, frame_stride, w, h, n_frames, ctx->copy_stream);
        if (rc) return rc;
    }
    if (resize) {
        uint8_t *dL = ctx->fb[buf] + (size_t)first_slot * fbytes;
        rc = resize_launch(ctx, g.tab, dst[0], dst[1], g.spitch, (int64_t)sbytes, dL, dL + frame_slots(ctx) * fbytes, ctx->stage_pitch,
                           (int64_t)fbytes, n_frames, ctx->copy_stream);
        if (rc) return rc;
    }
    SVO_HIP(hipEventRecord(ctx->ev_up[buf], ctx->copy_stream));
    ctx->fb_frames[buf] = first_slot + n_frames;
    ctx->fb_first[buf] = first_slot;
    return SVO_OK;
}

extern "C" int svo_upload_frames_at(svo_ctx *ctx, int buf, int first_slot, const uint8_t *left_frames, const uint8_t *right_frames,
                                    int pitch, int64_t frame_stride, int n_frames)
{
    if (!ctx) return SVO_ERR_ARG;
    return upload_frames_at(ctx, ctx->cfg.width, ctx->cfg.height, false, buf, first_slot, left_frames, right_frames, pitch, frame_stride,
                            n_frames);
}

extern "C" int svo_ingest_upload_frames_at(svo_ctx *ctx, int buf, int first_slot, const uint8_t *lefts, const uint8_t *rights,
                                           int pitch, int64_t frame_stride, int n_frames)
{
    if (!ctx) return SVO_ERR_ARG;
    SVO_INGEST_ON();
    return upload_frames_at(ctx, ctx->ingest.sw, ctx->ingest.sh, true, buf, first_slot, lefts, rights, pitch, frame_stride, n_frames);
}

extern "C" int svo_upload_frames(svo_ctx *ctx, int buf, const uint8_t *left_frames, const uint8_t *right_frames,
                                 int pitch, int64_t frame_stride, int n_frames)
{
    return svo_upload_frames_at(ctx, buf, 0, left_frames, right_frames, pitch, frame_stride, n_frames);
}

extern "C" int svo_wait_upload(svo_ctx *ctx, int buf)
{
    if (!ctx) return SVO_ERR_ARG;
    SVO_ARG(buf == 0 || buf == 1, "buf must be 0 or 1");
    SVO_ARG(ctx->fb_frames[buf] > 0, "nothing uploaded into this buffer");
    SVO_HIP(hipEventSynchronize(ctx->ev_up[buf]));
    return SVO_OK;
}

extern "C" int svo_track_uploaded(svo_ctx *ctx, int buf, int n_frames, const double *pose0,
                                  svo_step_result *results, int results_mem)
{
    if (!ctx) return SVO_ERR_ARG;
    SVO_ARG(buf == 0 || buf == 1, "buf must be 0 or 1");
    SVO_ARG(n_frames >= 2 && n_frames <= ctx->fb_frames[buf], "n_frames exceeds what was uploaded");
    // an upload that started at slot 1 left slot 0 to a carried frame: only an async launch with SVO_CONTINUE_CARRY_FRAME reads it
    SVO_ARG(ctx->fb_first[buf] == 0, "frame slot 0 of this buffer was not uploaded (svo_upload_frames_at first_slot = 1): "
                                     "launch it with svo_track_uploaded_async and SVO_CONTINUE_CARRY_FRAME");
    SVO_HIP(hipSetDevice(ctx->device));
    const size_t fbytes = work_frame_bytes(ctx), per_cam = fbytes * frame_slots(ctx);
    SVO_HIP(hipStreamWaitEvent(ctx->stream, ctx->ev_up[buf], 0));
    int rc = track_batch(ctx, ctx->cfg.width, ctx->cfg.height, false, ctx->fb[buf], ctx->fb[buf] + per_cam, ctx->stage_pitch,
                         (int64_t)fbytes, n_frames, pose0, results, results_mem);
    if (rc < 0) return rc;
    SVO_HIP(hipEventRecord(ctx->ev_fb_free[buf], ctx->stream));
    ctx->fb_used[buf] = true;
    return rc;
}

extern "C" int svo_track_uploaded_async(svo_ctx *ctx, int buf, int n_frames, const double *pose0, int continue_chain)
{
    if (!ctx) return SVO_ERR_ARG;
    SVO_ARG(buf == 0 || buf == 1, "buf must be 0 or 1");
    SVO_ARG(n_frames >= 2 && n_frames <= ctx->fb_frames[buf], "n_frames exceeds what was uploaded");
    SVO_ARG(ctx->async_tail - ctx->async_head < 2, "two batches are already outstanding: collect one first");
    SVO_HIP(hipSetDevice(ctx->device));
    const int r = (int)(ctx->async_tail & 1), n_pairs = n_frames - 1;
    if (async_ring(ctx) != SVO_OK) return SVO_ERR_HIP;       // an online-sized context (max_batch 1) sets the ring up on first use
    SVO_ARG((continue_chain & ~(SVO_CONTINUE_CHAIN | SVO_CONTINUE_CARRY_FRAME)) == 0, "unknown continue_chain bits");
    SVO_ARG(!(continue_chain & SVO_CONTINUE_CARRY_FRAME) || (continue_chain & SVO_CONTINUE_CHAIN),
            "SVO_CONTINUE_CARRY_FRAME without SVO_CONTINUE_CHAIN: the carried frame belongs to the chain being continued");
    SVO_ARG(ctx->fb_first[buf] == 0 || (continue_chain & SVO_CONTINUE_CARRY_FRAME),
            "frame slot 0 of this buffer was not uploaded (svo_upload_frames_at first_slot = 1): it holds stale pixels unless the "
            "launch carries the previous batch's last frame (SVO_CONTINUE_CHAIN | SVO_CONTINUE_CARRY_FRAME)");
    if (continue_chain) {
        SVO_ARG(ctx->async_tail > 0, "continue_chain needs a previous async batch");
        const int pr = r ^ 1;
        SVO_ARG(ctx->async_last_pairs > 0, "continue_chain needs a previous async batch");
        ctx->seed_dev = ctx->d_async[pr][ctx->async_last_pairs - 1].pose;
    }
    const size_t fbytes = work_frame_bytes(ctx), per_cam = fbytes * frame_slots(ctx);
    SVO_HIP(hipStreamWaitEvent(ctx->stream, ctx->ev_up[buf], 0));
    int rc = track_batch(ctx, ctx->cfg.width, ctx->cfg.height, false, ctx->fb[buf], ctx->fb[buf] + per_cam, ctx->stage_pitch,
                         (int64_t)fbytes, n_frames, continue_chain ? nullptr : pose0, ctx->d_async[r], SVO_MEM_DEVICE,
                         (continue_chain & SVO_CONTINUE_CARRY_FRAME) != 0);
    ctx->seed_dev = nullptr;
    if (rc < 0) return rc;
    SVO_HIP(hipEventRecord(ctx->ev_fb_free[buf], ctx->stream));
    ctx->fb_used[buf] = true;
    // the records land in d_async[r] at the end of the pose stage, wherever that ran
    SVO_HIP(hipEventRecord(ctx->ev_async[r], ctx->back_pending ? ctx->side_stream : ctx->stream));
    ctx->async_n[r] = n_pairs;
    ctx->async_last_pairs = n_pairs;
    ctx->async_tail++;
    ctx->carry_slot = n_pairs;                   // frame slot n_pairs now holds this batch's last frame
    return rc;
}

// Non-blocking companion of svo_collect_results (ABI v6): a streaming caller polls between frames.
extern "C" int svo_results_ready(svo_ctx *ctx, int *n_pairs)
{
    if (!ctx) return SVO_ERR_ARG;
    SVO_ARG(n_pairs, "null output");
    *n_pairs = 0;
    if (ctx->async_tail == ctx->async_head) return SVO_OK;
    const int r = (int)(ctx->async_head & 1);
    SVO_HIP(hipSetDevice(ctx->device));
    const hipError_t e = hipEventQuery(ctx->ev_async[r]);
    if (e == hipSuccess) *n_pairs = ctx->async_n[r];
    else if (e != hipErrorNotReady) SVO_HIP(e);
    return SVO_OK;
}

extern "C" int svo_collect_results(svo_ctx *ctx, svo_step_result *results, int n_pairs)
{
    if (!ctx) return SVO_ERR_ARG;
    SVO_ARG(ctx->async_tail != ctx->async_head, "no outstanding batch");
    const int r = (int)(ctx->async_head & 1);
    SVO_ARG(results && n_pairs >= 1 && n_pairs <= ctx->async_n[r], "the oldest outstanding batch has fewer pairs");
    SVO_HIP(hipSetDevice(ctx->device));
    // wait for THAT batch only (its successor may be running), then fetch on a stream of its own: the
    // copy stream may be busy with the next chunk's upload
    SVO_HIP(hipEventSynchronize(ctx->ev_async[r]));
    const int rc = deliver_records(ctx, ctx->d_async[r], n_pairs, results, SVO_MEM_HOST, ctx->fetch_stream);
    if (rc) return rc;
    ctx->async_n[r] = 0;
    ctx->async_head++;
    return SVO_OK;
}

// ---- stream sets: N independent live streams of one context, any subset advanced by one frame each per call --------
extern "C" int svo_streams_create(svo_ctx *ctx, int n_streams)
{
    if (!ctx) return SVO_ERR_ARG;
    return pipeline_streams_create(ctx, n_streams);
}

extern "C" int svo_streams_count(const svo_ctx *ctx, int *n_streams)
{
    if (!ctx || !n_streams) return SVO_ERR_ARG;
    *n_streams = ctx->streams.n;
    return SVO_OK;
}

// svo_streams_step / svo_ingest_streams_step.  HOST frames are staged first -- source-size ones in the ingest stage's staging, one
// frame of the context's size in the pinned staging of svo_add_frame, several in frame buffer 0 of svo_upload_frames -- and the
// caller's memory is free again when the call returns.
static int streams_step(svo_ctx *ctx, int w, int h, bool resize, const int32_t *stream_ids, int m, const uint8_t *lefts,
                        const uint8_t *rights, int pitch, int64_t frame_stride, int mem, svo_step_result *results, int results_mem)
{
    if (ctx->win.frames > 0) { ctx->err = "the sliding window (svo_set_window_ba) works on the online chain only: stream sets have no table yet"; return SVO_ERR_STATE; }
    if (ctx->kf.on) { ctx->err = "keyframe mode (svo_set_keyframe) works on the online chain only: stream sets have no keyframe yet"; return SVO_ERR_STATE; }
    SVO_ARG(ctx->streams.n > 0, "no stream set (svo_streams_create)");
    SVO_ARG(stream_ids && lefts && rights && (results || results_mem == SVO_MEM_DEVICE), "null pointer");
    SVO_ARG(m >= 1 && m <= (ctx->cfg.max_batch + 1) / 2, "m must be in [1, (max_batch + 1) / 2]");
    SVO_ARG(pitch >= w && (m == 1 || frame_stride >= (int64_t)pitch * h), "bad pitch / frame_stride");
    SVO_ARG(mem == SVO_MEM_HOST || mem == SVO_MEM_DEVICE, "bad mem");
    SVO_ARG(results_mem == SVO_MEM_HOST || results_mem == SVO_MEM_DEVICE, "bad results_mem");
    int rc = pipeline_streams_check_ids(ctx, stream_ids, m);
    if (rc) return rc;
    SVO_HIP(hipSetDevice(ctx->device));
    bool in_fb0 = false;
    if (mem == SVO_MEM_HOST) {
        if (resize) {
            rc = ingest_stage_host(ctx, &lefts, &rights, &pitch, &frame_stride, m);
        } else if (m == 1) {
            rc = stage_host_pair(ctx, &lefts, &rights, &pitch);
        } else {
            rc = upload_frames_at(ctx, w, h, false, 0, 0, lefts, rights, pitch, frame_stride, m);
            if (rc) return rc;
            SVO_HIP(hipEventSynchronize(ctx->ev_up[0]));
            ctx->fb_frames[0] = 0;                          // (not a batch a later svo_track_uploaded may claim)
            lefts = ctx->fb[0]; rights = ctx->fb[0] + frame_slots(ctx) * work_frame_bytes(ctx);
            pitch = ctx->stage_pitch; frame_stride = (int64_t)work_frame_bytes(ctx);
            in_fb0 = true;
        }
        if (rc) return rc;
    }
    if (resize) {
        rc = ingest_resize(ctx, &lefts, &rights, &pitch, &frame_stride, m);
        if (rc) return rc;
    }
    rc = pipeline_streams_step(ctx, stream_ids, m, lefts, rights, pitch, frame_stride, results, results_mem);
    if (in_fb0) {                                           // whatever the step has queued reads frame buffer 0
        SVO_HIP(hipEventRecord(ctx->ev_fb_free[0], ctx->stream));
        ctx->fb_used[0] = true;
    }
    return rc;
}

extern "C" int svo_streams_step(svo_ctx *ctx, const int32_t *stream_ids, int m, const uint8_t *left_frames,
                                const uint8_t *right_frames, int pitch, int64_t frame_stride, int mem,
                                svo_step_result *results, int results_mem)
{
    if (!ctx) return SVO_ERR_ARG;
    return streams_step(ctx, ctx->cfg.width, ctx->cfg.height, false, stream_ids, m, left_frames, right_frames, pitch, frame_stride, mem,
                        results, results_mem);
}

extern "C" int svo_ingest_streams_step(svo_ctx *ctx, const int32_t *stream_ids, int m, const uint8_t *lefts, const uint8_t *rights,
                                       int pitch, int64_t frame_stride, int mem, svo_step_result *results, int results_mem)
{
    if (!ctx) return SVO_ERR_ARG;
    SVO_INGEST_ON();
    return streams_step(ctx, ctx->ingest.sw, ctx->ingest.sh, true, stream_ids, m, lefts, rights, pitch, frame_stride, mem, results,
                        results_mem);
}

extern "C" int svo_streams_reset(svo_ctx *ctx, int stream_id)
{
    if (!ctx) return SVO_ERR_ARG;
    return pipeline_streams_reset(ctx, stream_id);
}

extern "C" int svo_streams_get_pose(svo_ctx *ctx, int stream_id, double pose[16])
{
    if (!ctx) return SVO_ERR_ARG;
    return pipeline_streams_get_pose(ctx, stream_id, pose);
}

extern "C" int svo_streams_set_pose(svo_ctx *ctx, int stream_id, const double pose[16])
{
    if (!ctx) return SVO_ERR_ARG;
    return pipeline_streams_set_pose(ctx, stream_id, pose);
}

// ---- ingest stage: source-size frames resized on the device into working-size frames the entry points above read --------
// (the kernel, the tap tables, svo_resize and svo_scale_projection: resize.hip)
extern "C" int svo_ingest_create(svo_ctx *ctx, int src_width, int src_height, int interp, double fx, double fy)
{
    if (!ctx) return SVO_ERR_ARG;
    Ingest &g = ctx->ingest;
    SVO_ARG(!g.on, "the context already has an ingest stage");
    SVO_HIP(hipSetDevice(ctx->device));
    int tab = -1;
    int rc = resize_plan(ctx, src_width, src_height, ctx->cfg.width, ctx->cfg.height, interp, fx, fy, &tab);
    if (rc) return rc;
    if (!g.work && dev_alloc(ctx, &g.work, 2 * work_frame_bytes(ctx) * frame_slots(ctx)) != SVO_OK) return SVO_ERR_HIP;
    g.sw = src_width; g.sh = src_height; g.tab = tab;
    g.spitch = (src_width + 15) & ~15;
    g.on = true;
    return SVO_OK;
}

extern "C" int svo_ingest_info(const svo_ctx *ctx, int *src_width, int *src_height, int *interp, double *inv_x, double *inv_y)
{
    if (!ctx) return SVO_ERR_ARG;
    if (!ctx->ingest.on) return SVO_ERR_STATE;
    const ResizeTab &t = ctx->resize_tabs[(size_t)ctx->ingest.tab];
    if (src_width) *src_width = t.sw;
    if (src_height) *src_height = t.sh;
    if (interp) *interp = t.interp;
    if (inv_x) *inv_x = t.inv_x;
    if (inv_y) *inv_y = t.inv_y;
    return SVO_OK;
}

extern "C" int svo_chain_relative(svo_ctx *ctx, const double *T_rel_inv, const int32_t *ok, int n, const double *pose0,
                                  double *poses_out, int mem)
{
    if (!ctx) return SVO_ERR_ARG;
    SVO_HIP(hipSetDevice(ctx->device));
    return stage_chain_relative(ctx, T_rel_inv, ok, n, pose0, poses_out, mem);
}

// ---- read-back of the online state: what the reference keeps in Frame::features_* / shows in
// displayTracking ------------------------------------------------------------------------------
extern "C" int svo_get_frame_keypoints(svo_ctx *ctx, int side, svo_keypoint *kps, uint8_t *descriptors, int cap, int *n_out)
{
    if (!ctx) return SVO_ERR_ARG;
    SVO_ARG(n_out && cap >= 0 && (kps || cap == 0), "null output");
    SVO_ARG(side == 0 || side == 1, "side must be 0 (left) or 1 (right)");
    SVO_ARG(ctx->online_frames > 0, "no frame has been added");
    SVO_HIP(hipSetDevice(ctx->device));
    if (svo_wait_results(ctx) != SVO_OK) return SVO_ERR_HIP;
    const int cur = ctx->online_cur;
    *n_out = 0;
    if (ctx->cfg.track_mode == SVO_MODE_ORB) {
        const int slot = 2 * cur + side, kcap = ctx->orb_kp_cap;
        int n = 0;
        SVO_TRY(count_read(ctx, ctx->orb_n + slot, &n));
        n = n < kcap ? n : kcap;
        SVO_ARG(n <= cap, "keypoint capacity too small");
        if (n > 0) {
            SVO_TRY(from_device(ctx, kps, (const svo_keypoint *)ctx->orb_kps + (size_t)slot * kcap, (size_t)n, SVO_MEM_HOST));
            SVO_TRY(from_device(ctx, descriptors, (const uint8_t *)ctx->orb_desc + (size_t)slot * kcap * 32, (size_t)32 * n, SVO_MEM_HOST));
            SVO_TRY(io_done(ctx, SVO_MEM_HOST));
        }
        *n_out = n;
        return SVO_OK;
    }
    SVO_ARG(side == 0, "LK mode detects on the left image only (src/tracking.cpp:94-113)");
    const int kcap = ctx->cfg.max_keypoints;
    int n = 0;
    SVO_TRY(count_read(ctx, ctx->kp_n + cur, &n));
    n = n < kcap ? n : kcap;
    SVO_ARG(n <= cap, "keypoint capacity too small");
    if (n > 0) {
        std::vector<float2> xy((size_t)n);
        std::vector<float> resp((size_t)n);
        SVO_TRY(from_device(ctx, xy.data(), (const float2 *)ctx->kp_xy + (size_t)cur * kcap, (size_t)n, SVO_MEM_HOST));
        SVO_TRY(from_device(ctx, resp.data(), (const float *)ctx->kp_resp + (size_t)cur * kcap, (size_t)n, SVO_MEM_HOST));
        SVO_TRY(io_done(ctx, SVO_MEM_HOST));
        // (a frame keeps the records of the detector that made them when svo_set_lk_detector switches between two frames)
        format_keypoints(xy.data(), resp.data(), n, kps);
    }
    *n_out = n;
    return SVO_OK;
}

// The four point lists and the inlier mask of n tracks that start at `offset` in the pair buffers (null: not wanted).
static int read_tracks(svo_ctx *ctx, size_t offset, int n, svo_pt2f *t1_left, svo_pt2f *t1_right, svo_pt2f *t2_right, svo_pt2f *t2_left,
                       uint8_t *inlier)
{
    svo_pt2f *dst[4] = {t1_left, t1_right, t2_right, t2_left};
    for (int k = 0; k < 4; k++) {
        if (!dst[k]) continue;
        if (k == 2 && ctx->cfg.track_mode == SVO_MODE_ORB) { memset(dst[k], 0, sizeof(svo_pt2f) * (size_t)n); continue; }
        SVO_TRY(from_device(ctx, (float2 *)dst[k], (const float2 *)ctx->cmp[k] + offset, (size_t)n, SVO_MEM_HOST));
    }
    SVO_TRY(from_device(ctx, inlier, pnp_inlier_mask(ctx) + offset, (size_t)n, SVO_MEM_HOST));
    return io_done(ctx, SVO_MEM_HOST);
}

// The same read-back for pair `pair` of the most recent svo_track_batch / svo_track_uploaded launch (ABI v6): what a
// caller needs to audit a batch against another implementation -- bench.py's self-check does.
extern "C" int svo_get_batch_tracks(svo_ctx *ctx, int pair, svo_pt2f *t1_left, svo_pt2f *t1_right, svo_pt2f *t2_right,
                                    svo_pt2f *t2_left, uint8_t *inlier, int cap, int *n_out)
{
    if (!ctx) return SVO_ERR_ARG;
    SVO_ARG(n_out && cap >= 0, "null output");
    SVO_TRY(read_back_ready(ctx, pair >= 0 && pair < ctx->last_batch_pairs, "pair is not part of the last batch launch"));
    int n;
    SVO_TRY(count_read(ctx, ctx->m_out + pair, &n));
    SVO_ARG(n >= 0 && n <= ctx->cfg.max_keypoints, "corrupt track count");
    SVO_ARG(n <= cap, "track capacity too small");
    *n_out = n;
    if (n == 0) return SVO_OK;
    return read_tracks(ctx, (size_t)pair * ctx->cfg.max_keypoints, n, t1_left, t1_right, t2_right, t2_left, inlier);
}

extern "C" int svo_streams_get_tracks(svo_ctx *ctx, int item, svo_pt2f *t1_left, svo_pt2f *t1_right, svo_pt2f *t2_right,
                                      svo_pt2f *t2_left, uint8_t *inlier, int cap, int *n_out)
{
    if (!ctx) return SVO_ERR_ARG;
    SVO_ARG(ctx->streams.n > 0, "no stream set (svo_streams_create)");
    // item i of a step is pair i of its launch set (an init item has no tracks: n = 0)
    return svo_get_batch_tracks(ctx, item, t1_left, t1_right, t2_right, t2_left, inlier, cap, n_out);
}

extern "C" int svo_get_last_tracks(svo_ctx *ctx, svo_pt2f *t1_left, svo_pt2f *t1_right, svo_pt2f *t2_right,
                                   svo_pt2f *t2_left, uint8_t *inlier, int cap, int *n_out)
{
    if (!ctx) return SVO_ERR_ARG;
    SVO_ARG(n_out && cap >= 0, "null output");
    SVO_HIP(hipSetDevice(ctx->device));
    if (svo_wait_results(ctx) != SVO_OK) return SVO_ERR_HIP;
    const int n = ctx->online_frames >= 2 ? ctx->online_tracked : 0;
    SVO_ARG(n <= cap, "track capacity too small");
    *n_out = n;
    if (n == 0) return SVO_OK;
    return read_tracks(ctx, 0, n, t1_left, t1_right, t2_right, t2_left, inlier);
}

// ---- FAST corner buckets: the strongest corners per grid cell (fast.hip: fast_bucket_kernel) -------------------------
static const int kMaxBucketCells = 16384;

static int64_t bucket_cell_count(int w, int h, int cw, int ch)
{
    return (int64_t)((w + cw - 1) / cw) * ((h + ch - 1) / ch);
}

extern "C" int svo_set_fast_buckets(svo_ctx *ctx, int cell_w, int cell_h, int per_cell)
{
    if (!ctx) return SVO_ERR_ARG;
    SVO_ARG(per_cell >= 0, "per_cell < 0");
    if (per_cell == 0) { ctx->bucket_keep = 0; return SVO_OK; }      // off: the sizes are ignored
    SVO_ARG(ctx->cfg.track_mode == SVO_MODE_LK, "FAST buckets are an LK-mode option (ORB mode spreads its keypoints with the quadtree)");
    SVO_ARG(ctx->lk_detector != SVO_DETECTOR_GFTT, "FAST buckets cannot be combined with the Shi-Tomasi detector (svo_set_lk_detector): it spaces its own corners");
    SVO_ARG(cell_w >= 1 && cell_h >= 1, "cell_w / cell_h < 1");
    const int64_t ncells = bucket_cell_count(ctx->cfg.width, ctx->cfg.height, cell_w, cell_h);
    SVO_ARG(ncells <= kMaxBucketCells, "more than 16384 cells per image");
    SVO_HIP(hipSetDevice(ctx->device));
    if (ncells > fast_bucket_lds_cells()) {
        // the per-cell words of such a grid live in device memory: every image slot of the context its own
        // (a call that cannot get them leaves the buckets as they were)
        if (dev_reserve(ctx, &ctx->bucket_cells, sizeof(int) * 4 * (size_t)ncells * (size_t)ctx->n_img) != SVO_OK) return SVO_ERR_HIP;
    }
    ctx->bucket_w = cell_w; ctx->bucket_h = cell_h; ctx->bucket_keep = per_cell;
    return SVO_OK;
}

extern "C" int svo_get_fast_buckets(const svo_ctx *ctx, int *cell_w, int *cell_h, int *per_cell)
{
    if (!ctx) return SVO_ERR_ARG;
    if (cell_w) *cell_w = ctx->bucket_keep > 0 ? ctx->bucket_w : 0;
    if (cell_h) *cell_h = ctx->bucket_keep > 0 ? ctx->bucket_h : 0;
    if (per_cell) *per_cell = ctx->bucket_keep;
    return SVO_OK;
}

extern "C" int svo_bucket_corners(svo_ctx *ctx, const svo_keypoint *in, int n, int width, int height, int cell_w, int cell_h,
                                  int per_cell, svo_keypoint *out, int cap, int *n_out, int mem)
{
    if (!ctx) return SVO_ERR_ARG;
    SVO_ARG(n >= 0 && n <= (1 << 24) && (in || n == 0) && (out || n == 0) && n_out, "null pointer / bad n");
    SVO_ARG(n <= cap, "n > cap");
    SVO_ARG(width >= 1 && height >= 1 && width <= 16384 && height <= 16384, "width / height out of range");
    SVO_ARG(cell_w >= 1 && cell_h >= 1 && per_cell >= 1, "cell_w / cell_h / per_cell < 1");
    SVO_ARG(mem == SVO_MEM_HOST || mem == SVO_MEM_DEVICE, "mem must be SVO_MEM_HOST or SVO_MEM_DEVICE");
    const int64_t ncells = bucket_cell_count(width, height, cell_w, cell_h);
    SVO_ARG(ncells <= kMaxBucketCells, "more than 16384 cells");
    SVO_HIP(hipSetDevice(ctx->device));
    const bool host = mem == SVO_MEM_HOST, dev_cells = ncells > fast_bucket_lds_cells();
    BlockCut cut;
    cut.add(256);                                           // the two counts
    const size_t o_xy = cut.add(sizeof(float2) * (size_t)n), o_resp = cut.add(sizeof(float) * (size_t)n),
                 o_cells = cut.add(dev_cells ? sizeof(int) * 4 * (size_t)ncells : 0),
                 o_in = cut.add(host ? sizeof(svo_keypoint) * (size_t)n : 0), o_out = cut.add(host ? sizeof(svo_keypoint) * (size_t)n : 0);
    if (dev_reserve(ctx, &ctx->bucket_stage, cut.total()) != SVO_OK) return SVO_ERR_HIP;
    uint8_t *s = ctx->bucket_stage.base;
    int *d_n = (int *)s, *d_nout = host ? (int *)s + 1 : n_out;
    float2 *xy = (float2 *)(s + o_xy);
    float *resp = (float *)(s + o_resp);
    const svo_keypoint *d_in;
    svo_keypoint *d_out = host ? (svo_keypoint *)(s + o_out) : out;
    SVO_TRY(to_device(ctx, in, (svo_keypoint *)(s + o_in), (size_t)n, mem, &d_in));
    launch_bucket_unpack(d_in, n, xy, resp, d_n, ctx->stream);
    BucketArgs k{};
    k.kp_xy = xy; k.kp_resp = resp; k.kp_stride = 0; k.n_out = d_n; k.cap = n;
    k.w = width; k.h = height; k.cw = cell_w; k.ch = cell_h; k.per_cell = per_cell;
    k.cols = (width + cell_w - 1) / cell_w; k.ncells = (int)ncells;
    k.cells = dev_cells ? (int *)(s + o_cells) : nullptr; k.cells_stride = 0;
    launch_fast_buckets(k, 1, ctx->stream);
    launch_bucket_pack(xy, resp, d_n, n, d_out, d_nout, ctx->stream);
    SVO_HIP(hipGetLastError());
    if (!host) return SVO_OK;
    SVO_TRY(count_read(ctx, d_nout, n_out));
    if (*n_out <= 0) return SVO_OK;
    SVO_TRY(from_device(ctx, out, (const svo_keypoint *)d_out, (size_t)*n_out, SVO_MEM_HOST));
    return io_done(ctx, SVO_MEM_HOST);
}

// ---- Shi-Tomasi corners: cv::goodFeaturesToTrack as the LK-mode detector and as stage calls (gftt.hip) ----------------
static int gftt_cell_of(double min_distance) { return min_distance >= 1.0 ? (int)nearbyint(min_distance) : 0; }   // cvRound: half to even

// Scratch for n images of w x h pixels with `cap` candidates each and a grid of ncells cells (+ `extra` bytes at the end,
// returned in *extra_at): reserved (a call that has to grow it waits for the device), cut up on every call.
// with_lists false: the per-image words only (svo_min_eigen_map writes its map where the caller says).
static int gftt_plan(svo_ctx *ctx, GfttBuf &g, int w, int h, int n, int cap, int64_t ncells, size_t extra, uint8_t **extra_at,
                     bool with_lists = true)
{
    int64_t ks = 64;
    while (ks < cap) ks <<= 1;
    const int mpitch = align_up(w, 64);
    const bool dev_cells = ncells > gftt_lds_cells();
    BlockCut cut;
    const size_t o_max = cut.add(sizeof(unsigned) * (size_t)n), o_cnt = cut.add(sizeof(int) * (size_t)n),
                 o_map = cut.add(with_lists ? sizeof(float) * (size_t)mpitch * h * n : 0),
                 o_keys = cut.add(with_lists ? sizeof(unsigned long long) * (size_t)ks * n : 0),
                 o_cells = cut.add(dev_cells ? sizeof(int) * 4 * (size_t)ncells * n : 0), o_extra = cut.add(extra);
    if (dev_reserve(ctx, &g, cut.total()) != SVO_OK) return SVO_ERR_HIP;
    g.maxkey = (unsigned *)(g.base + o_max); g.n_cand = (int *)(g.base + o_cnt);
    g.map = with_lists ? (float *)(g.base + o_map) : nullptr; g.mpitch = mpitch; g.map_stride = (int64_t)mpitch * h;
    g.keys = with_lists ? (unsigned long long *)(g.base + o_keys) : nullptr; g.keys_stride = ks;
    g.cells = dev_cells ? (int *)(g.base + o_cells) : nullptr; g.cells_stride = dev_cells ? 4 * ncells : 0;
    if (extra_at) *extra_at = g.base + o_extra;
    return SVO_OK;
}

// the detector's parameters into a launch block (the image, the scratch and the outputs are the caller's to fill)
static void gftt_params(GfttArgs &a, const GfttBuf &g, int w, int h, int cap, int max_corners, double quality, double min_distance)
{
    a.w = w; a.h = h; a.cap = cap;
    a.map = g.map; a.mpitch = g.mpitch; a.map_stride = g.map_stride; a.full = 0;
    a.maxkey = g.maxkey; a.n_cand = g.n_cand; a.keys = g.keys; a.keys_stride = g.keys_stride;
    a.quality = quality; a.min_dist2 = min_distance * min_distance; a.max_corners = max_corners;
    a.cell = gftt_cell_of(min_distance);
    a.gcols = a.cell > 0 ? (w + a.cell - 1) / a.cell : 0; a.grows = a.cell > 0 ? (h + a.cell - 1) / a.cell : 0;
    a.ncells = a.gcols * a.grows;
    a.cells = g.cells; a.cells_stride = g.cells_stride;
}

static int64_t gftt_cell_count(int w, int h, double min_distance)
{
    const int cell = gftt_cell_of(min_distance);
    return cell > 0 ? (int64_t)((w + cell - 1) / cell) * ((h + cell - 1) / cell) : 0;
}

namespace svo {
// pipeline.hip: the detector of the fused LK front end -- n_new left images -> kp_xy / kp_resp / kp_n of frame slots f0 ..
int gftt_detect_frames(svo_ctx *ctx, const uint8_t *L, int pitch, int64_t frame_stride, int f0, int n_new)
{
    GfttArgs a{};
    const int cap = ctx->cfg.max_keypoints;
    gftt_params(a, ctx->gftt_fused, ctx->cfg.width, ctx->cfg.height, cap, ctx->gftt_max_corners, ctx->gftt_quality, ctx->gftt_min_distance);
    a.img = L; a.pitch = pitch; a.img_stride = frame_stride;
    a.kp_xy = ctx->kp_xy + (size_t)f0 * cap; a.kp_resp = ctx->kp_resp + (size_t)f0 * cap; a.strength = nullptr; a.kp_stride = cap;
    a.n_out = ctx->kp_n + f0;
    // (stage marks of svo_get_timing: the detector stage is gftt_eigen + gftt_emit + the caller's `fast` mark, which ends the select)
    SVO_HIP(launch_gftt_eigen(a, n_new, ctx->stream));
    timing_mark(ctx, "gftt_eigen");
    SVO_HIP(launch_gftt_emit(a, n_new, ctx->stream));
    timing_mark(ctx, "gftt_emit");
    SVO_HIP(launch_gftt_select(a, n_new, ctx->stream));
    return SVO_OK;
}
}  // namespace svo

extern "C" int svo_set_lk_detector(svo_ctx *ctx, int detector, int max_corners, double quality_level, double min_distance)
{
    if (!ctx) return SVO_ERR_ARG;
    SVO_ARG(ctx->cfg.track_mode == SVO_MODE_LK, "the detector switch is an LK-mode option (ORB mode has its own extractor)");
    if (detector == SVO_DETECTOR_FAST) { ctx->lk_detector = SVO_DETECTOR_FAST; return SVO_OK; }      // the other arguments are ignored
    SVO_ARG(detector == SVO_DETECTOR_GFTT, "detector must be SVO_DETECTOR_FAST or SVO_DETECTOR_GFTT");
    SVO_ARG(std::isfinite(quality_level) && quality_level > 0.0, "quality_level must be finite and > 0");
    SVO_ARG(std::isfinite(min_distance) && min_distance >= 0.0, "min_distance must be finite and >= 0");
    const int64_t ncells = gftt_cell_count(ctx->cfg.width, ctx->cfg.height, min_distance);
    SVO_ARG(ncells <= kMaxBucketCells, "min_distance gives more than 16384 grid cells per image");
    SVO_ARG(ctx->bucket_keep == 0, "the Shi-Tomasi detector cannot be combined with the FAST buckets (svo_set_fast_buckets)");
    SVO_ARG(ctx->cfg.fast_keep_strongest == 0, "the Shi-Tomasi detector cannot be combined with svo_config.fast_keep_strongest");
    SVO_HIP(hipSetDevice(ctx->device));
    const int rc = gftt_plan(ctx, ctx->gftt_fused, ctx->cfg.width, ctx->cfg.height, ctx->n_img, ctx->cfg.max_keypoints, ncells, 0, nullptr);
    if (rc) return rc;                                   // (the scratch and the detector are what they were)
    ctx->lk_detector = SVO_DETECTOR_GFTT;
    ctx->gftt_max_corners = max_corners; ctx->gftt_quality = quality_level; ctx->gftt_min_distance = min_distance;
    return SVO_OK;
}

extern "C" int svo_get_lk_detector(const svo_ctx *ctx, int *detector, int *max_corners, double *quality_level, double *min_distance)
{
    if (!ctx) return SVO_ERR_ARG;
    const bool on = ctx->lk_detector == SVO_DETECTOR_GFTT;
    if (detector) *detector = ctx->lk_detector;
    if (max_corners) *max_corners = on ? ctx->gftt_max_corners : 0;
    if (quality_level) *quality_level = on ? ctx->gftt_quality : 0.0;
    if (min_distance) *min_distance = on ? ctx->gftt_min_distance : 0.0;
    return SVO_OK;
}

extern "C" int svo_min_eigen_map(svo_ctx *ctx, const uint8_t *img, int width, int height, int pitch, int mem, float *out, int out_pitch_floats)
{
    if (!ctx) return SVO_ERR_ARG;
    SVO_ARG(img && out, "null pointer");
    SVO_ARG(width >= 1 && height >= 1 && width <= 16384 && height <= 16384, "width / height out of range");
    SVO_ARG(pitch >= width && out_pitch_floats >= width, "pitch < width");
    SVO_ARG(mem == SVO_MEM_HOST || mem == SVO_MEM_DEVICE, "mem must be SVO_MEM_HOST or SVO_MEM_DEVICE");
    SVO_HIP(hipSetDevice(ctx->device));
    const bool host = mem == SVO_MEM_HOST;
    const int dpitch = align_up(width, 256);
    uint8_t *d_img = nullptr;
    GfttBuf &g = ctx->gftt_stage;
    // a device `out` is written in place: only the per-image words are needed then
    int rc = gftt_plan(ctx, g, width, height, 1, 64, 0, host ? (size_t)dpitch * height : 0, &d_img, /*with_lists*/ host);
    if (rc) return rc;
    GfttArgs a{};
    gftt_params(a, g, width, height, 64, 0, 1.0, 0.0);
    a.full = 1;
    if (host) {
        SVO_HIP(hipMemcpy2DAsync(d_img, (size_t)dpitch, img, (size_t)pitch, (size_t)width, (size_t)height, hipMemcpyHostToDevice, ctx->stream));
        a.img = d_img; a.pitch = dpitch;
    } else {
        a.img = img; a.pitch = pitch; a.map = out; a.mpitch = out_pitch_floats;
    }
    SVO_HIP(launch_gftt_eigen(a, 1, ctx->stream));
    SVO_HIP(hipGetLastError());
    if (!host) return SVO_OK;
    SVO_HIP(hipMemcpy2DAsync(out, sizeof(float) * (size_t)out_pitch_floats, g.map, sizeof(float) * (size_t)g.mpitch, sizeof(float) * (size_t)width,
                             (size_t)height, hipMemcpyDeviceToHost, ctx->stream));
    SVO_HIP(hipStreamSynchronize(ctx->stream));
    return SVO_OK;
}

extern "C" int svo_gftt_detect(svo_ctx *ctx, const uint8_t *img, int width, int height, int pitch, int mem, int max_corners,
                               double quality_level, double min_distance, svo_keypoint *out, float *strength, int cap, int *n_out)
{
    if (!ctx) return SVO_ERR_ARG;
    SVO_ARG(img && n_out && cap >= 0 && cap <= (1 << 24) && (out || cap == 0), "null pointer / bad cap");
    SVO_ARG(width >= 1 && height >= 1 && width <= 16384 && height <= 16384, "width / height out of range");
    SVO_ARG(pitch >= width, "pitch < width");
    SVO_ARG(mem == SVO_MEM_HOST || mem == SVO_MEM_DEVICE, "mem must be SVO_MEM_HOST or SVO_MEM_DEVICE");
    SVO_ARG(std::isfinite(quality_level) && quality_level > 0.0, "quality_level must be finite and > 0");
    SVO_ARG(std::isfinite(min_distance) && min_distance >= 0.0, "min_distance must be finite and >= 0");
    const int64_t ncells = gftt_cell_count(width, height, min_distance);
    SVO_ARG(ncells <= kMaxBucketCells, "min_distance gives more than 16384 grid cells");
    SVO_HIP(hipSetDevice(ctx->device));
    const bool host = mem == SVO_MEM_HOST;
    const int dpitch = align_up(width, 256);
    const size_t ncap = (size_t)(cap > 0 ? cap : 1);
    BlockCut cut;                                           // the stage call's own ranges, behind the detector's scratch
    const size_t o_n = cut.add(256), o_xy = cut.add(sizeof(float2) * ncap), o_resp = cut.add(sizeof(float) * ncap),
                 o_str = cut.add(sizeof(float) * ncap), o_rec = cut.add(host ? sizeof(svo_keypoint) * ncap : 0),
                 o_img = cut.add(host ? (size_t)dpitch * height : 0);
    uint8_t *x = nullptr;
    GfttBuf &g = ctx->gftt_stage;
    int rc = gftt_plan(ctx, g, width, height, 1, cap, ncells, cut.total(), &x);
    if (rc) return rc;
    GfttArgs a{};
    gftt_params(a, g, width, height, cap, max_corners, quality_level, min_distance);
    int *d_n = (int *)(x + o_n);
    float2 *xy = (float2 *)(x + o_xy);
    a.kp_xy = xy; a.kp_resp = (float *)(x + o_resp); a.kp_stride = 0; a.n_out = d_n;
    a.strength = host ? (float *)(x + o_str) : strength;
    svo_keypoint *d_rec = host ? (svo_keypoint *)(x + o_rec) : out;
    if (host) {
        uint8_t *d_img = x + o_img;
        SVO_HIP(hipMemcpy2DAsync(d_img, (size_t)dpitch, img, (size_t)pitch, (size_t)width, (size_t)height, hipMemcpyHostToDevice, ctx->stream));
        a.img = d_img; a.pitch = dpitch;
    } else {
        a.img = img; a.pitch = pitch;
    }
    SVO_HIP(launch_gftt_eigen(a, 1, ctx->stream));
    SVO_HIP(launch_gftt_emit(a, 1, ctx->stream));
    SVO_HIP(launch_gftt_select(a, 1, ctx->stream));
    launch_gftt_pack(xy, d_n, cap, d_rec, host ? nullptr : n_out, ctx->stream);
    SVO_HIP(hipGetLastError());
    if (!host) return SVO_OK;
    SVO_TRY(count_read(ctx, d_n, n_out));
    const int m = *n_out;
    SVO_ARG(m <= cap, "more candidates than cap");
    if (m <= 0) return SVO_OK;
    SVO_TRY(from_device(ctx, out, (const svo_keypoint *)d_rec, (size_t)m, SVO_MEM_HOST));
    SVO_TRY(from_device(ctx, strength, (const float *)a.strength, (size_t)m, SVO_MEM_HOST));
    return io_done(ctx, SVO_MEM_HOST);
}

// ---- robust two-view pose refinement after solvePnPRansac (refine.hip: pose_refine_kernel) ----------------------------
static int set_pose_refine(svo_ctx *ctx, int mode, int rounds, int iters, double sigma_px, int min_inliers)
{
    SVO_TRY(check_optimiser_params(ctx, rounds, iters, sigma_px));
    SVO_ARG(min_inliers >= 1, "min_inliers < 1");
    if (mode != SVO_REFINE_OFF) { const int rc = mode == SVO_REFINE_BA ? ba_alloc(ctx) : refine_alloc(ctx); if (rc) return rc; }
    ctx->refine_mode = mode; ctx->refine_rounds = rounds; ctx->refine_iters = iters;
    ctx->refine_sigma = sigma_px; ctx->refine_min_inliers = min_inliers;
    return SVO_OK;
}

extern "C" int svo_set_pose_refine(svo_ctx *ctx, int mode, int rounds, int iters, double sigma_px, int min_inliers)
{
    if (!ctx) return SVO_ERR_ARG;
    SVO_ARG(mode == SVO_REFINE_OFF || mode == SVO_REFINE_REPROJ, "mode must be SVO_REFINE_OFF or SVO_REFINE_REPROJ");
    return set_pose_refine(ctx, mode, rounds, iters, sigma_px, min_inliers);
}

// the stage's third mode has a setter of its own: svo_set_pose_refine goes on refusing every mode but OFF and REPROJ, as its
// callers were told it does
extern "C" int svo_set_pose_refine_ba(svo_ctx *ctx, int rounds, int iters, double sigma_px, int min_inliers)
{
    if (!ctx) return SVO_ERR_ARG;
    return set_pose_refine(ctx, SVO_REFINE_BA, rounds, iters, sigma_px, min_inliers);
}

extern "C" int svo_get_pose_refine(const svo_ctx *ctx, int *mode, int *rounds, int *iters, double *sigma_px, int *min_inliers)
{
    if (!ctx) return SVO_ERR_ARG;
    if (mode) *mode = ctx->refine_mode;
    if (rounds) *rounds = ctx->refine_rounds;
    if (iters) *iters = ctx->refine_iters;
    if (sigma_px) *sigma_px = ctx->refine_sigma;
    if (min_inliers) *min_inliers = ctx->refine_min_inliers;
    return SVO_OK;
}

extern "C" int svo_refine_pose(svo_ctx *ctx, const svo_pt3f *obj, const svo_pt2f *img_left, const svo_pt2f *img_right, int n,
                               const double P1[12], const double P2[12], const double rvec0[3], const double tvec0[3],
                               svo_refine_result *res, uint8_t *active, int mem)
{
    if (!ctx) return SVO_ERR_ARG;
    return stage_refine_pose(ctx, obj, img_left, img_right, n, P1, P2, rvec0, tvec0, res, active, mem);
}

extern "C" int svo_get_refine_result(svo_ctx *ctx, int pair, svo_refine_result *res, uint8_t *active, int cap, int *n_out)
{
    if (!ctx) return SVO_ERR_ARG;
    SVO_TRY(read_back_ready(ctx, ctx->last.refine_mode != SVO_REFINE_OFF && ctx->refine_buf, "the refinement stage was off for the last launch (svo_set_pose_refine)"));
    SVO_ARG(pair >= 0 && pair < ctx->last.pairs, "pair is not part of the last launch");
    SVO_ARG(active == nullptr || cap >= 0, "negative capacity");
    return refine_read_result(ctx, pair, res, active, cap, n_out);
}

// ---- the stage's bundle-adjustment mode (ba.hip: pose_ba_kernel) -------------------------------------------------------
extern "C" int svo_refine_ba(svo_ctx *ctx, const svo_pt3f *obj, const svo_pt2f *img1_left, const svo_pt2f *img1_right,
                             const svo_pt2f *img2_left, const svo_pt2f *img2_right, int n, const double P1[12], const double P2[12],
                             const double rvec0[3], const double tvec0[3], svo_refine_result *res, uint8_t *active, double *X_out,
                             int mem)
{
    if (!ctx) return SVO_ERR_ARG;
    return stage_refine_ba(ctx, obj, img1_left, img1_right, img2_left, img2_right, n, P1, P2, rvec0, tvec0, res, active, X_out, mem);
}

extern "C" int svo_get_refine_points(svo_ctx *ctx, int pair, double *X, int cap, int *n_out)
{
    if (!ctx) return SVO_ERR_ARG;
    SVO_TRY(read_back_ready(ctx, ctx->last.refine_mode == SVO_REFINE_BA && ctx->ba_buf, "the last launch did not run in SVO_REFINE_BA mode (svo_set_pose_refine_ba)"));
    SVO_ARG(pair >= 0 && pair < ctx->last.pairs, "pair is not part of the last launch");
    SVO_ARG(X == nullptr || cap >= 0, "negative capacity");
    return ba_read_points(ctx, pair, X, cap, n_out);
}

// ---- track carry: LK tracks kept across frames under persistent ids (carry.hip: carry_merge_kernel) ------------------------
static bool carry_params_ok(double min_distance, int max_age)
{
    return std::isfinite(min_distance) && min_distance >= 1.0 && min_distance <= 256.0 && max_age >= 0;
}

extern "C" int svo_set_track_carry(svo_ctx *ctx, int on, double min_distance, int max_age)
{
    if (!ctx) return SVO_ERR_ARG;
    if (!on && ctx->win.frames > 0) { ctx->err = "the sliding window is on and needs track carry (svo_set_window_ba(ctx, 0, ...) first)"; return SVO_ERR_STATE; }
    if (!on && ctx->kf.on) { ctx->err = "keyframe mode is on and needs track carry (svo_set_keyframe(ctx, 0, ...) first)"; return SVO_ERR_STATE; }
    if (!on) { ctx->carry.on = false; return SVO_OK; }               // off: the other arguments are ignored
    SVO_ARG(ctx->cfg.track_mode == SVO_MODE_LK, "track carry is an LK-mode option (ORB mode matches descriptors frame to frame)");
    SVO_ARG(carry_params_ok(min_distance, max_age), "min_distance must be finite and in [1, 256], max_age >= 0");
    SVO_HIP(hipSetDevice(ctx->device));
    SVO_TRY(carry_alloc(ctx));                                       // first enabling call: the working frames' and an existing stream set's share
    ctx->carry.on = true; ctx->carry.min_distance = min_distance; ctx->carry.max_age = max_age;
    chain_event(ctx, kChainCarrySet);
    return SVO_OK;
}

extern "C" int svo_get_track_carry(const svo_ctx *ctx, int *on, double *min_distance, int *max_age)
{
    if (!ctx) return SVO_ERR_ARG;
    if (on) *on = ctx->carry.on ? 1 : 0;
    if (min_distance) *min_distance = ctx->carry.on ? ctx->carry.min_distance : 0.0;
    if (max_age) *max_age = ctx->carry.on ? ctx->carry.max_age : 0;
    return SVO_OK;
}

extern "C" int svo_carry_merge(svo_ctx *ctx, int width, int height, double min_distance, int max_age, const svo_pt2f *trk_xy,
                               const float *trk_resp, const int64_t *trk_id, const int32_t *trk_age, const uint8_t *trk_keep, int n_trk,
                               const svo_pt2f *det_xy, const float *det_resp, int n_det, int64_t next_id, svo_pt2f *out_xy,
                               float *out_resp, int64_t *out_id, int32_t *out_age, int32_t *out_src, int cap, int *n_out, int *n_carried,
                               int mem)
{
    if (!ctx) return SVO_ERR_ARG;
    SVO_ARG(width >= 1 && height >= 1 && width <= 16384 && height <= 16384, "width / height out of range");
    SVO_ARG(carry_params_ok(min_distance, max_age), "min_distance must be finite and in [1, 256], max_age >= 0");
    SVO_ARG(n_trk >= 0 && n_det >= 0 && n_trk <= (1 << 20) && n_det <= (1 << 20), "bad n_trk / n_det");
    SVO_ARG(n_trk == 0 || (trk_xy && trk_resp && trk_id && trk_age && trk_keep), "null track list");
    SVO_ARG(n_det == 0 || (det_xy && det_resp), "null detection list");
    SVO_ARG(cap >= n_trk && cap <= (1 << 21), "cap < n_trk: only detections may fall off the list");
    SVO_ARG(n_out && n_carried && (cap == 0 || (out_xy && out_resp && out_id && out_age && out_src)), "null output");
    SVO_ARG(mem == SVO_MEM_HOST || mem == SVO_MEM_DEVICE, "mem must be SVO_MEM_HOST or SVO_MEM_DEVICE");
    SVO_HIP(hipSetDevice(ctx->device));
    const bool host = mem == SVO_MEM_HOST;
    const size_t nt = (size_t)n_trk, nd = (size_t)n_det, nc = (size_t)cap, ns = std::max(std::max(nt, nd), (size_t)1);
    BlockCut cut;
    const size_t o_cnt = cut.add(256), o_sorted = cut.add(sizeof(int) * ns), o_flag = cut.add(ns), o_dflag = cut.add(ns),
                 o_sxy = cut.add(sizeof(float2) * ns), o_sresp = cut.add(sizeof(float) * ns);
    const size_t i_xy = cut.add(host ? sizeof(float2) * nt : 0), i_resp = cut.add(host ? sizeof(float) * nt : 0),
                 i_id = cut.add(host ? sizeof(long long) * nt : 0), i_age = cut.add(host ? sizeof(int) * nt : 0), i_keep = cut.add(host ? nt : 0),
                 i_dxy = cut.add(host ? sizeof(float2) * nd : 0), i_dresp = cut.add(host ? sizeof(float) * nd : 0);
    const size_t r_xy = cut.add(host ? sizeof(float2) * nc : 0), r_resp = cut.add(host ? sizeof(float) * nc : 0),
                 r_id = cut.add(host ? sizeof(long long) * nc : 0), r_age = cut.add(host ? sizeof(int) * nc : 0), r_src = cut.add(host ? sizeof(int) * nc : 0);
    if (dev_reserve(ctx, &ctx->carry.stage, cut.total()) != SVO_OK) return SVO_ERR_HIP;
    uint8_t *s = ctx->carry.stage.base;
    CarryMergeArgs a{};
    a.w = width; a.h = height;
    carry_grid(width, height, min_distance, &a.cell, &a.cols, &a.rows);
    a.min_d2 = min_distance * min_distance; a.max_age = max_age;
    a.cap = (int)ns; a.out_cap = cap;
    a.n_trk = n_trk; a.n_det = n_det; a.next0 = (long long)next_id;
    SVO_TRY(to_device(ctx, (const float2 *)trk_xy, (float2 *)(s + i_xy), nt, mem, &a.q));
    SVO_TRY(to_device(ctx, trk_resp, (float *)(s + i_resp), nt, mem, &a.p_resp));
    SVO_TRY(to_device(ctx, (const long long *)trk_id, (long long *)(s + i_id), nt, mem, &a.p_id));
    SVO_TRY(to_device(ctx, (const int *)trk_age, (int *)(s + i_age), nt, mem, &a.p_age));
    SVO_TRY(to_device(ctx, trk_keep, s + i_keep, nt, mem, &a.keep));
    SVO_TRY(to_device(ctx, (const float2 *)det_xy, (float2 *)(s + i_dxy), nd, mem, &a.d_xy));
    SVO_TRY(to_device(ctx, det_resp, (float *)(s + i_dresp), nd, mem, &a.d_resp));
    a.o_xy = host ? (float2 *)(s + r_xy) : (float2 *)out_xy; a.o_resp = host ? (float *)(s + r_resp) : out_resp;
    a.o_id = host ? (long long *)(s + r_id) : (long long *)out_id; a.o_age = host ? (int *)(s + r_age) : (int *)out_age;
    a.o_src = host ? (int *)(s + r_src) : (int *)out_src;
    a.o_n = host ? (int *)(s + o_cnt) : n_out; a.o_carried = host ? (int *)(s + o_cnt) + 1 : n_carried;
    a.sorted = (int *)(s + o_sorted); a.flag = s + o_flag; a.dflag = s + o_dflag; a.s_dxy = (float2 *)(s + o_sxy); a.s_dresp = (float *)(s + o_sresp);
    launch_carry_merge(a, 1, ctx->stream);
    SVO_HIP(hipGetLastError());
    if (!host) return SVO_OK;
    const int *h;
    SVO_TRY(count_fetch(ctx, 0, a.o_n, 2));
    SVO_TRY(counts_wait(ctx, &h));
    *n_out = h[0]; *n_carried = h[1];
    const size_t n = (size_t)h[0];
    SVO_TRY(from_device(ctx, (float2 *)out_xy, (const float2 *)a.o_xy, n, mem));
    SVO_TRY(from_device(ctx, out_resp, (const float *)a.o_resp, n, mem));
    SVO_TRY(from_device(ctx, (long long *)out_id, (const long long *)a.o_id, n, mem));
    SVO_TRY(from_device(ctx, (int *)out_age, (const int *)a.o_age, n, mem));
    SVO_TRY(from_device(ctx, (int *)out_src, (const int *)a.o_src, n, mem));
    return io_done(ctx, mem);
}

// ---- sliding window: the landmark table's update on a caller's tables (window.hip: window_update_kernel) --------------------
extern "C" int svo_window_update(svo_ctx *ctx, int frames, const svo_window_table *in, const svo_window_table *out, int cap,
                                 const svo_pt2f *t1_left, const svo_pt2f *t1_right, const svo_pt2f *t2_left, const svo_pt2f *t2_right,
                                 const int64_t *ids, const svo_pt3f *tri, int n_trk, const double pose_a[16], const double pose_b[16], int mem)
{
    if (!ctx) return SVO_ERR_ARG;
    return stage_window_update(ctx, frames, in, out, cap, t1_left, t1_right, t2_left, t2_right, ids, tri, n_trk, pose_a, pose_b, mem);
}

extern "C" int svo_set_window_ba(svo_ctx *ctx, int frames, int rounds, int iters, double sigma_px, int min_obs)
{
    if (!ctx) return SVO_ERR_ARG;
    if (frames == 0) { ctx->win.frames = 0; chain_event(ctx, kChainWindowSet); return SVO_OK; }      // off: the other arguments are ignored
    SVO_ARG(frames >= 2 && frames <= SVO_WINDOW_MAX_FRAMES, "frames must be 0 or 2..SVO_WINDOW_MAX_FRAMES");
    SVO_TRY(check_optimiser_params(ctx, rounds, iters, sigma_px));
    SVO_ARG(min_obs >= 1, "min_obs < 1");
    SVO_TRY(follower_may_start(ctx, "the sliding window", ctx->kf.on, "keyframe mode", "svo_set_keyframe(ctx, 0, ...)"));
    SVO_TRY(window_alloc(ctx, frames));
    ctx->win.frames = frames; ctx->win.rounds = rounds; ctx->win.iters = iters; ctx->win.sigma = sigma_px; ctx->win.min_obs = min_obs;
    chain_event(ctx, kChainWindowSet);
    return SVO_OK;
}

extern "C" int svo_get_window_ba(const svo_ctx *ctx, int *frames, int *rounds, int *iters, double *sigma_px, int *min_obs)
{
    if (!ctx) return SVO_ERR_ARG;
    const bool on = ctx->win.frames > 0;
    if (frames) *frames = ctx->win.frames;
    if (rounds) *rounds = on ? ctx->win.rounds : 0;
    if (iters) *iters = on ? ctx->win.iters : 0;
    if (sigma_px) *sigma_px = on ? ctx->win.sigma : 0.0;
    if (min_obs) *min_obs = on ? ctx->win.min_obs : 0;
    return SVO_OK;
}

extern "C" int svo_get_window(svo_ctx *ctx, const svo_window_table *out, int cap)
{
    if (!ctx) return SVO_ERR_ARG;
    SVO_ARG(out && out->counts && cap >= 0, "null table / counts");
    SVO_TRY(read_back_ready(ctx, ctx->last.window_frames > 0 && ctx->win.block.base, "the sliding window was off for the last svo_add_frame step (svo_set_window_ba)"));
    return window_read(ctx, out, cap);
}

extern "C" int svo_get_window_result(svo_ctx *ctx, svo_window_result *res)
{
    if (!ctx) return SVO_ERR_ARG;
    SVO_ARG(res, "null result");
    SVO_TRY(read_back_ready(ctx, ctx->last.window_frames > 0 && ctx->win.block.base, "the sliding window was off for the last svo_add_frame step (svo_set_window_ba)"));
    return window_read_result(ctx, res);
}

extern "C" int svo_window_ba(svo_ctx *ctx, const svo_window_table *table, int cap, const double P1[12], const double P2[12], int rounds,
                             int iters, double sigma_px, int min_obs, svo_window_result *res, int mem)
{
    if (!ctx) return SVO_ERR_ARG;
    return stage_window_ba(ctx, table, cap, P1, P2, rounds, iters, sigma_px, min_obs, res, mem);
}

// ---- keyframe-relative pose on the online chain (keyframe.hip: keyframe_join_kernel, keyframe_update_kernel) -----------------
extern "C" int svo_set_keyframe(svo_ctx *ctx, int on, int min_tracks, int max_gap)
{
    if (!ctx) return SVO_ERR_ARG;
    if (!on) { ctx->kf.on = false; chain_event(ctx, kChainKeyframeSet); return SVO_OK; }      // off: the other arguments are ignored
    SVO_ARG(min_tracks >= 4 && min_tracks <= ctx->cfg.max_keypoints, "min_tracks outside 4..max_keypoints");
    SVO_ARG(max_gap >= 0 && max_gap != 1, "max_gap must be 0 (no limit) or >= 2: the smallest gap of a solve is 2");
    SVO_ARG(ctx->cfg.max_batch >= 2, "keyframe mode solves on item 1 of the pose workspace: max_batch must be >= 2");
    SVO_TRY(follower_may_start(ctx, "keyframe mode", ctx->win.frames > 0, "the sliding window", "svo_set_window_ba(ctx, 0, ...)"));
    SVO_TRY(keyframe_alloc(ctx));
    ctx->kf.on = true; ctx->kf.min_tracks = min_tracks; ctx->kf.max_gap = max_gap;
    chain_event(ctx, kChainKeyframeSet);
    return SVO_OK;
}

extern "C" int svo_get_keyframe(const svo_ctx *ctx, int *on, int *min_tracks, int *max_gap)
{
    if (!ctx) return SVO_ERR_ARG;
    if (on) *on = ctx->kf.on ? 1 : 0;
    if (min_tracks) *min_tracks = ctx->kf.on ? ctx->kf.min_tracks : 0;
    if (max_gap) *max_gap = ctx->kf.on ? ctx->kf.max_gap : 0;
    return SVO_OK;
}

static int keyframe_last_step(svo_ctx *ctx)
{
    return read_back_ready(ctx, ctx->online_frames >= 2 && ctx->last.keyframe && ctx->kf.buf,
                           "keyframe mode was off for the last svo_add_frame step, or no pair has been tracked (svo_set_keyframe)");
}

extern "C" int svo_get_keyframe_result(svo_ctx *ctx, svo_keyframe_result *res)
{
    if (!ctx) return SVO_ERR_ARG;
    SVO_ARG(res, "null result");
    SVO_TRY(keyframe_last_step(ctx));
    return keyframe_read_result(ctx, res);
}

extern "C" int svo_get_keyframe_matches(svo_ctx *ctx, int64_t *ids, svo_pt3f *X, svo_pt2f *xy, int32_t *trk_index, uint8_t *mask, int cap,
                                        int *n_out)
{
    if (!ctx) return SVO_ERR_ARG;
    SVO_ARG(n_out && cap >= 0, "null output");
    SVO_TRY(keyframe_last_step(ctx));
    return keyframe_read_matches(ctx, ids, X, xy, trk_index, mask, cap, n_out);
}

extern "C" int svo_get_keyframe_table(svo_ctx *ctx, int64_t *ids, svo_pt3f *X, int cap, int *n_out)
{
    if (!ctx) return SVO_ERR_ARG;
    SVO_ARG(n_out && cap >= 0, "null output");
    SVO_TRY(keyframe_last_step(ctx));
    return keyframe_read_table(ctx, ids, X, cap, n_out);
}

extern "C" int svo_keyframe_join(svo_ctx *ctx, const int64_t *tab_ids, const svo_pt3f *tab_X, int n_rows, const int64_t *trk_ids,
                                 const svo_pt2f *trk_xy, int n_trk, svo_pt3f *out_X, svo_pt2f *out_xy, int32_t *out_trk,
                                 int32_t *out_row, int cap, int *n_out, int mem)
{
    if (!ctx) return SVO_ERR_ARG;
    return stage_keyframe_join(ctx, tab_ids, tab_X, n_rows, trk_ids, trk_xy, n_trk, out_X, out_xy, out_trk, out_row, cap, n_out, mem);
}

// n ids and ages at `offset` of two device lists -> the caller's.  Capacity rule of the read-backs below: ids / ages null asks
// for the count only; otherwise the count must fit `cap`.
static int read_ids(svo_ctx *ctx, const long long *d_id, const int *d_age, size_t offset, int n, int64_t *ids, int32_t *ages, int cap, int *n_out)
{
    *n_out = n;
    if (!ids && !ages) return SVO_OK;
    SVO_ARG(n <= cap, "id capacity too small");
    SVO_TRY(from_device(ctx, (long long *)ids, d_id + offset, (size_t)n, SVO_MEM_HOST));
    SVO_TRY(from_device(ctx, (int *)ages, d_age + offset, (size_t)n, SVO_MEM_HOST));
    return io_done(ctx, SVO_MEM_HOST);
}

extern "C" int svo_get_frame_track_ids(svo_ctx *ctx, int64_t *ids, int32_t *ages, int cap, int *n_out)
{
    if (!ctx) return SVO_ERR_ARG;
    SVO_ARG(n_out && cap >= 0, "null output");
    SVO_ARG(ctx->online_frames > 0, "no frame has been added");
    const int cur = ctx->online_cur;
    SVO_TRY(read_back_ready(ctx, ctx->carry.ids[cur] && ctx->carry.buf, "track carry was off when the last frame was added (svo_set_track_carry)"));
    int n = 0;
    SVO_TRY(count_read(ctx, ctx->kp_n + cur, &n));
    const size_t kcap = (size_t)ctx->cfg.max_keypoints;
    n = n < (int)kcap ? n : (int)kcap;
    return read_ids(ctx, ctx->carry.kp_id, ctx->carry.kp_age, (size_t)cur * kcap, n, ids, ages, cap, n_out);
}

// ids / ages-at-t1 of the tracks of pair `pair` of the last fused launch, in the order of svo_get_batch_tracks' lists
static int pair_track_ids(svo_ctx *ctx, int pair, int64_t *ids, int32_t *ages, int cap, int *n_out)
{
    SVO_ARG(n_out && cap >= 0, "null output");
    SVO_TRY(read_back_ready(ctx, ctx->last.carry && ctx->carry.buf, "track carry was off for the last step (svo_set_track_carry)"));
    SVO_ARG(pair >= 0 && pair < ctx->last.pairs, "item is not part of the last step");
    int n;
    SVO_TRY(count_read(ctx, ctx->m_out + pair, &n));
    SVO_ARG(n >= 0 && n <= ctx->cfg.max_keypoints, "corrupt track count");
    return read_ids(ctx, ctx->carry.trk_id, ctx->carry.trk_age, (size_t)pair * ctx->cfg.max_keypoints, n, ids, ages, cap, n_out);
}

extern "C" int svo_get_last_track_ids(svo_ctx *ctx, int64_t *ids, int32_t *ages, int cap, int *n_out)
{
    if (!ctx) return SVO_ERR_ARG;
    SVO_ARG(ctx->online_frames >= 2, "no pair has been tracked by svo_add_frame");
    return pair_track_ids(ctx, 0, ids, ages, cap, n_out);
}

extern "C" int svo_streams_get_track_ids(svo_ctx *ctx, int item, int64_t *ids, int32_t *ages, int cap, int *n_out)
{
    if (!ctx) return SVO_ERR_ARG;
    SVO_ARG(ctx->streams.n > 0, "no stream set (svo_streams_create)");
    return pair_track_ids(ctx, item, ids, ages, cap, n_out);
}

extern "C" int svo_streams_get_frame_tracks(svo_ctx *ctx, int stream_id, svo_keypoint *kps, int64_t *ids, int32_t *ages, int cap, int *n_out)
{
    if (!ctx) return SVO_ERR_ARG;
    StreamSet &ss = ctx->streams;
    SVO_ARG(ss.n > 0, "no stream set (svo_streams_create)");
    SVO_ARG(stream_id >= 0 && stream_id < ss.n, "stream id out of range");
    SVO_ARG(n_out && cap >= 0, "null output");
    SVO_TRY(read_back_ready(ctx, ss.n_frames[(size_t)stream_id] > 0 && ss.has_ids[(size_t)stream_id] && ss.seg[4] && ss.seg[5],
                            "the stream has no stored list with ids (no frame yet, or track carry was off for its last step)"));
    const size_t kcap = (size_t)ctx->cfg.max_keypoints, sid = (size_t)stream_id;
    int n = 0;
    SVO_TRY(count_read(ctx, (const int *)ss.seg[3] + sid, &n));
    n = n < (int)kcap ? n : (int)kcap;
    *n_out = n;
    if (!kps && !ids && !ages) return SVO_OK;
    SVO_ARG(n <= cap, "capacity too small");
    if (kps && n > 0) {
        std::vector<float2> xy((size_t)n);
        std::vector<float> resp((size_t)n);
        SVO_TRY(from_device(ctx, xy.data(), (const float2 *)ss.seg[1] + sid * kcap, (size_t)n, SVO_MEM_HOST));
        SVO_TRY(from_device(ctx, resp.data(), (const float *)ss.seg[2] + sid * kcap, (size_t)n, SVO_MEM_HOST));
        SVO_TRY(io_done(ctx, SVO_MEM_HOST));
        format_keypoints(xy.data(), resp.data(), n, kps);
    }
    return read_ids(ctx, (const long long *)ss.seg[4], (const int *)ss.seg[5], sid * kcap, n, ids, ages, cap, n_out);
}
