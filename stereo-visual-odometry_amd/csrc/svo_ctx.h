// svo_ctx.h -- the context object behind the C-ABI (internal).
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include <functional>
#include <string>
#include <utility>
#include <vector>
#include "../../include/svo_abi.h"
#include "block_cut.h"
#include "chain_stages.h"
#include "pinned_layout.h"
#include "svo_kernels.h"

// What a context owns on the device, all of it released by free_all() (svo_abi.hip) and by nothing else.  Device memory has
// three lifetimes, and one function each:
//   - planned in svo_create: dev_alloc while `planning` only records (where the pointer goes, size); dev_commit makes ONE
//     hipMalloc of the sum (~30 separate allocations were a fifth of a short run's start-up), hands the pointers out and
//     runs the initialisations that were waiting for them (dev_defer);
//   - made on first use at a fixed size (ORB buffers of an LK context, frame buffers of an online-sized context, stream
//     stores, resize tables, matcher and refinement blocks): dev_alloc after the commit, an allocation of its own,
//     remembered in `extra`;
//   - made on first use and growable (the scratch of stage calls, staging of host frames, per-cell words): dev_reserve on a
//     DevScratch, remembered in `scratch` from its first allocation on.
// Events and streams are made by dev_event / dev_stream, in svo_create or on first use, and remembered in `events` / `streams`.
struct DevArena {
    char *base = nullptr;
    size_t planned = 0;
    bool planning = false;
    std::vector<std::pair<void **, size_t>> plan;
    std::vector<std::function<int()>> after;
    std::vector<void *> extra;
    std::vector<DevScratch *> scratch;
    std::vector<hipEvent_t> events;
    std::vector<hipStream_t> streams;      // in the order they were made: the context's own stream first
};

// A stream set (svo_streams_create): n independent live stereo streams of one context.  What a stream keeps in HBM between
// steps is the segments stream_segments() lists (pipeline.hip; carry_last_frame moves the same list) -- seg[k] + id * seg_bytes[k],
// k < n_seg -- and its frame_pose_ (pose + 16 * id); the INITING / TRACKING state is host-side (steps are issued in host order).
constexpr int kMaxSeg = 6;               // segments a frame carries at most (LK mode with track carry: the ids and the ages)
struct StreamSet {
    int n = 0;
    int n_seg = 0;
    uint8_t *seg[kMaxSeg] = {};
    size_t seg_bytes[kMaxSeg] = {};
    double *pose = nullptr;
    // track carry (svo_set_track_carry): the id counter of every stream, on the device; which streams' stored lists have ids, and
    // which start their ids over with the next step (a new or a reset stream)
    long long *next_id = nullptr;
    std::vector<uint8_t> has_ids, restart;
    std::vector<int> n_frames;        // frames fed since the stream's reset (0: INITING)
    std::vector<int> seen;            // call number a stream id was last named in (duplicate check)
    int call = 0;
};

// The launch shape of the table-driven resize kernel (resize.hip), derived from one geometry's tap tables: resize_shape.
struct ResizeShape {
    int bx_shift = 8, rpt = 8;        // workgroup = 2^bx_shift lanes along x (4 pixels each) x 256 >> bx_shift lane rows x rpt rows per lane
    int lds_pitch = 0, lds_rows = 0;  // staged source rows: bytes per row (multiple of 16), rows; 0 rows: gathered from global memory
};

// One cv::resize geometry (resize.hip): the tap tables of (source size, destination size, interpolation, factors), built on
// the host in double exactly as include/svo_abi.h states them and uploaded once, and the launch shape derived from them.
struct ResizeTab {
    int sw = 0, sh = 0, dw = 0, dh = 0, interp = 0;
    double fx = 0, fy = 0;            // the key: factor form (fx, fy > 0) or size form (0, 0)
    double inv_x = 1, inv_y = 1;
    bool box = false;                 // INTER_LINEAR at exactly 2x: the 2x2 mean, no tables
    void *xt = nullptr, *yt = nullptr;   // int2 per destination column (sx | sx1 << 16, a0 | a1 << 16), int4 per row (y0, y1, b0, b1)
    ResizeShape shape;
};

// The ingest stage of a context (svo_ingest_create): source-size frames -> the context's width x height.
struct Ingest {
    bool on = false;
    int sw = 0, sh = 0, tab = -1;
    int spitch = 0;                   // row pitch of the source-size staging (16-byte aligned)
    uint8_t *work = nullptr;          // working-size frames: 2 eyes x (max_batch + 1) slots, stage_pitch rows
    DevScratch src_stage;             // source-size staging of HOST frames (svo_ingest_add_frame / _streams_step): 2 eyes x the call's frames
    uint8_t *up_stage[2] = {nullptr, nullptr};   // source-size staging behind fb[0] / fb[1] (svo_ingest_upload_frames_at), first use
};

// Scratch of the Shi-Tomasi detector (gftt.hip) for n images of w x h pixels: ONE growable block cut into the candidate
// map, the per-image words, the candidate keys, the cell words of a grid too large for LDS and (stage calls) the staged image
// and the output lists.
struct GfttBuf : DevScratch {
    float *map = nullptr; int mpitch = 0; int64_t map_stride = 0;
    unsigned *maxkey = nullptr; int *n_cand = nullptr;
    unsigned long long *keys = nullptr; int64_t keys_stride = 0;
    int *cells = nullptr; int64_t cells_stride = 0;
};

struct svo_ctx {
    svo_config cfg;
    DevArena arena;
    int device = 0;
    hipStream_t own_stream = nullptr, stream = nullptr;
    std::string err;
    svo::PyrGeom geom;

    int n_img = 0;                    // images the batch buffers are sized for (max_batch + 1)
    // ---- stage-API resources
    uint8_t *slots = nullptr;         // num_slots pyramid slots
    std::vector<char> slot_built;
    uint8_t *stage_img = nullptr;     // device staging for host images (2 images, aligned pitch)
    int stage_pitch = 0;
    uint8_t *h_stage = nullptr;       // pinned mirror of stage_img: rows gathered on the host, one H2D copy per image
    hipEvent_t ev_stage[2] = {nullptr, nullptr};
    bool h_stage_busy[2] = {false, false};
    // ---- FAST scratch (corner records and their counts, fast_scratch.h) + outputs, n_img images
    uint8_t *score = nullptr; int spitch = 0; int64_t score_stride = 0;
    int *rowcount = nullptr; int64_t rowcount_stride = 0;
    float2 *kp_xy = nullptr; float *kp_resp = nullptr; int *kp_n = nullptr;
    // ---- LK buffers, max_batch items x max_keypoints
    float2 *pts_in = nullptr;
    float2 *pts_out[4] = {nullptr, nullptr, nullptr, nullptr};
    uint8_t *status[4] = {nullptr, nullptr, nullptr, nullptr};
    uint8_t *keep = nullptr;
    float2 *cmp[4] = {nullptr, nullptr, nullptr, nullptr};    // compacted t1l, t1r, t2r, t2l
    int *m_out = nullptr;
    // ---- pose stage buffers (geometry.hip solves into them; pose_chain.hip, refine.hip and ba.hip work on its records)
    float *X3 = nullptr;              // triangulated points, 3 floats per point
    void *pnp_ws = nullptr; size_t pnp_ws_bytes = 0;
    svo_step_result *d_results = nullptr;
    DevScratch chain_stage;           // svo_chain_relative: the caller's motions and flags and the poses (HOST calls)
    // ---- batch-mode pyramid slots: 2 * n_img
    uint8_t *bslots = nullptr;
    // ---- online state (svo_add_frame)
    int online_frames = 0;            // frames fed since reset
    int online_cur = 0;               // which half of the 2-frame ring holds the latest frame
    int last_batch_pairs = 0;         // pairs of the most recent batch launch (svo_get_batch_tracks)
    int carry_slot = -1;              // frame slot that still holds the LAST frame of the previous async batch (its pyramids /
                                      // keypoints / descriptors): set only by a successful svo_track_uploaded_async, dropped by
                                      // every other entry point that writes frame slots (SVO_CONTINUE_CARRY_FRAME needs it)
    int online_tracked = 0;           // tracks of the last svo_add_frame pair (0 when it stopped before matching)
    double pose[16];
    // ---- ORB path (allocated on first use: orb_alloc)
    bool orb_ready = false;
    bool orb_qt_parallel = false;            // the node-parallel quadtree kernel is usable for this configuration
    bool orb_level0_in_slot = false;         // the last extraction copied level 0 into the image slots (false: read in place, OrbL0)
    bool orb_resize_staged = false;          // SVO_ORB_RESIZE_STAGED: the table-driven staged kernel (resize.hip) on every level (A/B measurements, its tests)
    ResizeShape orb_resize_shape[svo::kOrbMaxLevels];    // that kernel's launch shape for level l >= 1
    bool orb_copy_level0 = false;            // SVO_ORB_COPY_LEVEL0: level 0 copied into the slot even where it could be read in place (A/B, its test)
    svo::OrbGeom orb_geom;
    uint8_t *orb_slots = nullptr, *orb_blur = nullptr;
    void *orb_xtab = nullptr, *orb_ytab = nullptr;       // cv::resize coordinate / weight tables
    float4 *orb_cell_cand = nullptr; int *orb_cell_cnt = nullptr;
    float4 *orb_lvl_cand = nullptr; int *orb_lvl_cnt = nullptr;
    int orb_node_cap = 0;                                // quadtree node capacity (largest level quota + slack)
    void *orb_qkeys = nullptr, *orb_qtmp = nullptr;      // quadtree key scratch (inputs larger than its LDS)
    int *orb_sel = nullptr, *orb_sel_cnt = nullptr, *orb_overflow = nullptr;
    void *orb_kps = nullptr; uint8_t *orb_desc = nullptr; int *orb_n = nullptr; int orb_kp_cap = 0, orb_cand_cap = 0;
    int *orb_midx[2] = {nullptr, nullptr}; float *orb_mdist[2] = {nullptr, nullptr};
    // ---- guided ORB matcher (svo_set_orb_matcher, orb_match.hip; off and nothing allocated until it is selected)
    int orbm_mode = SVO_ORB_MATCHER_BRUTE, orbm_th_stereo = 75, orbm_th_track = 100;
    double orbm_ratio = 0.9, orbm_radius = 0.0, orbm_max_disparity = 0.0;     // (the kernels take them as floats)
    int orbm_epoch = 0;                                  // selection count: a frame block written under another epoch has no stereo data
    int orbm_kc = 0; size_t orbm_frame_bytes = 0;        // keypoints per block (orb_kp_cap rounded up to 4), bytes of a frame's block
    uint8_t *orbm_frames = nullptr;                      // per frame slot: header, uR, sad, 128-byte patches
    float2 *orbm_t2 = nullptr; int *orbm_mj = nullptr; unsigned *orbm_mkey = nullptr, *orbm_win = nullptr;    // per pair x orbm_kc
    svo::OrbL0 orb_l0{}; int orb_l0_slot0 = 0;           // where the last extraction read level 0 in place (img null: it copied), its first image slot
    // ---- pinned host scratch, cut up by pinned_layout() (pinned_layout.h): device counts, the block of list / record
    //      read-backs, the step records.  Reached through abi_io.h only (count_fetch, pinned_block, pinned_records).
    void *h_pinned = nullptr; svo::PinnedLayout pinned;
    // ---- overlap mode (svo_set_overlap): the pose stage of batch k runs on side_stream while
    //      the caller's stream already ingests / tracks batch k+1
    bool overlap = false;
    hipStream_t side_stream = nullptr;
    // ---- host-frame batches (svo_upload_frames): two device frame buffers filled on copy_stream
    uint8_t *fb[2] = {nullptr, nullptr};
    hipStream_t copy_stream = nullptr;
    hipEvent_t ev_up[2] = {nullptr, nullptr}, ev_fb_free[2] = {nullptr, nullptr};
    bool fb_used[2] = {false, false};
    int fb_frames[2] = {0, 0};
    int fb_first[2] = {0, 0};          // first frame slot of the last upload into the buffer (svo_upload_frames_at: 0 or 1)
    // svo_track_uploaded_async: two result buffers, collected in launch order
    svo_step_result *d_async[2] = {nullptr, nullptr};
    hipEvent_t ev_async[2] = {nullptr, nullptr};
    int async_n[2] = {0, 0};          // pairs of the outstanding batch in each buffer (0 = free)
    unsigned async_head = 0, async_tail = 0;   // next to collect / next to launch
    int async_last_pairs = 0;         // pairs of the most recently launched async batch
    const double *seed_dev = nullptr; // device-side seed pose of the next chain launch (continue_chain)
    hipStream_t fetch_stream = nullptr;
    bool async_ready = false;                 // d_async / ev_async / fetch_stream all exist (set after the last of them succeeded)
    hipEvent_t ev_front = nullptr, ev_back = nullptr;
    hipEvent_t ev_order = nullptr;    // svo_wait_stream / svo_signal_stream (made on first use)
    bool back_pending = false;
    int *kp_n_snap = nullptr;         // n_prev / n_cur (/ ORB capacity flags) of the batch the pose stage works on: 3 x max_batch
    // ---- stream set (svo_streams_create; empty until then)
    StreamSet streams;
    // ---- cv::resize (svo_resize) and the ingest stage (svo_ingest_*); nothing is allocated until they are used
    std::vector<ResizeTab> resize_tabs;
    DevScratch resize_scratch[2];                        // device copies of svo_resize's HOST source / destination
    Ingest ingest;
    // ---- FAST corner buckets (svo_set_fast_buckets; off and nothing allocated until then)
    int bucket_w = 0, bucket_h = 0, bucket_keep = 0;     // cell size in pixels, corners kept per cell (0: off)
    DevScratch bucket_cells;                             // per-cell words of grids too large for LDS: 4 ints x cells x n_img
    DevScratch bucket_stage;                             // svo_bucket_corners: the caller's list as structure of arrays (+ its cells)
    // ---- Shi-Tomasi detector (svo_set_lk_detector / svo_gftt_detect; off and nothing allocated until then)
    int lk_detector = SVO_DETECTOR_FAST;
    int gftt_max_corners = 0;
    double gftt_quality = 0.0, gftt_min_distance = 0.0;
    GfttBuf gftt_fused, gftt_stage;                      // scratch of the fused path (n_img images of the context's size) / of the stage calls
    // ---- robust pose refinement after solvePnPRansac (svo_set_pose_refine / svo_refine_pose; off and nothing allocated until then)
    int refine_mode = SVO_REFINE_OFF, refine_rounds = 4, refine_iters = 10, refine_min_inliers = 6;
    double refine_sigma = 1.0;
    uint8_t *refine_buf = nullptr;                       // ONE block: records, per-point flags, stage-call scratch (refine.hip)
    uint8_t *ba_buf = nullptr;                           // SVO_REFINE_BA: the pairs' points, two buffers, + stage-call scratch (ba.hip)
    // ---- the online chain's stages (their lifecycle: chain_event, pipeline.hip)
    CarryStage carry;
    WindowStage win;
    KeyframeStage kf;
    LastLaunch last;
    // ---- timing
    // stage marks are HIP events recorded on the context's stream; they are resolved (elapsed
    // times averaged per stage over all steps since the last query) in svo_get_timing
    bool timing = false;
    std::vector<hipEvent_t> ev_pool;                               // every timing event made so far, reused after each query
    size_t ev_used = 0;
    std::vector<std::pair<const char *, hipEvent_t>> marks;        // log since the last query
    std::vector<std::pair<const char *, float>> last_times;
};

#define SVO_HIP(call)                                                                         \
    do {                                                                                      \
        hipError_t e__ = (call);                                                              \
        if (e__ != hipSuccess) {                                                              \
            ctx->err = std::string(#call) + ": " + hipGetErrorString(e__);                    \
            return SVO_ERR_HIP;                                                               \
        }                                                                                     \
    } while (0)

#define SVO_TRY(call)                                                                         \
    do {                                                                                      \
        const int rc__ = (call);                                                              \
        if (rc__ != SVO_OK) return rc__;                                                      \
    } while (0)

#define SVO_ARG(cond, msg)                                                                    \
    do {                                                                                      \
        if (!(cond)) { ctx->err = std::string("bad argument: ") + msg; return SVO_ERR_ARG; }   \
    } while (0)

namespace svo {
// the schedule limits of every robust optimiser (refine.hip, ba.hip, window.hip), setters and stage calls alike
inline int check_optimiser_params(svo_ctx *ctx, int rounds, int iters, double sigma_px)
{
    SVO_ARG(rounds >= 1 && rounds <= 16, "rounds outside 1..16");
    SVO_ARG(iters >= 1 && iters <= 100, "iters outside 1..100");
    SVO_ARG(std::isfinite(sigma_px) && sigma_px > 0.0, "sigma_px must be finite and > 0");
    return SVO_OK;
}
// svo_abi.hip: the context's device memory, events and streams (DevArena)
int dev_alloc_raw(svo_ctx *ctx, void **out, size_t bytes);
template <class T> inline int dev_alloc(svo_ctx *ctx, T **out, size_t bytes) { return dev_alloc_raw(ctx, (void **)out, bytes); }
int dev_defer(svo_ctx *ctx, std::function<int()> fn);      // runs fn now, or after dev_commit while the arena is being planned
// s holds at least `bytes` afterwards.  Growing allocates the larger block first, swaps it in and frees the old one (hipFree
// waits for the launches that still read it; its contents are NOT carried over): a refused growth leaves s, and with it the
// context, as it was, with ctx->err set.
int dev_reserve(svo_ctx *ctx, DevScratch *s, size_t bytes);
// make *ev / *st unless it exists already
int dev_event(svo_ctx *ctx, hipEvent_t *ev, unsigned flags = hipEventDisableTiming);
int dev_stream(svo_ctx *ctx, hipStream_t *st);
// geometry.hip: triangulation and solvePnPRansac
int geom_workspace_bytes(const svo_config &cfg, int n_items, size_t *bytes);
int geom_workspace_init(svo_ctx *ctx);
int stage_triangulate(svo_ctx *ctx, const double P1[12], const double P2[12], const svo_pt2f *x1, const svo_pt2f *x2, int n,
                      svo_pt3f *out, int mem);
int stage_pnp_ransac(svo_ctx *ctx, const svo_pt3f *obj, const svo_pt2f *img, int n, const double K[9], int iterations,
                     float reproj_err, double confidence, svo_pnp_result *res, uint8_t *inlier_mask, int mem);
// snap: the frames' keypoint counts / capacity flags to freeze into ctx->kp_n_snap beside the triangulation (null: none)
struct SnapSpec { const int *n, *ovf; int fp0, fc0, fstep, per; };
void launch_triangulate_batch(svo_ctx *ctx, int n_items, int max_pts, const float2 *x1, const float2 *x2,
                              const int *n_pts, int n_fixed, const SnapSpec *snap = nullptr, hipStream_t st = nullptr);   // st null: the context's stream
void launch_snap_counts(svo_ctx *ctx, int n_items, const SnapSpec &snap, hipStream_t st);
void launch_pnp_batch(svo_ctx *ctx, int n_items, const float2 *img, const int *n_pts, int n_fixed, hipStream_t st);
void launch_pnp_item(svo_ctx *ctx, int item, const float *X3, const float2 *img, const int *n_pts, hipStream_t st);    // one more solve, workspace item `item`
const PnpRecord *pnp_record(const svo_ctx *ctx, int item);
const uint8_t *pnp_inlier_mask(const svo_ctx *ctx);
// refine.hip: pose_refine_kernel, one workgroup per pair, on the records solvePnPRansac left in ctx->pnp_ws
int refine_alloc(svo_ctx *ctx);                          // the stage's device block, on first use (waits for the device)
void launch_refine_batch(svo_ctx *ctx, int n_pairs, hipStream_t st);
int stage_refine_pose(svo_ctx *ctx, const svo_pt3f *obj, const svo_pt2f *img_left, const svo_pt2f *img_right, int n, const double P1[12],
                      const double P2[12], const double rvec0[3], const double tvec0[3], svo_refine_result *res, uint8_t *active, int mem);
int refine_read_result(svo_ctx *ctx, int pair, svo_refine_result *res, uint8_t *active, int cap, int *n_out);
// ba.hip: pose_ba_kernel, the stage's SVO_REFINE_BA mode (pose and points together); same records, same flags
int ba_alloc(svo_ctx *ctx);                              // refine_alloc + the mode's point buffers, on first use
void launch_ba_batch(svo_ctx *ctx, int n_pairs, hipStream_t st);
int stage_refine_ba(svo_ctx *ctx, const svo_pt3f *obj, const svo_pt2f *img1_left, const svo_pt2f *img1_right, const svo_pt2f *img2_left,
                    const svo_pt2f *img2_right, int n, const double P1[12], const double P2[12], const double rvec0[3],
                    const double tvec0[3], svo_refine_result *res, uint8_t *active, double *X_out, int mem);
int ba_read_points(svo_ctx *ctx, int pair, double *X, int cap, int *n_out);
// orb.hip
int orb_alloc(svo_ctx *ctx);
int orb_max_keypoints(const svo_ctx *ctx);             // what one image holds at most: the level quotas + 8 each, capped at orb_kp_cap
void timing_mark(svo_ctx *ctx, const char *name);     // HIP event on the context's stream when timing is enabled
int stage_host_image(svo_ctx *ctx, const uint8_t *img, int pitch, int stage_idx, const uint8_t **dptr, int *dpitch);
int orb_extract_batch(svo_ctx *ctx, const uint8_t *img, const uint8_t *img2, int pitch, int64_t img_stride, int slot0,
                      int n_img, hipStream_t st, bool in_place = false);
int orb_match_pairs(svo_ctx *ctx, int n_pairs, int fp0, int fc0, int fstep, hipStream_t st);
void orb_launch_match_fixed(svo_ctx *ctx, const uint8_t *q, int nq, const uint8_t *t, int nt, hipStream_t st);
// orb_match.hip: the guided ORB matcher
int orbm_alloc(svo_ctx *ctx);                            // its device blocks, on first use
int orbm_stereo_frames(svo_ctx *ctx, int slot0, int n_frames, hipStream_t st);      // stage S on frames just extracted into image slots slot0 ..
int orbm_track_pairs(svo_ctx *ctx, int n_pairs, int fp0, int fc0, int fstep, hipStream_t st, int *idx_prev = nullptr, int *idx_cur = nullptr);
// resize.hip
// cv::resize's INTER_LINEAR tap tables, xt[dw] and yt[dh], for inv = the destination's size over the source's
void resize_linear_tables(int sw, int sh, int dw, int dh, double inv_x, double inv_y, int2 *xt, int4 *yt);
// the workgroup shape for tables xt[dw], yt[dh], its staged rows within lds_budget bytes
ResizeShape resize_shape(int interp, int dw, int dh, const int2 *xt, const int4 *yt, size_t lds_budget);
int resize_plan(svo_ctx *ctx, int sw, int sh, int dw, int dh, int interp, double fx, double fy, int *tab);
// n_frames images per eye (eye 1 may be null), frame f at base + f * stride; one launch (n_frames x eyes <= 65535: grid.z)
int resize_launch_tab(svo_ctx *ctx, const ResizeShape &shape, int interp, const int2 *xt, const int4 *yt, int dw, int dh,
                      const uint8_t *src0, const uint8_t *src1, int spitch, int64_t sstride,
                      uint8_t *dst0, uint8_t *dst1, int dpitch, int64_t dstride, int n_frames, hipStream_t st);
int resize_launch(svo_ctx *ctx, int tab, const uint8_t *src0, const uint8_t *src1, int spitch, int64_t sstride,
                  uint8_t *dst0, uint8_t *dst1, int dpitch, int64_t dstride, int n_frames, hipStream_t st);
// pose_chain.hip: the gates and the pose chain behind a solve (the algebra is pose_device.h's)
// One step of a stream set: item i of a launch works for stream id[i]; init[i]: the stream's first frame (no previous one).
constexpr int kStreamChunk = 128;                       // items per gather / scatter / finalize launch (the table is a kernel argument)
struct StreamTable { int32_t id[kStreamChunk]; uint8_t init[kStreamChunk]; };
void launch_finalize_streams(svo_ctx *ctx, int item0, int n_items, int n_pairs, const int *n_prev, const int *n_cur, const int *ovf,
                             const StreamTable &tab, hipStream_t st);
void launch_streams_set_pose(svo_ctx *ctx, int id0, int n, const double *pose_host);    // null: identity
void launch_finalize_chain(svo_ctx *ctx, int n_pairs, const int *n_prev, const int *n_cur, const int *ovf,
                           const double *pose0_host, hipStream_t st);      // ctx->seed_dev != null: seed read on the device
int stage_chain_relative(svo_ctx *ctx, const double *T, const int32_t *ok, int n, const double *pose0_host, double *out, int mem);
// pipeline.hip: the fused steps.  Their arguments arrive checked -- the rules of each entry-point family are written once, in
// svo_abi.hip, and run before anything is copied or launched -- and their frames are DEVICE frames of the context's size,
// already ordered before the context's stream, on the device svo_abi.hip has made current.
int pipeline_add_frame(svo_ctx *ctx, const uint8_t *left, const uint8_t *right, int pitch, svo_step_result *res);
// what can break the online chain, and the one statement of which stage starts fresh after it (the rule table is its comment)
enum ChainEvent { kChainNew, kChainPoseSet, kChainCarrySet, kChainWindowSet, kChainKeyframeSet };
void chain_event(svo_ctx *ctx, ChainEvent ev);
int pipeline_track_batch(svo_ctx *ctx, const uint8_t *left_frames, const uint8_t *right_frames, int pitch, int64_t frame_stride,
                         int n_frames, const double *pose0, svo_step_result *results, int results_mem, int carry_first);
// window.hip: window_update_kernel on a caller's tables
int stage_window_update(svo_ctx *ctx, int frames, const svo_window_table *in, const svo_window_table *out, int cap, const svo_pt2f *t1_left,
                        const svo_pt2f *t1_right, const svo_pt2f *t2_left, const svo_pt2f *t2_right, const int64_t *ids, const svo_pt3f *tri,
                        int n_trk, const double *pose_a, const double *pose_b, int mem);
int window_alloc(svo_ctx *ctx, int frames);
int window_fused_step(svo_ctx *ctx, const double *pose0_host, hipStream_t st);
int window_read(svo_ctx *ctx, const svo_window_table *out, int cap);
int window_read_result(svo_ctx *ctx, svo_window_result *res);
int stage_window_ba(svo_ctx *ctx, const svo_window_table *tab, int cap, const double *P1, const double *P2, int rounds, int iters,
                    double sigma_px, int min_obs, svo_window_result *res, int mem);
// keyframe.hip: the keyframe stage of the online chain and the join kernel on a caller's arrays
int keyframe_alloc(svo_ctx *ctx);
int keyframe_fused_step(svo_ctx *ctx, const double *pose0_host, hipStream_t st);
int keyframe_read_result(svo_ctx *ctx, svo_keyframe_result *res);
int keyframe_read_matches(svo_ctx *ctx, int64_t *ids, svo_pt3f *X, svo_pt2f *xy, int32_t *trk_index, uint8_t *mask, int cap, int *n_out);
int keyframe_read_table(svo_ctx *ctx, int64_t *ids, svo_pt3f *X, int cap, int *n_out);
int stage_keyframe_join(svo_ctx *ctx, const int64_t *tab_ids, const svo_pt3f *tab_X, int n_rows, const int64_t *trk_ids,
                        const svo_pt2f *trk_xy, int n_trk, svo_pt3f *out_X, svo_pt2f *out_xy, int32_t *out_trk, int32_t *out_row,
                        int cap, int *n_out, int mem);
int carry_alloc(svo_ctx *ctx);                           // track carry: its block and, for an existing stream set, the store's share
int pipeline_streams_create(svo_ctx *ctx, int n_streams);
int pipeline_streams_reset(svo_ctx *ctx, int id);
int pipeline_streams_set_pose(svo_ctx *ctx, int id, const double *pose);
int pipeline_streams_get_pose(svo_ctx *ctx, int id, double *pose);
int pipeline_streams_check_ids(svo_ctx *ctx, const int32_t *ids, int m);      // in range, no id twice; nothing launched
int pipeline_streams_step(svo_ctx *ctx, const int32_t *ids, int m, const uint8_t *L, const uint8_t *R, int pitch,
                          int64_t frame_stride, svo_step_result *results, int results_mem);
// svo_abi.hip: the Shi-Tomasi detector of the fused LK front end (svo_set_lk_detector), n_new left images into frame slots f0 ..
int gftt_detect_frames(svo_ctx *ctx, const uint8_t *L, int pitch, int64_t frame_stride, int f0, int n_new);
// n step records from device memory to `out`, in the order of stream `st`: SVO_MEM_DEVICE: one copy, nothing waited for
// (out null: they stay where they are); SVO_MEM_HOST: through the pinned records range, and `st` is synchronised.
int deliver_records(svo_ctx *ctx, const svo_step_result *d_src, int n, svo_step_result *out, int mem, hipStream_t st);
}  // namespace svo
