/*
 * svo_abi.h -- C-ABI of the MI355X-native stereo-VO hot path (libsvo_hip.so).
 *
 * The reference (liuzhenboo/Stereo-Visual-Odometry) has no plugin/FFI layer: its hot path is
 * the private part of lzb_vio::Tracking, which calls OpenCV 3.  Each entry point below replaces
 * one of those call sites (cited as reference file:line); the host-side C++ mirror of
 * lzb_vio::{System,Tracking,Frame,...} in stereo-visual-odometry_amd/host/ and the Python test
 * binding both sit on top of exactly this surface.  INTEGRATION.md shows the reference-side
 * binding a maintainer would add.
 *
 * Conventions
 *  - plain C types only; every function returns an int status (SVO_OK == 0, < 0 hard error,
 *    > 0 soft "tracking failed" reason mirroring the reference's failure exits); nothing throws
 *    or aborts across the boundary; svo_last_error() gives a message for the last hard error.
 *  - `mem` says where the caller's buffers live: SVO_MEM_HOST (copied H2D/D2H by the call) or
 *    SVO_MEM_DEVICE (HBM pointers, e.g. a torch tensor's data_ptr(); no copies).  STREAM ORDER of device buffers: every
 *    kernel of a call runs on the context's stream (svo_set_stream) -- the pose stage of an overlap-mode batch on the
 *    context's side stream --, and the library orders nothing against other streams by itself.  A caller that produces
 *    inputs or (zero-)fills outputs on ANOTHER stream calls svo_wait_stream(ctx, that_stream) before the entry point, and
 *    svo_signal_stream(ctx, consumer_stream) -- or svo_sync() -- before it reads device-resident results from another
 *    stream (ABI v7; both are event waits on the device, no host synchronisation).
 *  - one context per (thread, GPU); calls on a context are serialised by the caller.
 *  - images are 8-bit grayscale, row-major, `pitch` bytes per row.  A call's kernels read the caller's DEVICE frames in the order
 *    of the context's stream until the call's last front-end kernel (ORB mode reads pyramid level 0 in place; LK mode runs FAST
 *    on the frame itself): frames handed over with SVO_MEM_DEVICE stay unchanged until then (svo_sync, or stream order).
 */
#ifndef SVO_ABI_H
#define SVO_ABI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SVO_ABI_VERSION 9

/* status codes */
#define SVO_OK                 0
#define SVO_ERR_ARG           -1   /* bad argument / capacity exceeded */
#define SVO_ERR_HIP           -2   /* a HIP runtime call failed */
#define SVO_ERR_NOMEM         -3
#define SVO_ERR_STATE         -4   /* e.g. pyramid slot not built */
/* soft failures of one frame step == the reference's `return false` exits */
#define SVO_FAIL_FEW_KEYPOINTS 1   /* src/tracking.cpp:261  (< 30 FAST corners)           */
#define SVO_FAIL_FEW_TRACKS    2   /* src/tracking.cpp:274  (< num_features_tracking)      */
#define SVO_FAIL_INLIER_RATIO  3   /* src/tracking.cpp:491  (inliers / tracked < rate)     */
#define SVO_FAIL_ROTATION_GATE 4   /* src/tracking.cpp:308  (|euler| >= 0.1 rad)           */
#define SVO_FAIL_TRANSL_GATE   5   /* src/tracking.cpp:311  (|t|^2 outside the window)     */
#define SVO_FAIL_CAPACITY      6   /* not a reference exit: a frame of the pair had more keypoints
                                      than svo_config.max_keypoints (cv::FAST is uncapped); the
                                      pair is reported failed instead of tracking a truncated set */

#define SVO_MEM_HOST   0
#define SVO_MEM_DEVICE 1

typedef struct svo_ctx svo_ctx;

typedef struct { float x, y; } svo_pt2f;                 /* cv::Point2f */
typedef struct { float x, y, z; } svo_pt3f;              /* cv::Point3f */
typedef struct {                                         /* cv::KeyPoint */
    float x, y, size, angle, response;
    int32_t octave, class_id;
} svo_keypoint;

/* Mirrors the live keys of config/default.yaml + capacities. */
typedef struct {
    int32_t width, height;          /* image size, fixed per context                          */
    int32_t max_keypoints;          /* capacity per image; exceeding it is SVO_ERR_ARG         */
    int32_t max_batch;              /* frame pairs per svo_track_batch launch (>= 1)           */
    int32_t num_slots;              /* pyramid slots for the stage API (>= 4)                  */
    int32_t fast_threshold;         /* 20, hard-coded at src/tracking.cpp:99                   */
    int32_t num_features_tracking;  /* config/default.yaml:69                                  */
    int32_t iterations;             /* iterationsCount, :80                                    */
    float   reproj_err;             /* reprojectionError, :81                                  */
    float   confidence;             /* confidence, :82 (a float at src/tracking.cpp:481)       */
    double  feature_match_error;    /* :66                                                     */
    double  inlier_rate;            /* :77                                                     */
    double  min_move2, max_move2;   /* squared translation gate; LK mode: 0.0005^2, 100 (:311) */
    double  P1[12], P2[12];         /* projMatr1_/projMatr2_, src/parameter.cpp:44-45, row-major 3x4.
                                       The pose stage takes K from P1 alone: fx = P1[0], fy = P1[5], cx = P1[2],
                                       cy = P1[6]; as in OpenCV 3 (K = P1(Rect(0, 0, 3, 3)), src/tracking.cpp:476-477)
                                       it ignores P1's skew P1[1] and its 4th column.  Triangulation reads all 24
                                       entries: P2 is fully general (K2 [R_rl | t_rl] of any rig).                */
    /* track_mode (config/default.yaml:75) and the ORBextractor constructor arguments (:89-93)   */
    int32_t track_mode;             /* SVO_MODE_LK ("LK_stereof2f_pnp") or SVO_MODE_ORB ("ORB_stereof2f_pnp");
                                       in ORB mode min_move2 / max_move2 = minmove^2 / maxmove^2 (:87-88).
                                       ORB mode refuses (SVO_ERR_ARG) a configuration with
                                       - more than 1024 cells on a pyramid level: level 0 has ((w - 32) / 30) x
                                         ((h - 32) / 30) cells, so about 1 MP at most (992x992 = 1024 cells is accepted,
                                         1920x1080 = 2108 cells is refused);
                                       - a level WITH cells whose keypoint area (w_l - 32) x (h_l - 32) rounds to more
                                         than 64 : 1 (the quadtree's root strips); levels without cells are not checked;
                                       - a level that rounds to 0 px (w or h / scale_factor^l < 0.5);
                                       - max_keypoints > 16384.
                                       A level whose keypoint area is more than twice as tall as wide yields no keypoints
                                       (DistributeOctTree's nIni = 0: DESIGN.md section 2). */
    int32_t orb_nfeatures;          /* nFeatures 2000 */
    float   orb_scale_factor;       /* fScaleFactor 1.2 */
    int32_t orb_nlevels;            /* nLevels 8 */
    int32_t orb_ini_th, orb_min_th; /* fIniThFAST 20, fMinThFAST 7 */
    /* ABI v6.  Order of the five float sums A11, A12, A22, b1, b2 inside cv::calcOpticalFlowPyrLK
       (src/tracking.cpp:593-618), the one place where upstream's result depends on the build's SIMD width:
       SVO_LK_ACCUM_EXACT (default): exact integer sums converted to float once -- upstream's acctype = int64
           variant, independent of any order (canonical choice C0);
       SVO_LK_ACCUM_SSE2: float accumulation in a lane order of upstream's x86 SIMD code AS RESTATED in oracle/lk.c
           mode 2 (four lanes over x = 0..19 + scalar tail for A, madd pairs (k, k + 4) over x = 0..15 + scalar tail
           for b) -- recalled from lkpyramid.cpp, NOT validated against an OpenCV binary (none exists in the build
           environment; tests/test_cv_crosscheck.py is the check for a box that has one).  Bit-identical to that
           oracle mode; about 1.9x the LK kernel time;
       SVO_LK_ACCUM_SIMD128 (ABI v7): the universal-intrinsic (CV_SIMD128) block restated whole = oracle mode 4: b
           as above, A in groups of eight pixels (four lanes over x = 0..15 + scalar tail x = 16..20).  Same cost.
       SVO_LK_ACCUM_SSE2_LEGACY (ABI v8): the older hand-written CV_SSE2 block restated whole = oracle mode 3: A as in
           SVO_LK_ACCUM_SSE2, b with one float add per pixel product (_mm_mullo / _mm_mulhi_epi16 of (It_k It_k) x (Ix_k Iy_k):
           pixels 0, 1, then 4, 5 of a group of eight into qb0, 2, 3, then 6, 7 into qb1).  About 2.2x the LK kernel time.
       Which of the three an x86 OpenCV 3 build runs depends on its version; none is validated
       against a binary.  YAML key `lk_accum: exact | sse2 | simd128 | sse2_legacy`. */
    int32_t lk_accum;
    /* ABI v6.  LK mode, fused entry points only (svo_add_frame / svo_track_*): 0 = track every cv::FAST corner, as
       the reference does (src/tracking.cpp:94-113); N > 0 = keep the N highest-response corners of every left image
       (ties: raster order first; the kept corners stay in raster order) -- BASELINE config #4's "2000 features per
       frame".  n_prev_kps / n_cur_kps then report the kept counts.  YAML key `fast_keep_strongest`. */
    int32_t fast_keep_strongest;
} svo_config;

#define SVO_MODE_LK  0
#define SVO_MODE_ORB 1
#define SVO_LK_ACCUM_EXACT 0
#define SVO_LK_ACCUM_SSE2  1
#define SVO_LK_ACCUM_SIMD128 2
#define SVO_LK_ACCUM_SSE2_LEGACY 3

typedef struct {                    /* solvePnPRansac + Rodrigues outcome */
    double rvec[3], tvec[3], R[9];
    int32_t n_inliers, ransac_iters, best_iter, lm_iters, ok, _pad;
} svo_pnp_result;

typedef struct {                    /* one Tracking::AddFrame step (LK mode) */
    int32_t ok;                     /* Track() result                                           */
    int32_t fail_stage;             /* 0 or one of SVO_FAIL_*                                   */
    int32_t n_prev_kps, n_cur_kps, n_tracked, n_inliers;
    int32_t ransac_iters, lm_iters;
    double  rvec[3], tvec[3], R[9];
    double  T_rel_inv[16];          /* inv([R t; 0 1]) -- what frame_pose_ is multiplied by     */
    double  pose[16];               /* frame_pose_ after this step (chained from the batch's
                                       initial pose; failed steps leave it unchanged)           */
} svo_step_result;

/* ---- lifecycle ------------------------------------------------------------------------- */
int         svo_abi_version(void);
int         svo_config_bytes(void);      /* sizeof(svo_config) of this build (ABI v6): a binding checks its own struct against it */
void        svo_default_config(svo_config *cfg, int width, int height);   /* default.yaml + KITTI rig */
int         svo_device_count(int *n);   /* HIP devices visible to this process (ABI v5): the multi-sequence runner deals
                                           sequences to them; SVO_ERR_HIP with *n = 0 when the runtime finds none */
int         svo_create(const svo_config *cfg, int device, svo_ctx **out);
void        svo_destroy(svo_ctx *ctx);
const char *svo_last_error(const svo_ctx *ctx);
int         svo_set_stream(svo_ctx *ctx, void *hip_stream);   /* NULL -> context's own stream */
int         svo_sync(svo_ctx *ctx);
/* ABI v7.  svo_wait_stream: everything queued on `hip_stream` so far happens-before whatever this context launches next
 * (an event recorded on hip_stream, waited for by the context's stream).  svo_signal_stream: everything this context has
 * launched so far -- the side-stream pose stage of an overlap-mode svo_track_batch included -- happens-before whatever is
 * queued on `hip_stream` next.  NULL = the legacy default stream.  Device-side waits only. */
int         svo_wait_stream(svo_ctx *ctx, void *hip_stream);
int         svo_signal_stream(svo_ctx *ctx, void *hip_stream);
/* ABI v9.  svo_signal_stream_inputs: every kernel that READS the caller's input buffers of the calls made so far (the frames
 * of svo_track_batch / svo_add_frame are read in place until the end of the front end) happens-before whatever is queued on
 * `hip_stream` next -- the stream may then overwrite or free them.  Unlike svo_signal_stream it does NOT wait for the
 * side-stream pose stage of an overlap-mode batch: a producer that calls it after every batch keeps the overlap of batch k's
 * pose stage with batch k + 1's front end (svo_signal_stream after every batch would serialise them through the producer's
 * stream).  Results are complete only after svo_signal_stream / svo_sync. */
int         svo_signal_stream_inputs(svo_ctx *ctx, void *hip_stream);
int         svo_num_levels(const svo_ctx *ctx);               /* LK pyramid levels actually built */

/* ---- stage API: one call per OpenCV call site of the reference ---------------------------- */

/* cv::FAST(img, kps, threshold, nonmax)  -- src/tracking.cpp:101 (Detect_OpenCVFASTFeatures),
 * src/ORBextractor.cpp:763,768.  Row-major ordered output. */
int svo_fast_detect(svo_ctx *ctx, const uint8_t *img, int pitch, int mem, int threshold,
                    int nonmax, svo_keypoint *out, int cap, int *n_out);

/* buildOpticalFlowPyramid half of cv::calcOpticalFlowPyrLK (src/tracking.cpp:593-618): builds the
 * padded 4-level pyramid of one image into slot `slot`; consecutive LK calls reuse it. */
int svo_build_pyramid(svo_ctx *ctx, int slot, const uint8_t *img, int pitch, int mem);
/* test/debug read-back of one level (without border) */
int svo_read_pyramid_level(svo_ctx *ctx, int slot, int level, uint8_t *out, int out_pitch, int mem,
                           int *w, int *h);

/* cv::calcOpticalFlowPyrLK(prev, next, prev_pts, next_pts, status, err, Size(21,21), 3,
 *   TermCriteria(COUNT+EPS, 30, 0.01), 0, 0.001)  -- src/tracking.cpp:593,600,607,613 */
int svo_lk_track(svo_ctx *ctx, int slot_prev, int slot_next, const svo_pt2f *prev_pts, int n,
                 svo_pt2f *next_pts, uint8_t *status, int mem);

/* Tracking::LK_Robust_Find_MuliImage_MatchedFeatures incl. deleteBadmatchFeatures
 * (src/tracking.cpp:583-660): the 4-call loop L1->R1->R2->L2->L1' fused per point, then the
 * stable filter.  out_* receive the M survivors in input order; *m_out = M. */
int svo_circular_match(svo_ctx *ctx, int slot_prevL, int slot_prevR, int slot_curL, int slot_curR,
                       const svo_pt2f *t1_left, int n, svo_pt2f *out_t1_left,
                       svo_pt2f *out_t1_right, svo_pt2f *out_t2_right, svo_pt2f *out_t2_left,
                       int *m_out, int mem);

/* cv::triangulatePoints + cv::convertPointsFromHomogeneous -- src/tracking.cpp:292-294, :190-192 */
int svo_triangulate(svo_ctx *ctx, const double P1[12], const double P2[12], const svo_pt2f *x1,
                    const svo_pt2f *x2, int n, svo_pt3f *out, int mem);

/* cv::solvePnPRansac(obj, img, K, 0, rvec, t, true, iterations, reproj_err, confidence, inliers,
 *   SOLVEPNP_ITERATIVE) + cv::Rodrigues -- src/tracking.cpp:485-488.  res is always a HOST
 * struct; inlier_mask (n bytes, may be NULL) follows `mem`. */
int svo_pnp_ransac(svo_ctx *ctx, const svo_pt3f *obj, const svo_pt2f *img, int n, const double K[9],
                   int iterations, float reproj_err, double confidence, svo_pnp_result *res,
                   uint8_t *inlier_mask, int mem);

/* ORBextractor::operator()(image, mask, keypoints, descriptors) -- src/ORBextractor.cpp:990-1055,
 * called twice per frame by Tracking::Detect_MyORBFeatures (src/tracking.cpp:502-532).  kps is a HOST
 * array of cv::KeyPoint records, desc n x 32 bytes (HOST).  per_level (8 ints, may be NULL) receives
 * the keypoints kept per pyramid level. */
int svo_orb_extract(svo_ctx *ctx, const uint8_t *img, int pitch, int mem, svo_keypoint *kps, uint8_t *desc,
                    int cap, int *n_out, int *per_level);
/* test/debug read-back of one ORB pyramid level (tight rows) of the last svo_orb_extract.  (After svo_add_frame / a batch call in
 * ORB mode level 0 may not be there -- those read it in place from the input frame -- and asking for it is SVO_ERR_ARG.) */
int svo_orb_read_level(svo_ctx *ctx, int level, uint8_t *out, int *w, int *h);
/* test/debug: FAST candidates (x, y, response, 0) of one level of the last svo_orb_extract, before the quadtree */
int svo_orb_read_candidates(svo_ctx *ctx, int level, float *out4, int cap, int *n_out);

/* DescriptorMatcher::create("BruteForce-Hamming")->match(query, train, matches) --
 * src/tracking.cpp:539-544: for every query row the first train row of minimum Hamming distance.
 * Descriptors are 32-byte rows (16-byte aligned when device-resident). */
int svo_match_hamming(svo_ctx *ctx, const uint8_t *query, int nq, const uint8_t *train, int nt, int32_t *train_idx,
                      float *distance, int mem);

/* ---- fused API: Tracking::AddFrame in LK mode (src/tracking.cpp:49-77, 258-344) ------------ */

/* Online step: feeds one stereo frame.  The first call only detects features (StereoInit_f2f,
 * :78-92) and returns SVO_OK with res->ok = 1, n_prev_kps = 0.  Later calls track against the
 * previous frame.  Returns SVO_OK (res->ok = 1), a SVO_FAIL_* code (res->ok = 0; the pose chain
 * skips this step, as the reference does), or a hard error < 0.  res is a HOST struct. */
int svo_add_frame(svo_ctx *ctx, const uint8_t *left, const uint8_t *right, int pitch, int mem,
                  svo_step_result *res);
int svo_reset(svo_ctx *ctx);                         /* back to INITING, pose = identity */
int svo_get_pose(svo_ctx *ctx, double pose[16]);     /* frame_pose_ (src/tracking.h:117)  */
int svo_set_pose(svo_ctx *ctx, const double pose[16]);   /* seeds frame_pose_ of the online path (e.g. a context
                                                            rebuilt for another frame size continues the chain) */

/* Batched step: n_frames consecutive stereo frames resident in HBM (frame f at base +
 * f*frame_stride), n_frames - 1 <= max_batch pairs processed as one set of launches
 * (every consecutive pair is independent: SURVEY.md section 0 fact 3), poses chained on device.
 * results: n_frames - 1 records, location per `results_mem`.  pose0 (host, may be NULL = identity)
 * seeds the chain.  Frame 0's features are detected as part of the batch. */
int svo_track_batch(svo_ctx *ctx, const uint8_t *left_frames, const uint8_t *right_frames,
                    int pitch, int64_t frame_stride, int n_frames, const double *pose0,
                    svo_step_result *results, int results_mem);

/* Overlap mode for svo_track_batch with DEVICE-resident results (off by default).  The pose stage
 * (RANSAC-EPnP + LM, gates, chain: one latency-bound wave per pair) of batch k then runs on a side
 * stream while the context's stream already builds pyramids / detects / tracks batch k+1.  The
 * results of a batch are complete after svo_sync(), or -- in stream order, without a host sync --
 * after svo_wait_results(); the next svo_track_batch call waits for them by itself before it
 * reuses the shared buffers. */
int svo_set_overlap(svo_ctx *ctx, int on);
int svo_wait_results(svo_ctx *ctx);

/* Host-resident frame batches: image ingest off the critical path (replaces
 * the per-frame cv::imread -> Tracking::AddFrame hand-over of reference src/System.cpp:46-58,75-104
 * for the batched runner).
 *   svo_host_alloc / svo_host_free : page-locked host memory, so decoder threads write straight
 *       into DMA-able buffers;
 *   svo_upload_frames : ASYNCHRONOUS host-to-device copy of n_frames stereo frames (frame f at
 *       base + f*frame_stride, rows `pitch` apart) into the context's device frame buffer `buf`
 *       (0 or 1) on the context's copy stream -- it runs beside the kernels of the batch that
 *       lives in the other buffer.  The host memory must stay untouched until svo_wait_upload;
 *   svo_track_uploaded : svo_track_batch on the frames of buffer `buf` (ordered after their upload
 *       on the device, no host wait). */
int svo_host_alloc(svo_ctx *ctx, size_t bytes, void **out);   /* ctx may be NULL (ABI v6): the memory is portable across
                                                                  devices, so it can be pinned while svo_create still runs */
int svo_host_free(svo_ctx *ctx, void *p);
int svo_upload_frames(svo_ctx *ctx, int buf, const uint8_t *left_frames, const uint8_t *right_frames,
                      int pitch, int64_t frame_stride, int n_frames);
/* ABI v7: the same into frame slots first_slot .. first_slot + n_frames - 1 of the buffer (svo_upload_frames = first_slot 0).
 * A stream's micro-batch whose frame 0 is CARRIED on the device (SVO_CONTINUE_CARRY_FRAME) uploads its new frames only:
 * first_slot = 1; slot 0 is then never read. */
int svo_upload_frames_at(svo_ctx *ctx, int buf, int first_slot, const uint8_t *left_frames, const uint8_t *right_frames,
                         int pitch, int64_t frame_stride, int n_frames);
int svo_wait_upload(svo_ctx *ctx, int buf);
int svo_track_uploaded(svo_ctx *ctx, int buf, int n_frames, const double *pose0,
                       svo_step_result *results, int results_mem);
/* The same without waiting for the GPU (ABI v4): the n_frames - 1 step records stay in the context
 * until svo_collect_results copies them to a HOST array (it waits for that batch only).  Up to TWO
 * batches may be outstanding, collected in launch order, so a caller keeps the GPU busy like this:
 *     upload(0); track_async(0);  upload(1); track_async(1); collect(0);  upload(2); track_async(2); collect(1); ...
 * -- the upload of chunk k+1 and, in overlap mode, the pose stage of chunk k run beside chunk k+1's
 * front end, and the host only ever waits for a batch that has a successor queued behind it.
 * continue_chain != 0 seeds the pose chain with the LAST pose of the previous async batch on the device
 * (no host round trip; pose0 is ignored); 0 seeds it with pose0 (NULL = identity).
 * ABI v6: continue_chain may also carry SVO_CONTINUE_CARRY_FRAME (continue_chain = SVO_CONTINUE_CHAIN |
 * SVO_CONTINUE_CARRY_FRAME): the caller states that frame 0 of this batch IS the last frame of the previous async batch
 * (the halo frame of a stream's micro-batches); its pyramids / keypoints / descriptors are then carried over on the device
 * instead of being computed again from the uploaded copy. */
#define SVO_CONTINUE_CHAIN       1
#define SVO_CONTINUE_CARRY_FRAME 2
int svo_track_uploaded_async(svo_ctx *ctx, int buf, int n_frames, const double *pose0, int continue_chain);
int svo_collect_results(svo_ctx *ctx, svo_step_result *results, int n_pairs);
/* ABI v6, non-blocking: *n_pairs = the pairs of the OLDEST outstanding async batch when its records are complete (a
 * following svo_collect_results does not wait), 0 when it is still running or nothing is outstanding.  What a
 * streaming caller polls between frames (host: System::StreamPoll behind Step_ros, reference src/System.cpp:60-74). */
int svo_results_ready(svo_ctx *ctx, int *n_pairs);

/* Read-back of the online state (after svo_add_frame), for callers that keep the reference's
 * per-frame carriers or draw what Tracking::displayTracking drew (src/tracking.cpp:345-382):
 *   svo_get_frame_keypoints : the keypoints detected on the frame just added.  LK mode: the
 *       cv::FAST corners of the LEFT image, in cv::FAST order, as the cv::KeyPoint records
 *       Detect_OpenCVFASTFeatures pushes into Frame::features_left_ (src/tracking.cpp:94-113);
 *       side must be 0.  ORB mode: side 0 / 1 = left / right ORB keypoints and, if `descriptors`
 *       is not NULL, their n x 32 descriptor bytes (Frame::left_/right_Descriptors_, :511-526).
 *   svo_get_last_tracks : the matched tracks that fed the pose solver for the pair just tracked
 *       (t1_left, t1_right, t2_right -- zeros in ORB mode --, t2_left) and the RANSAC inlier flags;
 *       n = 0 when the step stopped before matching.  Any output pointer may be NULL.
 * Host pointers; capacities in elements; SVO_ERR_ARG when a capacity is too small. */
int svo_get_frame_keypoints(svo_ctx *ctx, int side, svo_keypoint *kps, uint8_t *descriptors, int cap, int *n_out);
int svo_get_last_tracks(svo_ctx *ctx, svo_pt2f *t1_left, svo_pt2f *t1_right, svo_pt2f *t2_right,
                        svo_pt2f *t2_left, uint8_t *inlier, int cap, int *n_out);
/* ABI v6: the same for pair `pair` (0-based) of the most recent svo_track_batch / svo_track_uploaded(_async) launch --
 * valid until the next launch on this context; waits for that batch's pose stage. */
int svo_get_batch_tracks(svo_ctx *ctx, int pair, svo_pt2f *t1_left, svo_pt2f *t1_right, svo_pt2f *t2_right,
                         svo_pt2f *t2_left, uint8_t *inlier, int cap, int *n_out);

/* ---- stream sets: many independent LIVE stereo streams through one launch set (additive; detected by symbol, the ABI
 * version stays 9) ---------------------------------------------------------------------------------------------------
 * A live camera has no future frames, so svo_add_frame tracks one pair per call and leaves the chip almost empty.  Every
 * pair is independent of every other ACROSS cameras as it is along time: a stream set keeps,
 * for each of n_streams streams, what one lzb_vio::Tracking keeps between AddFrame calls -- last_frame_'s features
 * (LK mode: both pyramids, the FAST corners; ORB mode: both images' keypoints and descriptors), frame_pose_ and the
 * INITING / TRACKING status (reference src/tracking.h:105-117) -- in device memory, and one svo_streams_step does for m
 * of them what m Tracking::AddFrame calls do (src/tracking.cpp:49-77), as ONE set of launches.  All streams share the
 * context's frame size, rig, mode and every other svo_config field.
 *   svo_streams_create : allocates the set (once per context; SVO_ERR_ARG on a second call or n_streams < 1).  A context
 *       that never calls it pays nothing.
 *   svo_streams_count  : *n_streams = streams of the set, 0 before svo_streams_create.
 *   svo_streams_step   : frame i (at base + i * frame_stride, rows `pitch` apart, where `mem` says) is the next stereo
 *       frame of stream stream_ids[i]; results[i] (where `results_mem` says; NULL with SVO_MEM_DEVICE: the records stay
 *       in the context) is its step record.  The ids are distinct, in any order, any subset: 1 <= m <=
 *       (max_batch + 1) / 2 -- the step uses 2 m of the context's max_batch + 1 working frame slots, so a caller that
 *       advances 128 streams a call creates the context with max_batch = 256.  A stream's first frame since its reset
 *       gives the StereoInit_f2f record (:78-92): ok = 1, n_prev_kps = 0, R = T_rel_inv = I, pose = the stream's pose.
 *       Later frames track against the stream's previous frame, which the new one replaces on success AND on every
 *       SVO_FAIL_* outcome (last_frame_ = current_frame_, :59-68); a failed step leaves the stream's pose unchanged.
 *       Returns SVO_OK or a hard error < 0; soft failures are in results[i].ok / .fail_stage only.  Each record is what
 *       svo_add_frame returns for the same frames on a context of its own, bit for bit.
 *       SVO_MEM_HOST frames are copied by the call (one frame: the staging of svo_add_frame; more: frame buffer 0 of
 *       svo_upload_frames, whose previous contents are lost) and are free again when it returns.  SVO_MEM_HOST results: the
 *       call returns when they are there.  SVO_MEM_DEVICE results: in stream order on the context's stream, no host
 *       synchronisation inside the call; the poses live on the device, so a queued step depends on no host memory.
 *       Overlap mode, the async queue and SVO_CONTINUE_* do not apply to stream steps.
 *   svo_streams_reset  : that stream (-1: every stream) back to INITING, pose = identity (svo_reset per
 *       stream); in stream order after the steps queued so far.
 *   svo_streams_get_pose / svo_streams_set_pose : the stream's frame_pose_ (src/tracking.h:117); set seeds the chain as
 *       pose0 seeds svo_track_batch.  HOST pointers; get waits for the steps queued so far.
 *   svo_streams_get_tracks : svo_get_batch_tracks for item `item` of the most recent step (n = 0 for an init item).
 * The set is separate memory: svo_add_frame, svo_track_batch, the stage API ... keep working on the same context and do not
 * disturb the streams.  In the other direction a step is one more writer of the working frame slots, exactly like
 * svo_track_batch: it waits for a pending overlap-mode pose stage, ends a carried frame (SVO_CONTINUE_CARRY_FRAME), and
 * svo_add_frame's two-frame ring does not survive it -- call svo_reset before svo_add_frame is used again. */
int svo_streams_create(svo_ctx *ctx, int n_streams);
int svo_streams_count(const svo_ctx *ctx, int *n_streams);
int svo_streams_step(svo_ctx *ctx, const int32_t *stream_ids, int m, const uint8_t *left_frames,
                     const uint8_t *right_frames, int pitch, int64_t frame_stride, int mem,
                     svo_step_result *results, int results_mem);
int svo_streams_reset(svo_ctx *ctx, int stream_id);
int svo_streams_get_pose(svo_ctx *ctx, int stream_id, double pose[16]);
int svo_streams_set_pose(svo_ctx *ctx, int stream_id, const double pose[16]);
int svo_streams_get_tracks(svo_ctx *ctx, int item, svo_pt2f *t1_left, svo_pt2f *t1_right, svo_pt2f *t2_right,
                           svo_pt2f *t2_left, uint8_t *inlier, int cap, int *n_out);

/* ---- cv::resize and the ingest stage: full-size camera frames downscaled on the GPU before tracking (additive; detected by
 * symbol, the ABI version stays 9 and svo_config is unchanged) -----------------------------------------------------------
 * The reference resizes both images before Tracking::AddFrame -- cv::resize(img, img, cv::Size(), 0.5, 0.5, cv::INTER_NEAREST)
 * at src/System.cpp:94-97, the same with 0.6 at app/ros/robust-vslam/src/robust_vslam_ros.cpp:86-89 -- and every other entry
 * point of this library takes frames of exactly the context's width x height.  The calls below take frames of ANOTHER
 * (larger or equal) size and make working-size frames of them on the device.
 *
 * Semantics, bit for bit (restated from OpenCV 3's resize.cpp; "parity unpinned": no OpenCV binary exists in the build
 * environment).  Source sw x sh, destination dw x dh, 8-bit gray, both with a row pitch.  The scale is given
 *   - in FACTOR form, fx > 0 and fy > 0 (cv::resize(src, dst, Size(), fx, fy)): inv_x = fx, and dw must equal
 *     cvRound(sw * fx) (rint, ties to even), likewise dh, else SVO_ERR_ARG; or
 *   - in SIZE form, fx = fy = 0 (cv::resize(src, dst, Size(dw, dh))): inv_x = (double)dw / sw, likewise y.
 * scale_x = 1.0 / inv_x in double, likewise y.  Only 0 < inv <= 1 on both axes (downscale or identity) and sw, sh <= 8192;
 * anything else is SVO_ERR_ARG.
 *   SVO_INTERP_NEAREST: dst[dy][dx] = src[min((int)floor(dy * scale_y), sh - 1)][min((int)floor(dx * scale_x), sw - 1)].
 *   SVO_INTERP_LINEAR : scale_x == 2.0 && scale_y == 2.0 exactly: upstream reroutes INTER_LINEAR to its integer-area path,
 *       dst[y][x] = (s[2y][2x] + s[2y][2x+1] + s[2y+1][2x] + s[2y+1][2x+1] + 2) >> 2; needs 2 dw <= sw and 2 dh <= sh
 *       (SVO_ERR_ARG otherwise: upstream's partial-window tail is not restated).  Any other scale: the 11-bit fixed-point
 *       bilinear of the ORB pyramid (orc_resize_linear_u8 in oracle/orb.c), with scale_x / scale_y as defined above.
 *
 * svo_scale_projection (no context, no device): the projection matrix of the resized image, P_out = S * P with
 *   S = [[inv_x, 0, ox], [0, inv_y, oy], [0, 0, 1]]; nearest: ox = oy = 0 (destination pixel dx shows source pixel
 *   dx * scale_x); linear, both branches: ox = 0.5 (inv_x - 1), oy = 0.5 (inv_y - 1) (pixel centres: x_dst =
 *   (x_src + 0.5) inv_x - 0.5).  A context that tracks resized frames is created with its P1 / P2 passed through it.
 *   Thresholds in pixels (feature_match_error, reproj_err, the FAST thresholds) are the caller's configuration AT THE
 *   WORKING SIZE and are not touched.
 * svo_resize (stage API): n_frames images, frame f at base + f * stride (strides ignored for n_frames = 1), any sizes within
 *   the limits above, independent of the context's frame size.  `mem` says where BOTH images live; SVO_MEM_DEVICE: one launch
 *   in stream order on the context's stream, no host synchronisation; SVO_MEM_HOST: copied through device scratch that
 *   grows on demand, returns when dst is complete.  Bytes of a destination row beyond dw are not written.  The tap tables
 *   of a geometry (sizes, interp, factors) are built on the host on first use and cached in the context (at most 64
 *   distinct geometries per context; 8 bytes per destination column + 16 per row on the device).
 * svo_ingest_create : the ingest stage of a context, source size -> the context's width x height.  Once per context (a
 *   second call: SVO_ERR_ARG); a context that never calls it allocates and pays nothing.  It allocates the working-size
 *   device frames the ingest calls resize into: 2 x (max_batch + 1) frames of align256(width) x height bytes (960 x 540,
 *   max_batch = 256: 284 MB).  Source-size staging for HOST frames comes on first use: svo_ingest_add_frame /
 *   svo_ingest_streams_step 2 x m frames of align16(src_width) x src_height bytes, svo_ingest_upload_frames_at
 *   2 x (max_batch + 1) such frames per upload buffer (1920 x 1080, max_batch = 256: 1.07 GB per buffer, 2.1 GB for both).
 *   The other svo_ingest_* calls before it: SVO_ERR_STATE.
 * svo_ingest_info   : what the stage was created with, and inv_x / inv_y to hand to svo_scale_projection.
 * svo_ingest_X (add_frame, track_batch, streams_step, upload_frames_at): svo_X on source-size frames.  `pitch` and
 *   `frame_stride` describe the SOURCE frames.  The contract is one sentence: its records and every later read-back
 *   (svo_get_last_tracks, svo_get_batch_tracks, svo_streams_get_tracks, svo_get_frame_keypoints, poses) are byte for byte
 *   what svo_X gives when it is fed the frames svo_resize makes of the same sources.  Same argument rules, same return
 *   codes, same stream order as svo_X: the resize runs on the stream svo_X reads its frames on (svo_ingest_upload_frames_at:
 *   the copy stream, so svo_wait_upload, svo_track_uploaded(_async), SVO_CONTINUE_CARRY_FRAME and svo_collect_results work
 *   unchanged behind it), device frames are read in stream order (they may be overwritten once svo_signal_stream_inputs /
 *   svo_sync says so), and with device frames and device results nothing synchronises with the host.  The working-size
 *   frames of call k are not overwritten before call k's front end has read them (stream order).
 * The plain entry points keep working on a context with an ingest stage, on working-size frames, undisturbed. */
#define SVO_INTERP_NEAREST 0
#define SVO_INTERP_LINEAR  1
int svo_scale_projection(const double P[12], double inv_x, double inv_y, int interp, double P_out[12]);
int svo_resize(svo_ctx *ctx, const uint8_t *src, int sw, int sh, int spitch, int64_t sstride,
               uint8_t *dst, int dw, int dh, int dpitch, int64_t dstride, int n_frames,
               int interp, double fx, double fy, int mem);
int svo_ingest_create(svo_ctx *ctx, int src_width, int src_height, int interp, double fx, double fy);
int svo_ingest_info(const svo_ctx *ctx, int *src_width, int *src_height, int *interp, double *inv_x, double *inv_y);
int svo_ingest_add_frame(svo_ctx *ctx, const uint8_t *left, const uint8_t *right, int pitch, int mem, svo_step_result *res);
int svo_ingest_track_batch(svo_ctx *ctx, const uint8_t *lefts, const uint8_t *rights, int pitch, int64_t frame_stride,
                           int n_frames, const double *pose0, svo_step_result *results, int results_mem);
int svo_ingest_streams_step(svo_ctx *ctx, const int32_t *stream_ids, int m, const uint8_t *lefts, const uint8_t *rights,
                            int pitch, int64_t frame_stride, int mem, svo_step_result *results, int results_mem);
int svo_ingest_upload_frames_at(svo_ctx *ctx, int buf, int first_slot, const uint8_t *lefts, const uint8_t *rights,
                                int pitch, int64_t frame_stride, int n_frames);

/* ---- FAST corner buckets: the strongest corners per grid cell before LK tracking (additive; detected by symbol, the ABI
 * version stays 9 and svo_config is unchanged) ---------------------------------------------------------------------------
 * The LK step's cost is proportional to the corners it is handed, and cv::FAST is uncapped (src/tracking.cpp:94-113).
 * svo_config.fast_keep_strongest bounds the count but not where the corners lie; the reference's author asked for spacing
 * too (cv::GFTTDetector::create(n, 0.01, 20) at src/tracking.cpp:18, never called).  Bucketing keeps coverage of the image:
 *
 * Semantics.  A grid of cell_w x cell_h pixel cells anchored at (0, 0): ceil(w / cell_w) x ceil(h / cell_h) cells, edge
 * cells may be partial; a corner at integer (x, y) belongs to cell (y / cell_h) * cols + x / cell_w.  Per image and per cell
 * the per_cell corners of highest response stay (ties: raster order first); the survivors stay in raster order with their
 * responses intact -- np.argsort(-response, kind="stable")[:per_cell] per cell, then a sort of the kept indices.  At most
 * 16384 cells per image.
 *   svo_set_fast_buckets : LK mode, fused entry points only (svo_add_frame, svo_track_batch, svo_track_uploaded(_async),
 *       svo_streams_step and their svo_ingest_* twins).  per_cell = 0 (the default): off, the sizes are ignored.  May be
 *       called at any time between calls on the context and applies to frames whose corners are detected by LATER calls: a
 *       frame already detected (svo_add_frame's previous frame, a stream's stored frame, a carried frame) keeps its corners.
 *       svo_config.fast_keep_strongest = N > 0 runs AFTER the buckets, on their survivors.  n_prev_kps / n_cur_kps, the
 *       < 30 gate, svo_get_frame_keypoints and the tracks read-backs see the kept set, as with fast_keep_strongest; a frame
 *       whose RAW corner count exceeds max_keypoints is left alone and still ends in SVO_FAIL_CAPACITY.  SVO_ERR_ARG:
 *       cell_w < 1, cell_h < 1, per_cell < 0, more than 16384 cells at the context's size, an ORB-mode context (ORB mode
 *       spreads its keypoints with the quadtree).  Grids of more than 3072 cells keep their per-cell words in device memory
 *       (16 bytes x cells x (max_batch + 1)), allocated by the call that first asks for such a grid (that call waits for the
 *       device); a context that never enables buckets allocates and pays nothing.
 *   svo_get_fast_buckets : what is set (0, 0, 0 while off).  Any pointer may be NULL.
 *   svo_bucket_corners (stage API): the same kernel on a caller's list -- any raster-ordered list of n records with integer
 *       coordinates inside width x height and responses in 1..255 --, independent of the context's frame size and mode.
 *       out receives the survivors as the records cv::FAST makes (x, y, response of the input; size 7, angle -1, octave 0,
 *       class_id -1), *n_out their count.  `mem` says where in, out AND n_out live; SVO_MEM_DEVICE: in stream order on the
 *       context's stream, no host synchronisation (device scratch of 12 bytes per corner grows on demand; a call that grows
 *       it waits for the device); SVO_MEM_HOST: returns when out is complete.  in == out is allowed.  SVO_ERR_ARG: n > cap,
 *       per_cell < 1, a size < 1 or > 16384, more than 16384 cells. */
int svo_set_fast_buckets(svo_ctx *ctx, int cell_w, int cell_h, int per_cell);
int svo_get_fast_buckets(const svo_ctx *ctx, int *cell_w, int *cell_h, int *per_cell);
int svo_bucket_corners(svo_ctx *ctx, const svo_keypoint *in, int n, int width, int height,
                       int cell_w, int cell_h, int per_cell, svo_keypoint *out, int cap, int *n_out, int mem);

/* ---- Shi-Tomasi corners: cv::goodFeaturesToTrack as the LK-mode detector (additive; detected by symbol, the ABI version
 * stays 9 and svo_config is unchanged) -------------------------------------------------------------------------------------
 * The detector the reference's author prepared and never called: cv::GFTTDetector::create(num_features, 0.01, 20)
 * (src/tracking.cpp:18,41), i.e. cv::goodFeaturesToTrack(img, maxCorners, qualityLevel, minDistance, noArray(), 3, false,
 * 0.04).  A bounded, strength-ordered corner set spaced at least minDistance apart.  The default detector stays cv::FAST.
 *
 * Semantics (restated from memory of OpenCV 3.4, unpinned; every choice is listed in DESIGN.md section 2; the numpy twin is
 * tests/_gftt_ref.py).  float32 with one rounding per operation (no fused multiply-add) unless stated; s = float(1/(4*3*255)),
 * f0 = 2s, f1 = s; image border reflect-101.
 *   1. dx: r = p[x+1] - p[x-1] in integers, dx = float(r[y])*f0 + float(r[y-1] + r[y+1])*f1.
 *   2. dy: q = float(p[x])*f0 + float(p[x-1] + p[x+1])*f1, dy = q[y+1] - q[y-1].
 *   3. cxx = dx*dx, cxy = dx*dy, cyy = dy*dy.
 *   4. Sxx, Sxy, Syy: 3x3 unnormalised box sums, accumulated in double -- the three products of a row first, (p0 + p1) + p2, then
 *      the rows, (r0 + r1) + r2 -- and rounded once; the border is reflect-101 OF THE
 *      COVARIANCE MAPS (c(-1, y) := c(1, y)), not the covariance of the reflected image.
 *   5. a = Sxx*0.5f, b = Sxy, c = Syy*0.5f; eig = (a + c) - sqrtf((a - c)*(a - c) + b*b), correctly rounded sqrt; tiny
 *      negative values are kept.
 *   6. thr = float(double(max eig over the image) * double(qualityLevel)).
 *   7. Candidates: 1 <= x <= w-2, 1 <= y <= h-2, eig > thr, eig >= all eight neighbours.
 *   8. Order: eig descending, ties to the LARGER raster index y*w + x first.
 *   9. minDistance >= 1: cell = cvRound(minDistance) (half to even), grid of ceil(w/cell) x ceil(h/cell) cells; a candidate is
 *      dropped when a kept corner in its 3x3 cell neighbourhood has integer dx*dx + dy*dy < double(minDistance)^2, else kept;
 *      stop at maxCorners when maxCorners > 0.  minDistance < 1: the first maxCorners of the order.  maxCorners <= 0: uncapped.
 *  10. Output in SELECTION order (strongest first), each the record GFTTDetector::detect makes: (x, y, size 3, angle -1,
 *      response 0, octave 0, class_id -1).
 *   svo_set_lk_detector : LK mode.  Applies to frames whose corners are detected by LATER calls on every fused entry point
 *       (svo_add_frame, svo_track_batch, svo_track_uploaded(_async), svo_streams_step and their svo_ingest_* twins): a frame
 *       already detected (svo_add_frame's previous frame, a stream's stored frame, a carried frame) keeps its corners.
 *       n_prev_kps / n_cur_kps, the < 30 gate, svo_get_frame_keypoints (records as in 10) and the tracks read-backs see the kept
 *       set.  An image with more CANDIDATES (step 7) than svo_config.max_keypoints gets no list and its pairs end in
 *       SVO_FAIL_CAPACITY.  SVO_DETECTOR_FAST switches back; the other arguments are ignored.  SVO_ERR_ARG (nothing changes):
 *       an ORB-mode context; an unknown detector; quality_level not in (0, inf) or not finite; min_distance negative, not
 *       finite, or >= 1 with more than 16384 grid cells at the context's size; SVO_DETECTOR_GFTT while the FAST buckets are on or
 *       svo_config.fast_keep_strongest > 0 -- and svo_set_fast_buckets with per_cell > 0 while the detector is GFTT.
 *       Memory: allocated by the first call that selects SVO_DETECTOR_GFTT (that call, and one that needs more, waits for the
 *       device), per working frame (max_batch + 1 of them) one float per pixel (rows of align64(width)) -- the eigenvalue where
 *       the pixel is a candidate before the threshold -- 8 bytes per max_keypoints rounded up to a power of two, and 16 bytes per
 *       grid cell where the grid has more than 1536 cells (1241 x 376, max_batch = 256, max_keypoints = 8192: 512 MB).  A
 *       context that never selects it allocates and pays nothing.
 *   svo_get_lk_detector : what is set (max_corners, quality_level, min_distance 0 while the detector is FAST).  Any pointer may
 *       be NULL.
 *   svo_min_eigen_map (stage API): steps 1-5 of one width x height image (1..16384 each), independent of the context's frame
 *       size and mode.  `mem` says where img AND out live; SVO_MEM_DEVICE: in stream order on the context's stream, no host
 *       synchronisation; SVO_MEM_HOST: returns when out is complete.  Floats of an out row beyond width are not written.
 *   svo_gftt_detect (stage API): steps 1-10.  `mem` says where img, out, strength AND n_out live.  out receives the records,
 *       strength (may be NULL) the eigenvalue of each, *n_out the count.  More candidates (step 7) than cap: nothing is listed
 *       and *n_out is the candidate count; SVO_MEM_HOST returns SVO_ERR_ARG then (SVO_MEM_DEVICE cannot know: compare *n_out
 *       with cap).  Device scratch grows on demand (a call that grows it waits for the device). */
#define SVO_DETECTOR_FAST 0
#define SVO_DETECTOR_GFTT 1
int svo_set_lk_detector(svo_ctx *ctx, int detector, int max_corners, double quality_level, double min_distance);
int svo_get_lk_detector(const svo_ctx *ctx, int *detector, int *max_corners, double *quality_level, double *min_distance);
int svo_min_eigen_map(svo_ctx *ctx, const uint8_t *img, int width, int height, int pitch, int mem, float *out, int out_pitch_floats);
int svo_gftt_detect(svo_ctx *ctx, const uint8_t *img, int width, int height, int pitch, int mem,
                    int max_corners, double quality_level, double min_distance,
                    svo_keypoint *out, float *strength, int cap, int *n_out);

/* ---- robust two-view pose refinement after solvePnPRansac (additive; detected by symbol, the ABI version stays 9 and
 * svo_config / svo_step_result are unchanged) -------------------------------------------------------------------------------
 * The stage the reference's author prepared and never finished: Tracking::G2O_EstimatePose_PnP (src/tracking.cpp:384-426,
 * include/lzb_vio/tracking.h:82; g2o found and linked at CMakeLists.txt:31,54, the body a copy of the OpenCV one, never
 * called).  A motion-only bundle adjustment in the style of ORB-SLAM2's PoseOptimization: robust (Huber) Levenberg-Marquardt
 * rounds on the reprojection error of BOTH cameras' observations at t2, a chi-square re-classification of the inliers after
 * every round, and the 6 x 6 information matrix of the pose.  Off by default; with it off every record is byte for byte what
 * it was.
 *
 * Arithmetic, all in double (the numpy twin is tests/_refine_ref.py):
 *   R1 views.  View L projects with [K1 | 0], K1 = (fx, fy, cx, cy) taken from P1 as the PnP stage takes it (skew and 4th
 *      column ignored); view R with the full 3 x 4 P2.  LK mode uses both (d = 4 residuals per point), ORB mode view L only
 *      (d = 2; its t2_right is zeros and is not read); the stage call uses d = 4 when img_right is given, else d = 2.
 *   R2 state (R, t), Y = R X + t; update (R, t) <- exp(xi) (R, t), xi = (rho, phi), closed-form SO(3) / SE(3) exponentials
 *      (series form below |phi| < 1e-10).  The start is the PnP record's R, t.
 *   R3 r_i stacks pi(P_v [Y; 1]) - x_v over the views; with M = P_v[:, :3], h = M Y + p4, u = h0 / h2, w = h1 / h2:
 *      du/dY = (M0 - u M2) / h2, dw/dY = (M1 - w M2) / h2, dY/dxi = [I | -[Y]x].  A point is projectable when h2 > 1e-6 in
 *      every view used; a point that is not has weight 0 and is never an inlier.
 *   R4 c_i = |r_i|^2 / sigma^2; tau = 5.991 (d = 2) or 9.488 (d = 4), the chi-square 95 % points.
 *   R5 `rounds` rounds of at most `iters` LM iterations.  The active set starts as ALL projectable points, not RANSAC's
 *      inliers.  Rounds 0 and 1: Huber IRLS on the active set, w_i = 1 if c_i <= tau else sqrt(tau / c_i), cost = sum of c_i
 *      or 2 sqrt(tau c_i) - tau; later rounds w_i = 1, cost = sum c_i.  After each round every projectable point is
 *      re-classified: active iff c_i <= tau (re-admission allowed).  The estimate carries over between rounds.
 *   R6 H = sum w_i J_i^T J_i / sigma^2, g = sum w_i J_i^T r_i / sigma^2; (H + lambda diag H) xi = -g by 6 x 6 Cholesky (fails
 *      unless every pivot is > 0); lambda = 1e-4 at the start of each round.  Accepted when the round's cost decreases (the
 *      cost is summed without rounding loss and compared as a (sum, remainder) pair: the decision does not depend on the order
 *      of the additions) and no active point becomes non-projectable: lambda <- max(lambda / 10, 1e-12), the round ends if |xi| < 1e-10.  Rejected
 *      otherwise or when the factorisation fails: lambda <- 10 lambda, the round ends if lambda > 1e10.  A rejected step
 *      counts as an iteration.
 *   R7 after the last re-classification info = sum over the active points of J_i^T J_i / sigma^2 at the final pose.  The
 *      refined pose replaces the PnP pose iff the active count >= min_inliers, info is positive definite (its Cholesky
 *      factorisation succeeds) and every output is finite: status SVO_REFINE_APPLIED.  Otherwise SVO_REFINE_KEPT_PNP and the
 *      PnP pose stands.  A pair whose solvePnPRansac failed is not refined: SVO_REFINE_SKIPPED.
 * svo_refine_result: rvec / tvec / R the pose that stands (refined or PnP's), pnp_rvec / pnp_tvec the PnP pose it started
 *   from, info row-major 6 x 6 in the order of xi (translation first), cost_first / cost_last the cost at the start of round 0
 *   and at the end of the last round (each in its round's own measure), n_points the points handed in, n_active the active
 *   count after the last re-classification, iters the LM iterations run (rejected ones included; depends on rounding at
 *   convergence -- report it, do not compare it), views 1 or 2.
 *   svo_set_pose_refine : every fused entry point (svo_add_frame, svo_track_batch, svo_track_uploaded(_async),
 *       svo_streams_step and their svo_ingest_* twins) then runs pose_refine_kernel between solvePnPRansac and the gates, on the
 *       pose stage's stream: the gates, T_rel_inv and the pose chain see the refined pose; n_inliers, ransac_iters, lm_iters
 *       and the RANSAC mask stay RANSAC's.  SVO_ERR_ARG (nothing changes): mode not OFF / REPROJ, rounds outside 1..16, iters
 *       outside 1..100, sigma_px not finite or <= 0, min_inliers < 1.  The first call that enables the stage (or the first
 *       svo_refine_pose) allocates ONE device block -- (max_batch + 1) records of 496 bytes + (max_batch + 1) x max_keypoints
 *       flag bytes + 28 bytes x max_keypoints of stage-call scratch (256 pairs x 8192 points: 2.3 MB) -- and waits for the
 *       device; a context that never enables it allocates nothing.
 *   svo_get_pose_refine : what is set.  Any pointer may be NULL.
 *   svo_refine_pose (stage API): the same kernel on a caller's points (n <= max_keypoints), with the CURRENT settings even
 *       while the mode is OFF.  obj, img_left, img_right and active follow `mem`; res is a HOST struct; the call returns when
 *       it is filled.  The start pose is (Rodrigues(rvec0), tvec0); pnp_rvec / pnp_tvec return them bit for bit.
 *   svo_get_refine_result : the record and the active flags of pair `pair` of the most recent fused launch, addressed as
 *       svo_get_batch_tracks addresses pairs (svo_add_frame: pair 0 is the last step; svo_streams_step: the item index);
 *       waits for that launch's pose stage.  HOST pointers; *n_out = n_points; SVO_ERR_ARG when the stage was off for that
 *       launch, pair is out of range or cap < n_points (active may be NULL: cap is ignored).  A capacity that is too small
 *       leaves *res and active untouched and still sets *n_out, the size to come back with. */
#define SVO_REFINE_OFF    0
#define SVO_REFINE_REPROJ 1
#define SVO_REFINE_BA     2     /* two-frame stereo bundle adjustment: the block below; selected by svo_set_pose_refine_ba */
#define SVO_REFINE_APPLIED  0
#define SVO_REFINE_KEPT_PNP 1
#define SVO_REFINE_SKIPPED  2
typedef struct {
    double rvec[3], tvec[3], R[9];
    double pnp_rvec[3], pnp_tvec[3];
    double info[36];
    double cost_first, cost_last;
    int32_t n_points, n_active, iters, views, status, _pad;
} svo_refine_result;
int svo_set_pose_refine(svo_ctx *ctx, int mode, int rounds, int iters, double sigma_px, int min_inliers);
int svo_get_pose_refine(const svo_ctx *ctx, int *mode, int *rounds, int *iters, double *sigma_px, int *min_inliers);
int svo_refine_pose(svo_ctx *ctx, const svo_pt3f *obj, const svo_pt2f *img_left, const svo_pt2f *img_right, int n,
                    const double P1[12], const double P2[12], const double rvec0[3], const double tvec0[3],
                    svo_refine_result *res, uint8_t *active, int mem);
int svo_get_refine_result(svo_ctx *ctx, int pair, svo_refine_result *res, uint8_t *active, int cap, int *n_out);

/* ---- two-frame stereo bundle adjustment: the refinement stage's second mode (additive; detected by symbol, the ABI version
 * stays 9 and svo_config / svo_step_result / svo_refine_result are unchanged) -------------------------------------------------
 * SVO_REFINE_REPROJ treats the triangulated t1 points as exact.  They are not: they are the float32 triangulation of noisy t1
 * tracks.  SVO_REFINE_BA is the maximum-likelihood estimator for a stereo pair of pairs instead: it minimises the
 * reprojection error in all four images over the pose AND the points.  Every pair stays independent; OFF and REPROJ are byte
 * for byte what they were.  rounds / iters / sigma_px / min_inliers keep their meaning and their ranges.
 *
 * Arithmetic, all in double (the numpy twin is tests/_ba_ref.py); R1-R7 are the rules above:
 *   unknowns  the pose (R, t) of R2, started at the PnP record, and one X_i per point, started at (double) of the triangulated
 *      float32 point.
 *   views     as R1.  At t1 both views project X_i, at t2 they project Y_i = R X_i + t.  LK mode: four observations, d = 8
 *      residuals per point (t1_left, t1_right, t2_left, t2_right).  ORB mode (both matchers): t1_left, t1_right, t2_left,
 *      d = 6; its t2_right is not read.  svo_refine_ba: d = 8 when img2_right is given, else d = 6.  A point is projectable
 *      when h2 > 1e-6 in every view used, at both times; otherwise its weight is 0, it is never active and it is never moved.
 *   cost      c_i = |r_i|^2 / sigma^2; tau = 11.070 (d = 8) or 7.815 (d = 6): the chi-square 95 % points for d - 3 degrees of
 *      freedom, three being absorbed by the point.
 *   rounds    exactly R5 (Huber in rounds 0 and 1, plain afterwards, every projectable point re-classified after each round,
 *      the estimate carried over).  A point that a re-classification leaves inactive returns to its triangulation: its
 *      position means nothing by then (a gross outlier wanders off under the Huber weight), and a later re-admission is
 *      judged on the triangulated point.
 *   one LM iteration.  Per active point, with J_x (d x 3: the t1 rows du/dX, the t2 rows (du/dY) R) and J_p (the t2 rows only,
 *      (du/dY) [I | -[Y]x]), weighted by w_i / sigma^2: V = J_x^T J_x, W = J_p^T J_x, U = J_p^T J_p, g_x = J_x^T r, g_p = J_p^T r;
 *      V* = V + lambda diag V is factored by a 3 x 3 Cholesky; if a pivot is <= 0 the point contributes U, g_p only and is not
 *      moved in this step.  Reduced system: H = sum (U - W V*^-1 W^T), g = sum (g_p - W V*^-1 g_x);
 *      (H + lambda diag sum U) xi = -g by the 6 x 6 Cholesky of R6; dX_i = -V*^-1 (g_x + W^T xi).  The trial pose and all
 *      trial points are accepted or rejected together by R6's test (the cost a (sum, remainder) pair; no active point may
 *      become non-projectable); lambda's schedule and the exits are R6's, the short-step exit being |xi| < 1e-10 and
 *      max |dX_i| < 1e-9 (Euclidean norm).
 *   outcome   as R7, with info = the reduced H at lambda = 0 over the active points at the final estimate: the pose's marginal
 *      information, the uncertainty of the structure included.  Same APPLIED / KEPT_PNP / SKIPPED rules; the PnP record's rvec /
 *      tvec / R are overwritten when applied; n_inliers, ransac_iters, lm_iters and the RANSAC mask stay RANSAC's.  When the
 *      PnP pose is kept the points that stand are the triangulated ones.  svo_refine_result.views is the number of t2 views.
 *   svo_set_pose_refine_ba : selects the mode, with svo_set_pose_refine's other arguments, ranges and errors;
 *       svo_get_pose_refine then reports mode SVO_REFINE_BA, and svo_set_pose_refine(OFF or REPROJ) leaves it.  The mode has a
 *       setter of its own because svo_set_pose_refine's contract is to refuse every mode but OFF and REPROJ, and it still
 *       does.  Every fused entry point then runs pose_ba_kernel where it would run
 *       pose_refine_kernel.  The first call that selects the mode (or the first svo_refine_ba) allocates, beside the stage's
 *       block, 48 bytes x (max_batch + 1) x max_keypoints + 16 bytes x max_keypoints (two buffers of double points per pair,
 *       stage-call scratch; 256 pairs x 8192 points: 101 MB) and waits for the device; a context that never does allocates
 *       nothing.  svo_get_refine_result works unchanged.
 *   svo_refine_ba (stage API): the same kernel on a caller's points (n <= max_keypoints) with the CURRENT settings, whatever
 *       the mode.  obj, img*, active and X_out (n x 3 doubles, the points that stand; may be NULL) follow `mem`; img2_right may
 *       be NULL (d = 6); res is a HOST struct.  The start pose is (Rodrigues(rvec0), tvec0).
 *   svo_get_refine_points : the points that stand of pair `pair` of the most recent fused launch, addressed as
 *       svo_get_refine_result addresses pairs; HOST pointer, *n_out = n_points.  SVO_ERR_ARG unless that launch ran in
 *       SVO_REFINE_BA mode, when pair is out of range or cap < n_points (X may be NULL: cap is ignored; *n_out is still set). */
int svo_set_pose_refine_ba(svo_ctx *ctx, int rounds, int iters, double sigma_px, int min_inliers);
int svo_refine_ba(svo_ctx *ctx, const svo_pt3f *obj, const svo_pt2f *img1_left, const svo_pt2f *img1_right,
                  const svo_pt2f *img2_left, const svo_pt2f *img2_right /* may be NULL */, int n, const double P1[12],
                  const double P2[12], const double rvec0[3], const double tvec0[3], svo_refine_result *res, uint8_t *active,
                  double *X_out /* n x 3 doubles, may be NULL */, int mem);
int svo_get_refine_points(svo_ctx *ctx, int pair, double *X, int cap, int *n_out);

/* ---- guided ORB matcher: epipolar stereo and sub-pixel refinement (additive; detected by symbol, the ABI version stays 9 and
 * svo_config / svo_step_result are unchanged) -------------------------------------------------------------------------------
 * The reference matches its ORB features by global brute force (Tracking::ORB_Robust_Find_MuliImage_MatchedFeatures); the
 * extractor it carries comes from ORB-SLAM2, whose own matcher (Frame::ComputeStereoMatches) searches the epipolar row band,
 * refines the disparity by an 11 x 11 SAD slide with a parabola fit and cuts outliers by the median SAD.  This is that matcher
 * plus a temporal ratio-test match with a sub-pixel step, as a second ORB-mode matcher.  Off by default; with it off every
 * record is byte for byte what it was.
 *
 * Arithmetic (restated from memory of ORB-SLAM2 and simplified where said, unpinned; every choice is listed in DESIGN.md
 * section 2; the numpy twin is tests/_orbmatch_ref.py).  float32 with one rounding per operation.  scale[l] is the extractor's
 * mvScaleFactor[l] (scale[0] = 1, scale[l] = float(scale[l-1] * double(orb_scale_factor))), inv[l] = 1.0f / scale[l];
 * rnd(x) = (int)floorf(x + 0.5f); I_l is the UNBLURRED pyramid level l (what svo_orb_read_level returns), w_l x h_l; Hamming
 * distances are integers over the 32 descriptor bytes.
 *   Patch of a left keypoint i: o = octave, (pu, pv) = (rnd(x*inv[o]), rnd(y*inv[o])); valid iff 5 <= pu < w_o - 5 and
 *      5 <= pv < h_o - 5.  T_i[dy][dx] = I_o[pv+dy][pu+dx] - I_o[pv][pu] (integers, dx, dy in [-5, 5]);
 *      SAD(T, J, cu, cv) = sum |T[dy][dx] - (J[cv+dy][cu+dx] - J[cv][cu])|.  The 121 raw bytes are stored per left keypoint
 *      (128-byte records) when the frame is ingested: ORB mode carries no pyramid from step to step.
 *   Stage S (stereo, once per frame at ingest).  maxD = max_disparity, 0 meaning (float)P1[0].
 *   S1 right keypoint j is a candidate of left keypoint i (uL, vL, oL) iff floorf(y_j - r_j) <= truncf(vL) <= ceilf(y_j + r_j)
 *      with r_j = 2.0f*scale[octave_j], |octave_j - oL| <= 1 and uL - maxD <= x_j <= uL.
 *   S2 the smallest Hamming distance among the candidates, ties to the lowest j; reject i when there is none or
 *      best >= th_stereo.
 *   S3 slide: sr = rnd(x_j*inv[oL]), J = the right image's I_oL; reject when the patch is invalid, sr - 10 < 0 or
 *      sr + 11 >= w_oL; d[k] = SAD(T_i, J, sr + k, pv), k = -5..5; kb = the first minimum; reject when kb = +-5.
 *   S4 parabola: d1, d2, d3 = (float)d[kb-1], d[kb], d[kb+1]; den = 2.0f*((d1 + d3) - 2.0f*d2); delta = den == 0 ? 0 :
 *      (d1 - d3)/den; uR = scale[oL]*(((float)sr + (float)kb) + delta); disp = uL - uR; accept iff 0 <= disp < maxD; when
 *      disp <= 0, uR = uL - 0.01f.
 *   S5 median cut over the accepted keypoints of the frame: med = element n/2 of their SADs in ascending order; those with
 *      (float)sad >= (1.5f*1.4f)*(float)med are dropped.
 *   S6 per left keypoint: uR[i] (-1.0f: none) and sad[i] (-1: none); the right-image point of a stereo match is (uR[i], y_i).
 *   Stage T (temporal, per pair: last frame -> current frame, left images).
 *   T1 for each last-left i with uR[i] >= 0, current-left j is a candidate iff |octave_j - octave_i| <= 1 and, when
 *      radius > 0, |x_j - x_i| <= radius and |y_j - y_i| <= radius (radius 0: the whole image).  b / s = the smallest / second
 *      smallest distance over the candidates, ties to the lowest j; keep iff b <= th_track and (there is no second candidate
 *      or (float)b < ratio*(float)s).
 *   T2 uniqueness: of several i that keep the same j, the smallest b wins, ties to the lowest i.
 *   T3 sub-pixel step: o = octave_i, (cu, cv) = (rnd(x_j*inv[o]), rnd(y_j*inv[o])), J = the current-left I_o; reject unless
 *      7 <= cu < w_o - 7 and 7 <= cv < h_o - 7; D[dy][dx] = SAD(T_i, J, cu+dx, cv+dy), dx, dy in [-2, 2]; (by, bx) = the
 *      first minimum in raster order; reject when it lies on the 5 x 5 border; the S4 parabola along each axis through the
 *      minimum; t2 = (scale[o]*(((float)cu + (float)bx) + dx'), scale[o]*(((float)cv + (float)by) + dy')).
 *   T4 emitted in ascending i: t1_left = (x_i, y_i), t1_right = (uR[i], y_i), t2_left = t2 -- the lists the brute matcher
 *      writes.  Triangulation, solvePnPRansac, the refinement stage, the gates and SVO_FAIL_FEW_TRACKS
 *      (n_tracked < num_features_tracking) are untouched.
 *   svo_set_orb_matcher : ORB mode.  Applies to frames ingested by LATER calls on every fused entry point.  A frame stored
 *       from before the switch to SVO_ORB_MATCHER_GUIDED (svo_add_frame's previous frame, a stream's stored frame, a carried
 *       frame) has no patches and no stereo matches: its first pair ends as SVO_FAIL_FEW_TRACKS with n_tracked = 0, the next
 *       pair is a regular one.  SVO_ERR_ARG (nothing changes): an LK-mode context; an unknown mode; th_stereo or th_track
 *       outside 1..256; ratio outside (0, 1]; radius or max_disparity negative or not finite.  Memory: allocated by the first
 *       call that selects SVO_ORB_MATCHER_GUIDED (or the first stage call), with cap = max_keypoints rounded up to 4: per
 *       working frame (max_batch + 1 of them) and per stream of a stream set 16 + 136*cap bytes (the 128-byte patch, uR and
 *       sad per keypoint), and 20*cap bytes per pair of max_batch (max_batch = 256, max_keypoints = 8192: 273 MB + 40 MB;
 *       max_keypoints = 2048: 68 MB + 10 MB; 1 MB = 2^20 bytes).  A context that never selects it allocates and pays nothing.
 *   svo_get_orb_matcher : what is set.  Any pointer may be NULL.
 *   svo_orb_stereo_frame (stage API): extracts both images (HOST or DEVICE, one pitch) into stage slot `slot` in {0, 1} -- frame
 *       slots 0 / 1 of the context: the online ring and a carried frame do not survive -- and runs stage S with the current
 *       settings.  kps / uR / sad (HOST, each may be NULL) receive the left keypoints and S6, *n_out the count;
 *       SVO_ERR_ARG when cap is too small.
 *   svo_orb_track_frames (stage API): stage T from stage slot slot_prev to slot_cur (both filled by svo_orb_stereo_frame).
 *       HOST outputs, each may be NULL: the three point lists and the keypoint indices of every track; *n_out the count.
 *   svo_get_frame_stereo : S6 of the current frame of svo_add_frame (the left keypoints: svo_get_frame_keypoints). */
#define SVO_ORB_MATCHER_BRUTE  0
#define SVO_ORB_MATCHER_GUIDED 1
int svo_set_orb_matcher(svo_ctx *ctx, int mode, int th_stereo, int th_track, double ratio, double radius, double max_disparity);
int svo_get_orb_matcher(const svo_ctx *ctx, int *mode, int *th_stereo, int *th_track, double *ratio, double *radius, double *max_disparity);
int svo_orb_stereo_frame(svo_ctx *ctx, const uint8_t *left, const uint8_t *right, int pitch, int mem, int slot,
                         svo_keypoint *kps, float *uR, int32_t *sad, int cap, int *n_out);
int svo_orb_track_frames(svo_ctx *ctx, int slot_prev, int slot_cur, svo_pt2f *t1_left, svo_pt2f *t1_right, svo_pt2f *t2_left,
                         int32_t *idx_prev, int32_t *idx_cur, int cap, int *n_out);
int svo_get_frame_stereo(svo_ctx *ctx, float *uR, int32_t *sad, int cap, int *n_out);

/* ---- Track carry: LK tracks kept across frames under persistent ids, on the online paths (additive; detected by symbol, the
 * ABI version stays 9 and svo_config is unchanged) ---------------------------------------------------------------------------
 * By default every frame's corners are detected afresh and tracked through exactly one pair (src/tracking.cpp:258-344).  With
 * track carry on, the list a frame hands to the next pair is the points the circular LK has just tracked INTO it, each under
 * the id it already had, followed by those of the frame's detections that do not crowd them.  A back end gets the same
 * physical point over many frames under one id; the odometry chain tracks from sub-pixel positions.
 *
 * Semantics (the numpy twin is tests/_carry_ref.py; the kernel equals it bit for bit).  A frame's list is up to max_keypoints
 * entries (xy float32 x 2, response, id int64, age int32).  Inputs of a pair: the previous frame's list Lp (n_p entries); the
 * new frame's detections D (n_d entries, in the order the detector chain leaves them); per i < n_p the keep byte of the
 * circular LK and q[i] = its t2_left.
 *   C1 candidates: ascending i with keep[i] != 0, q[i] finite, 0 <= q.x <= w-1 and 0 <= q.y <= h-1 (float compares), and
 *      max_age == 0 or age[i] + 1 <= max_age.
 *   C2 near(a, b): dx = a.x - b.x, dy = a.y - b.y in float32 (one rounding each); d2 = (double)dx*dx + (double)dy*dy (the
 *      products are exact, the sum is the only rounding); near iff d2 < min_distance * min_distance in double.
 *   C3 carried: candidate i is carried iff no candidate j < i is near it -- every earlier candidate counts, carried itself or
 *      not.  The rule depends on indices only (it evaluates in parallel) and list order is seniority order: the older track
 *      wins.  It drops a little more than a greedy pass would.
 *   C4 detections: detection k is kept iff no CARRIED point is near it.  Detections are not tested against each other.
 *   C5 the new list: the carried points in ascending i as (q[i], response[i], id[i], age[i] + 1), then the kept detections in
 *      ascending k as (xy, response, id = next_id + rank, age 0), cut at max_keypoints: only trailing detections fall off, and
 *      they get no id.  next_id advances by the number of detections listed.  This list is what the next pair tracks from and
 *      what svo_get_frame_keypoints returns (x, y: the tracked sub-pixel position; the other fields as the detector made them).
 *   C6 a list without ids -- a chain's first frame, the first frame after a reset, a frame stored before the switch -- is
 *      numbered next_id.. in list order, age 0, by the step that first sees it.  ids start at 0 per stream and per online
 *      chain; svo_reset / svo_streams_reset restart them.
 *   C7 an image whose detector count exceeds max_keypoints contributes no detections.  Its pair ends in SVO_FAIL_CAPACITY as
 *      without carry; the following pair tracks the carried points and is a regular pair.
 *   C8 the carry happens whatever the step's outcome (the reference replaces last_frame_ on every exit).  n_prev_kps = the
 *      length of Lp; n_cur_kps and the < 30 gate stay the detector's count.
 *   svo_set_track_carry : LK mode; svo_add_frame, svo_streams_step and their svo_ingest_* twins.  on = 0 (the default): off, the
 *       other arguments are ignored, and every step runs exactly the launches it ran before this option existed.
 *       Recommended when on: min_distance 3.0, max_age 0 (unlimited).  May be called at any time between calls on the
 *       context.  While on, svo_track_batch, svo_track_uploaded(_async) and svo_ingest_track_batch return SVO_ERR_STATE: a
 *       batch treats its pairs as independent.  SVO_ERR_ARG (nothing changes): an ORB-mode context; min_distance not finite,
 *       < 1 or > 256; max_age < 0.  Memory: allocated by the first enabling call -- 12 bytes x max_keypoints per working frame
 *       (max_batch + 1) and per stream of an existing stream set, 30 bytes x max_keypoints per pair of max_batch; a stream set
 *       created afterwards includes its share.  A context that never enables it allocates and pays nothing.  The id counters
 *       live on the device (one for the online ring, one per stream): no host synchronisation is added to a step.
 *   svo_get_track_carry : what is set (0, 0.0, 0 while off).  Any pointer may be NULL.
 *   svo_carry_merge (stage API): the same kernel on a caller's arrays, independent of the context's size and mode.  Tracks:
 *       trk_xy = q, trk_resp / trk_id / trk_age / trk_keep, n_trk entries; detections det_xy / det_resp, n_det entries; next_id.
 *       Outputs, cap >= n_trk entries each: the list (out_xy, out_resp, out_id, out_age), out_src = the track index or n_trk +
 *       the detection index of every entry, *n_out the length, *n_carried the carried points.  `mem` says where every array AND
 *       the two counts live; SVO_MEM_DEVICE: in stream order on the context's stream, no host synchronisation (scratch grows
 *       on demand; a call that grows it waits for the device), inputs and outputs must not overlap; SVO_MEM_HOST: returns when
 *       the outputs are complete.  SVO_ERR_ARG: a size < 1 or > 16384, the parameter rules above, cap < n_trk, n > 2^20.
 *   Read-backs (HOST).  ids / ages NULL (both): *n_out only; otherwise SVO_ERR_ARG when cap is too small.  SVO_ERR_ARG when
 *   track carry was off for the step in question.
 *       svo_get_frame_track_ids      : ids and ages of the list svo_get_frame_keypoints returns.
 *       svo_get_last_track_ids       : id and age at t1 of every track of svo_get_last_tracks, in its order.
 *       svo_streams_get_track_ids    : the same for item `item` of the last svo_streams_step (svo_streams_get_tracks).
 *       svo_streams_get_frame_tracks : a stream's stored list: records as svo_get_frame_keypoints makes them, ids, ages. */
int svo_set_track_carry(svo_ctx *ctx, int on, double min_distance, int max_age);
int svo_get_track_carry(const svo_ctx *ctx, int *on, double *min_distance, int *max_age);
int svo_carry_merge(svo_ctx *ctx, int width, int height, double min_distance, int max_age,
                    const svo_pt2f *trk_xy, const float *trk_resp, const int64_t *trk_id, const int32_t *trk_age,
                    const uint8_t *trk_keep, int n_trk, const svo_pt2f *det_xy, const float *det_resp, int n_det, int64_t next_id,
                    svo_pt2f *out_xy, float *out_resp, int64_t *out_id, int32_t *out_age, int32_t *out_src, int cap,
                    int *n_out, int *n_carried, int mem);
int svo_get_frame_track_ids(svo_ctx *ctx, int64_t *ids, int32_t *ages, int cap, int *n_out);
int svo_get_last_track_ids(svo_ctx *ctx, int64_t *ids, int32_t *ages, int cap, int *n_out);
int svo_streams_get_track_ids(svo_ctx *ctx, int item, int64_t *ids, int32_t *ages, int cap, int *n_out);
int svo_streams_get_frame_tracks(svo_ctx *ctx, int stream_id, svo_keypoint *kps, int64_t *ids, int32_t *ages, int cap, int *n_out);

/* ---- Sliding window: the landmark table over carried tracks (additive; detected by symbol, the ABI version stays 9 and
 * svo_config is unchanged) ------------------------------------------------------------------------------------------------
 * Track carry gives one physical point one id over many frames.  The table below is the store a fixed-lag back end needs on
 * top of that: the last W <= SVO_WINDOW_MAX_FRAMES frames of a chain and, per id, one world point with the stereo observation
 * of every frame of the window that saw it.  svo_window_update is the stage call that moves a table on by one tracked pair;
 * nothing in a context's fused steps uses it yet.
 *
 * A table (svo_window_table) is `cap` rows of room plus
 *   counts    int32[4]: n frames (0..W; slot 0 oldest, slot n-1 newest), m rows, the rows the last update needed, 0
 *   poses     double[SVO_WINDOW_MAX_FRAMES][12]: per slot the camera-from-world pose, R row-major then t (Y = R X + t);
 *             slots >= n are 0
 *   ids       int64[m], strictly ascending            X       double[m][3], world
 *   seen      uint32[m], bit s = slot s has an observation of the row
 *   active    uint32[m], bit s = the back end's last verdict on that observation (the update only moves it; new observations
 *             enter with the bit clear)
 *   obs_left / obs_right   svo_pt2f[m][SVO_WINDOW_MAX_FRAMES]; columns without a seen bit are 0
 * Rules (the numpy twin is tests/_window_ref.py; the kernel equals it bit for bit in counts, ids, masks and observations, and
 * to 1e-12 relative in poses and X).  One call = one step with ok = 1 on pair a -> b; pose_a is the chain pose before the step
 * (frame a, world from camera, 4 x 4 row-major as svo_get_pose returns it), pose_b the step record's pose.
 *   T1 a cleared table is n = m = 0.  The caller clears: on a chain's first frame, after a failed step, a reset or a re-seeded pose.
 *   T2 n = 0: slot 0 becomes frame a with pose inverse(pose_a); rows of the input are ignored.
 *   T3 n = W: slide -- slot 0 leaves; seen, active and the observation columns move down by one (the top column is 0); rows
 *      whose seen is now 0 leave, the others keep their order.
 *   T4 frame b becomes the newest slot with pose inverse(pose_b).  inverse(T): R = Rw^T, t_i = -((R_i0 tw_0 + R_i1 tw_1) +
 *      R_i2 tw_2), in double.
 *   T5 for every track of the pair -- in the order svo_get_last_tracks lists them, which by rule C5 is ascending id -- that is
 *      usable (t1_left, t1_right, t2_left, t2_right and the float32 triangulated point all finite): the newest slot gets
 *      (t2_left, t2_right); the slot before it gets (t1_left, t1_right) unless its seen bit is already set; an id without a
 *      row creates one with X_j = (Ra_0j d_0 + Ra_1j d_1) + Ra_2j d_2, d = (double)X_tri - ta, (Ra, ta) = slot a's pose.
 *   T6 the result is the merge of the two id-sorted lists: a usable track whose row was never made (its triangulation was not
 *      finite earlier) or has left enters at its id's place.
 *   T7 the update needs (surviving rows + new rows) <= cap.  A chain whose pairs have at most K tracks never needs more than
 *      (W - 1) x K.  When cap is too small NOTHING of `out` is written but counts = {0, 0, rows needed, 0} -- a cleared table.
 *   svo_window_update: independent of the context's size and mode.  `frames` = W, 2..SVO_WINDOW_MAX_FRAMES.  `in` and `out`
 *       both have `cap` rows of room and must not overlap; `in` is not written.  ids must be strictly ascending (unspecified
 *       rows, but no access outside the arrays, otherwise).  `mem` says where every array, both poses and the counts live
 *       (the two svo_window_table structs themselves are host memory).  SVO_MEM_DEVICE: one launch in stream order on the
 *       context's stream, no host synchronisation (scratch grows on demand; a call that grows it waits for the device); a
 *       short cap shows in out->counts[2] > cap.  SVO_MEM_HOST: returns when `out` is complete; SVO_ERR_ARG when cap was too
 *       small (out->counts is set as above).  SVO_ERR_ARG also: frames out of range, cap < 1 or > 2^21, n_trk < 0 or > 2^20,
 *       a null pointer, and (HOST) input counts outside 0..frames / 0..cap.
 *
 * The optimiser over a table: a sliding-window stereo bundle adjustment, the two-frame SVO_REFINE_BA generalised to n <= 8
 * frames.  All arithmetic in double; R1-R7 are the rules of the refinement stage above; the numpy twin is solve() of
 * tests/_window_ref.py (the kernel agrees with it in status, masks and counts, and to 1e-9 in poses, X and info).
 *   W1 slot 0 is fixed (the gauge; stereo fixes the scale).  Unknowns: xi_f for slots 1..n-1 (R2's update on the slot's
 *      camera-from-world pose) and X_i per usable landmark.
 *   W2 observation (i, f) -- a seen bit -- has d = 4 residuals: view L [K1 | 0] and view R the full P2 of Y = R_f X_i + t_f, as
 *      R1 and R3 (K1 = fx, fy, cx, cy of P1).  It is projectable when h2 > 1e-6 in both views.  c = |r|^2 / sigma^2, tau = 9.488
 *      (the chi-square 95 % point for 4 degrees of freedom: the share of the landmark's three is spread over its observations
 *      and is not subtracted).
 *   W3 a landmark is usable in a round when >= 2 of its observations are active; otherwise it has no active observation, weighs
 *      nothing and is not moved.
 *   W4 rounds are R5's, per observation: rounds 0 and 1 Huber (w = 1 if c <= tau else sqrt(tau / c)), later rounds plain; the
 *      first round starts from all projectable seen observations; after each round every projectable seen observation is
 *      re-classified (active iff c <= tau, re-admission allowed); a landmark that falls below two active observations returns
 *      to the X it had at entry.
 *   W5 one LM iteration.  Per usable landmark over its active observations, weighted by w / sigma^2: V = sum J_x^T J_x, g_x,
 *      V* = V + lambda diag V = L L^T (3 x 3 Cholesky; a pivot <= 0: the landmark contributes U and g_p only and is not moved);
 *      per slot f >= 1: W_if = J_p^T J_x, U_f += J_p^T J_p, g_pf += J_p^T r, T_if = W_if L^-T, y_i = L^-1 g_x.  Reduced system
 *      of dimension 6 (n - 1) <= 42: H_ff' = delta_ff' sum U_f - sum_i T_if T_if'^T, g_f = sum (g_pf - T_if y_i);
 *      (H + lambda diag sum U) xi = -g by Cholesky, every pivot > 0; dX_i = -L^-T (y_i + sum_f T_if^T xi_f).  Slot 0's
 *      observations enter V and g_x only.
 *   W6 accept / reject as R6: the cost a (sum, remainder) pair; no active observation may become non-projectable; all poses and
 *      points are accepted or rejected together; lambda 1e-4 at the start of a round, / 10 (floor 1e-12) on accept, x 10 on
 *      reject or a failed factorisation, the round ends past 1e10; short-step exit |xi| < 1e-10 (the whole vector) and
 *      max |dX_i| < 1e-9.  A rejected step counts as an iteration.
 *   W7 after the last re-classification info = the reduced H at lambda = 0 over the active set at the final estimate.
 *      SVO_REFINE_APPLIED iff every slot 1..n-1 has >= min_obs active observations, info factors and everything (poses, points,
 *      info, cost_first, cost_last) is finite: then the table's poses, X and active are overwritten.  SVO_REFINE_KEPT_PNP
 *      otherwise: the table is left as it was, bit for bit.  SVO_REFINE_SKIPPED when n < 2.
 *   W8 the same input gives the same bytes on every run: sums run in a fixed order, there are no floating-point atomics.
 *   svo_window_result: status; n_frames, n_landmarks (rows); n_usable, n_active (landmarks / observations active after the last
 *      re-classification), n_obs (seen bits); iters (LM iterations run, rejected ones included); frame_active[8] per slot;
 *      cost_first / cost_last as svo_refine_result; info row-major 42 x 42, the leading 6 (n - 1) square in the order of xi
 *      (slot 1 first, translation first), the rest 0 -- also when the table is kept.
 *   svo_window_ba (stage API): window_ba_kernel on a caller's table, independent of the context's size and mode.  The table has
 *      `cap` rows of room (counts[1] <= cap); ids is not read.  P1, P2 are HOST pointers; rounds, iters, sigma_px keep
 *      svo_set_pose_refine's ranges, min_obs >= 1 (SVO_ERR_ARG otherwise).  `mem` says where the table's arrays, its counts
 *      and *res live.  SVO_MEM_DEVICE: one launch in stream order on the context's stream, the table updated in place, no host
 *      synchronisation (scratch -- 1140 bytes a row -- grows on demand; a call that grows it waits for the device).
 *      SVO_MEM_HOST: returns when *res and the table's poses, X and active are complete.
 *   svo_set_window_ba : LK mode, the online chain (svo_add_frame / svo_ingest_add_frame) with track carry on.  frames = 0 (the
 *      default) switches it off -- the other arguments are ignored and every step runs exactly the launches it ran before this
 *      option existed; frames 2..8 = W.  While on, every step with a previous frame runs window_update_kernel and
 *      window_ba_kernel after the gates and the pose chain, on the step's stream, before the record is delivered (timing marks
 *      win_update, win_ba); no host synchronisation is added.  The table is cleared (T1) by a chain's first frame, by a step
 *      whose record has ok = 0 (on the device), by svo_reset, svo_set_pose, svo_set_window_ba and svo_set_track_carry.  The
 *      pair's tracks are those of svo_get_last_tracks, their ids those of svo_get_last_track_ids, the triangulation the pose
 *      stage's.  SVO_REFINE_APPLIED: the step record's pose, and with it frame_pose_ (svo_get_pose), become inverse(newest
 *      slot); T_rel_inv, rvec, tvec, R, the counts and every track stay the pair's.  Otherwise the record is untouched.
 *      SVO_ERR_ARG (nothing changes): an ORB-mode context, frames not 0 or 2..8, rounds / iters / sigma_px outside
 *      svo_set_pose_refine's ranges, min_obs < 1.  SVO_ERR_STATE: track carry is off.  While it is on, svo_set_track_carry(off),
 *      svo_streams_step and svo_ingest_streams_step return SVO_ERR_STATE (stream sets have no table yet).  Memory: the first
 *      enabling call (and a later one with a larger W) allocates ONE block for (W - 1) x max_keypoints rows -- 2 tables of 168
 *      bytes a row and 1140 bytes a row of scratch -- and waits for the device; a context that never enables it allocates
 *      nothing.
 *   svo_get_window_ba : what is set (all 0 while off).  Any pointer may be NULL.
 *   svo_get_window : the online chain's table after the last svo_add_frame step, into HOST arrays with `cap` rows of room
 *      (counts first; every other pointer NULL: the counts only; SVO_ERR_ARG when counts[1] > cap).
 *   svo_get_window_result : that step's svo_window_result (SKIPPED after a failed step or with fewer than two frames).  Both
 *      return SVO_ERR_ARG when the window was off for the last step or no pair has been tracked.
 *   Host mirror: YAML window_ba: W with window_ba_rounds / _iters / _sigma / _min_obs. */
#define SVO_WINDOW_MAX_FRAMES 8
typedef struct {
    int32_t  *counts;
    double   *poses;
    int64_t  *ids;
    double   *X;
    uint32_t *seen, *active;
    svo_pt2f *obs_left, *obs_right;
} svo_window_table;
int svo_window_update(svo_ctx *ctx, int frames, const svo_window_table *in, const svo_window_table *out, int cap,
                      const svo_pt2f *t1_left, const svo_pt2f *t1_right, const svo_pt2f *t2_left, const svo_pt2f *t2_right,
                      const int64_t *ids, const svo_pt3f *tri, int n_trk, const double pose_a[16], const double pose_b[16], int mem);

typedef struct {
    int32_t status, n_frames, n_landmarks, n_usable, n_obs, n_active, iters, _pad;
    int32_t frame_active[SVO_WINDOW_MAX_FRAMES];
    double cost_first, cost_last;
    double info[42 * 42];
} svo_window_result;
int svo_set_window_ba(svo_ctx *ctx, int frames, int rounds, int iters, double sigma_px, int min_obs);
int svo_get_window_ba(const svo_ctx *ctx, int *frames, int *rounds, int *iters, double *sigma_px, int *min_obs);
int svo_get_window(svo_ctx *ctx, const svo_window_table *out, int cap);
int svo_get_window_result(svo_ctx *ctx, svo_window_result *res);
int svo_window_ba(svo_ctx *ctx, const svo_window_table *table, int cap, const double P1[12], const double P2[12], int rounds, int iters,
                  double sigma_px, int min_obs, svo_window_result *res, int mem);

/* ---- Keyframe-relative pose on the online chain over carried LK tracks (additive; detected by symbol, the ABI version stays 9
 * and svo_config / svo_step_result are unchanged) ---------------------------------------------------------------------------
 * Every pose the chain reports is a product of one relative motion per frame (frame_pose_ = frame_pose_ * T.inv(),
 * src/tracking.cpp:318).  With keyframe mode on, the current frame is ALSO localised by solvePnPRansac against 3-D points
 * triangulated once, at a keyframe several frames back, and where that solve is accepted its pose replaces the chained one:
 * error then accumulates per keyframe, and the baseline of a solve is longer.  Off by default; with it off every step runs
 * exactly the launches it ran before and every record is byte for byte what it was.
 *
 * State of a chain, on the device: valid; kf_index (the chain's frame counter at the keyframe; frames count from 0 at a
 * chain's first frame); pose_K (world from camera, 4 x 4 row-major) and inv_K (camera from world, rule T4's closed form);
 * n_rows; ids int64[n_rows], strictly ascending; X float32[n_rows][3] in the keyframe's camera frame.
 * Rules (the numpy twin is tests/_keyframe_ref.py; the kernels equal it bit for bit in every integer, list and table, and to
 * the chain's bar in poses).  One step is a pair a -> b.  Its record r is the record as the gates -- and the refinement stage,
 * if on -- leave it; its tracks are those of svo_get_last_tracks, their ids those of svo_get_last_track_ids (ascending, rule
 * C5); tri is the pose stage's float32 triangulation of (t1_left, t1_right), in a's camera frame; pose_a is the chain pose
 * before the step; index(b) is b's frame counter.
 *   K1 cleared.  The state becomes not valid on a chain's first frame and on svo_reset, svo_set_pose, svo_set_keyframe and
 *      svo_set_track_carry.  A failed step (r.ok = 0) does NOT clear it: the carry goes on whatever the outcome (C8) and the
 *      gap simply grows.
 *   K2 join.  With a valid state, for every track i in ascending order whose id has a row j, the joined lists gain
 *      (X[j], t2_left[i]) and the index pair (i, j); n_join is their length.  The result is the merge of two id-sorted lists
 *      and contains nothing else; ids compare as 64-bit integers.  With an invalid state n_join = 0.
 *   K3 solve.  With a valid state and n_join >= min_tracks: solvePnPRansac(joined X, joined t2_left) with the context's K,
 *      iterationsCount, reprojectionError and confidence -- exactly the pair's solve on other lists, from the same cv::RNG(-1)
 *      state -- gives [R t], X_b = R X_K + t.  Otherwise nothing is solved (n_inliers, ransac_iters, lm_iters, rvec, tvec are
 *      0) and the status is SVO_KF_SHORT, or SVO_KF_NONE with an invalid state.
 *   K4 accept.  SVO_KF_APPLIED iff r.ok = 1, the solve succeeded, (double)n_inliers / (double)n_join >= inlier_rate, and the
 *      motion a -> b that the keyframe pose implies passes the pair's own gates: F = ([R t; 0 0 0 1] inv_K) pose_a, both
 *      products in chain_relative's association order (k ascending, separate multiply and add, from 0); on F's rotation the
 *      three Euler angles of rotationMatrixToEulerAngles as the pair's gate computes them must each be below 0.1 in absolute
 *      value; on F's translation |t|^2 < max_move2 (t0 t0 + t1 t1 + t2 t2, left to right).  There is no lower bound: the pair
 *      has passed it.  Otherwise SVO_KF_REJECTED, or SVO_KF_PAIR_FAILED when r.ok = 0.
 *   K5 apply.  On APPLIED r.pose := pose_K inverse([R t]), the inverse in the closed form of T_rel_inv (R^T, -(R^T t) summed
 *      left to right), the product in the chain's order; frame_pose_ (svo_get_pose) follows.  T_rel_inv, rvec, tvec, R, every
 *      count, every track and the inlier mask stay the pair's.  With any other status the record is untouched, bit for bit.
 *   K6 switch.  After K5 and only when r.ok = 1: a new keyframe is taken iff the state is not valid, or the status is not
 *      APPLIED, or max_gap > 0 and gap >= max_gap, gap = index(b) - kf_index.  The new keyframe is frame a: kf_index =
 *      index(b) - 1, pose_K = pose_a, inv_K by T4; the table becomes this pair's tracks whose three tri floats are finite,
 *      in list order, as (id, tri).  Frame a because its stereo triangulation already exists; the step that switches reports
 *      the pair's own pose, and that pose IS the keyframe solution for K = a.  The smallest gap of a solve is therefore 2.
 *   K7 with r.ok = 0 the state keeps everything.  The join and the solve are still launched (no host decision is added) and
 *      reported; they are not used.
 *   K8 the same input gives the same bytes on every run: no floating-point atomics, the lists are in id order.
 *   svo_set_keyframe : LK mode, the online chain (svo_add_frame / svo_ingest_add_frame) with track carry on.  on = 0 (the
 *      default): off, the other arguments are ignored.  While on, every step with a previous frame runs keyframe_join_kernel,
 *      one solvePnPRansac on the joined lists (item 1 of the pose workspace) and keyframe_update_kernel after the gates and the
 *      pose chain, on the step's stream, before the record is delivered (timing marks kf_join, kf_pnp, kf_update); no host
 *      synchronisation is added.  max_gap = 0: no limit.  SVO_ERR_ARG (nothing changes): an ORB-mode context, min_tracks < 4
 *      or > max_keypoints, max_gap < 0 or = 1, max_batch < 2.  SVO_ERR_STATE: track carry is off, or the sliding window is on
 *      (both would rewrite `pose`).  While it is on, svo_set_window_ba(on), svo_set_track_carry(off), svo_streams_step and
 *      svo_ingest_streams_step return SVO_ERR_STATE (stream sets have no keyframe yet).  The refinement stage is independent:
 *      the pair's record is refined as before, the keyframe solve never is.  Memory: the first enabling call allocates ONE
 *      block -- 20 bytes x max_keypoints for the table, 36 bytes x max_keypoints for the joined lists, the state and the
 *      result -- and waits for the device; a context that never enables it allocates nothing.
 *   svo_get_keyframe : what is set (0, 0, 0 while off).  Any pointer may be NULL.
 *   svo_keyframe_result: status; switched (K6 took a new keyframe); kf_index, gap, n_rows and pose_K of the keyframe the step
 *      joined against (-1, 0, 0 and zeros when there was none); n_join; n_inliers, ransac_iters, lm_iters, rvec, tvec of the
 *      solve; pose_pair, the chained pair pose the record held before K5.
 *   Read-backs (HOST; they wait for the step).  SVO_ERR_ARG when keyframe mode was off for the last svo_add_frame step or no
 *   pair has been tracked.  Every list pointer NULL: *n_out only; otherwise SVO_ERR_ARG when cap is too small (*n_out is still
 *   set); a NULL list is left out.
 *      svo_get_keyframe_result  : the last step's svo_keyframe_result.
 *      svo_get_keyframe_matches : the joined lists -- id, X, t2_left, track index i, and the solve's inlier mask (zeros when
 *                                 nothing was solved) -- n_join entries each.
 *      svo_get_keyframe_table   : the table after the step (ids, X), n_rows entries.
 *   svo_keyframe_join (stage API): keyframe_join_kernel on a caller's arrays, independent of the context's size and mode.
 *      Table tab_ids / tab_X (n_rows x 3 floats), tracks trk_ids / trk_xy; both id lists strictly ascending (unspecified rows,
 *      but no access outside the arrays, otherwise).  Outputs, cap >= min(n_rows, n_trk) entries each: out_X, out_xy, out_trk
 *      (i), out_row (j), *n_out.  `mem` says where every array AND the count live; SVO_MEM_DEVICE: one launch in stream order
 *      on the context's stream, no host synchronisation, inputs and outputs must not overlap; SVO_MEM_HOST: returns when the
 *      outputs are complete (scratch grows on demand; a call that grows it waits for the device).  SVO_ERR_ARG: a count < 0 or
 *      > 2^20, a null pointer, cap < min(n_rows, n_trk).
 *   Host mirror: YAML keyframe: 0 | 1 with keyframe_max_gap; min_tracks is num_features_needed_for_keyframe. */
#define SVO_KF_NONE        0
#define SVO_KF_SHORT       1
#define SVO_KF_PAIR_FAILED 2
#define SVO_KF_REJECTED    3
#define SVO_KF_APPLIED     4
typedef struct {
    int32_t status, switched, kf_index, gap, n_rows, n_join, n_inliers, ransac_iters, lm_iters, _pad;
    double rvec[3], tvec[3];
    double pose_K[16], pose_pair[16];
} svo_keyframe_result;
int svo_set_keyframe(svo_ctx *ctx, int on, int min_tracks, int max_gap);
int svo_get_keyframe(const svo_ctx *ctx, int *on, int *min_tracks, int *max_gap);
int svo_get_keyframe_result(svo_ctx *ctx, svo_keyframe_result *res);
int svo_get_keyframe_matches(svo_ctx *ctx, int64_t *ids, svo_pt3f *X, svo_pt2f *xy, int32_t *trk_index, uint8_t *mask, int cap, int *n_out);
int svo_get_keyframe_table(svo_ctx *ctx, int64_t *ids, svo_pt3f *X, int cap, int *n_out);
int svo_keyframe_join(svo_ctx *ctx, const int64_t *tab_ids, const svo_pt3f *tab_X, int n_rows, const int64_t *trk_ids,
                      const svo_pt2f *trk_xy, int n_trk, svo_pt3f *out_X, svo_pt2f *out_xy, int32_t *out_trk, int32_t *out_row,
                      int cap, int *n_out, int mem);

/* Serial prefix product of n inverse relative motions (svo_step_result.T_rel_inv, row-major 4x4),
 * skipping pairs with ok == 0:  poses_out[p] = pose0 * prod_{q <= p, ok[q]} T[q]  -- the
 * `frame_pose_ = frame_pose_ * T.inv()` recurrence of reference src/tracking.cpp:318 for frame
 * pairs that were tracked as independent chunks (other launches, contexts or GPUs: SURVEY.md 8e
 * granularity 2).  pose0 is a HOST pointer (NULL = identity); T_rel_inv, ok and poses_out live where
 * `mem` says.  SVO_MEM_HOST: the call returns when poses_out is complete; SVO_MEM_DEVICE: one
 * launch in stream order on the context's stream, no host synchronisation. */
int svo_chain_relative(svo_ctx *ctx, const double *T_rel_inv, const int32_t *ok, int n,
                       const double *pose0, double *poses_out, int mem);

/* Kernel-level timing of the last svo_track_batch / svo_add_frame, measured with HIP events on
 * the context's stream: fills up to `cap` (name, milliseconds) pairs, returns the count.
 * Enabled by svo_enable_timing(ctx, 1); adds event records between stages. */
int svo_enable_timing(svo_ctx *ctx, int on);
int svo_get_timing(svo_ctx *ctx, const char **names, float *ms, int cap);

#ifdef __cplusplus
}
#endif
#endif /* SVO_ABI_H */
