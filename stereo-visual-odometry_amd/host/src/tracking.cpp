// tracking.cpp -- lzb_vio::Tracking on top of the HIP library (reference src/tracking.cpp).
// The state machine is the reference's (AddFrame :49-77, StereoInit_f2f :78-92, Track :115-128);
// everything below it is ONE svo_add_frame call: FAST -> 4x LK -> filter -> triangulate ->
// solvePnPRansac -> gates -> frame_pose_ update all happen on the GPU.
#include "lzb_vio/tracking.h"
#include <cmath>

namespace lzb_vio {

bool Tracking::ReadImageScale(double *scale, int *interp, std::string *err)
{
    *scale = 1.0; *interp = SVO_INTERP_NEAREST;
    if (Config::Has("image_interp")) {
        const std::string v = Config::Get<std::string>("image_interp");
        if (v == "linear") *interp = SVO_INTERP_LINEAR;
        else if (v != "nearest") LZB_LOG("WARNING", "image_interp: '%s' is neither 'nearest' nor 'linear'; using 'nearest'", v.c_str());
    }
    if (!Config::Has("image_scale")) return true;
    const double f = Config::Get<double>("image_scale");
    if (!(f > 0.0 && f <= 1.0)) {
        char msg[160];
        snprintf(msg, sizeof(msg), "image_scale: %g is outside (0, 1] (frames are downscaled before tracking, never enlarged)", f);
        if (err) *err = msg;
        return false;
    }
    *scale = f;
    return true;
}

bool Tracking::ReadFastBuckets(int *cell_w, int *cell_h, int *keep, std::string *err)
{
    *cell_w = *cell_h = *keep = 0;
    const bool has_w = Config::Has("fast_bucket_width"), has_h = Config::Has("fast_bucket_height");
    const int w = has_w ? Config::Get<int>("fast_bucket_width") : 0, h = has_h ? Config::Get<int>("fast_bucket_height") : 0;
    const int k = Config::Has("fast_bucket_keep") ? Config::Get<int>("fast_bucket_keep") : 0;
    char msg[200] = "";
    if (has_w && w < 1) snprintf(msg, sizeof(msg), "fast_bucket_width: %d is < 1 (the cell width in pixels)", w);
    else if (has_h && h < 1) snprintf(msg, sizeof(msg), "fast_bucket_height: %d is < 1 (the cell height in pixels)", h);
    else if (k < 0) snprintf(msg, sizeof(msg), "fast_bucket_keep: %d is < 0 (corners kept per cell; 0 = off)", k);
    else if (k > 0 && !(has_w && has_h))
        snprintf(msg, sizeof(msg), "fast_bucket_keep: %d needs the cell size: %s is absent", k, has_w ? "fast_bucket_height" : "fast_bucket_width");
    else if (k > 0 && Config::Has("track_mode") && Config::Get<std::string>("track_mode") == "ORB_stereof2f_pnp")
        snprintf(msg, sizeof(msg), "fast_bucket_keep: %d with track_mode ORB_stereof2f_pnp (buckets are an LK-mode option; ORB mode "
                                   "spreads its keypoints with the quadtree)", k);
    if (msg[0]) { if (err) *err = msg; return false; }
    if (k > 0) { *cell_w = w; *cell_h = h; *keep = k; }
    return true;
}

bool Tracking::ReadLkDetector(int *detector, int *max_corners, double *quality_level, double *min_distance, std::string *err)
{
    *detector = SVO_DETECTOR_FAST; *max_corners = 500; *quality_level = 0.01; *min_distance = 20.0;
    const std::string d = Config::Has("lk_detector") ? Config::Get<std::string>("lk_detector") : std::string("fast");
    const int n = Config::Has("num_features") ? Config::Get<int>("num_features") : 500;
    // (a value that does not parse as a number reads as 0)
    const double q = Config::Has("gftt_quality_level") ? Config::Get<double>("gftt_quality_level") : 0.01;
    const double m = Config::Has("gftt_min_distance") ? Config::Get<double>("gftt_min_distance") : 20.0;
    const bool gftt = d == "gftt";
    char msg[240] = "";
    if (d != "fast" && !gftt) snprintf(msg, sizeof(msg), "lk_detector: '%s' is neither 'fast' nor 'gftt'", d.c_str());
    else if (!(std::isfinite(q) && q > 0.0)) snprintf(msg, sizeof(msg), "gftt_quality_level: %g is not a finite number > 0", q);
    else if (!(std::isfinite(m) && m >= 0.0)) snprintf(msg, sizeof(msg), "gftt_min_distance: %g is not a finite number >= 0", m);
    else if (gftt && Config::Has("track_mode") && Config::Get<std::string>("track_mode") == "ORB_stereof2f_pnp")
        snprintf(msg, sizeof(msg), "lk_detector: gftt with track_mode ORB_stereof2f_pnp (the detector switch is an LK-mode option)");
    else if (gftt && Config::Has("fast_bucket_keep") && Config::Get<int>("fast_bucket_keep") > 0)
        snprintf(msg, sizeof(msg), "lk_detector: gftt with fast_bucket_keep > 0 (the Shi-Tomasi detector spaces its own corners)");
    else if (gftt && Config::Has("fast_keep_strongest") && Config::Get<int>("fast_keep_strongest") > 0)
        snprintf(msg, sizeof(msg), "lk_detector: gftt with fast_keep_strongest > 0 (num_features bounds the Shi-Tomasi corners)");
    if (msg[0]) { if (err) *err = msg; return false; }
    if (gftt) { *detector = SVO_DETECTOR_GFTT; *max_corners = n; *quality_level = q; *min_distance = m; }
    return true;
}

bool Tracking::ReadPoseRefine(int *mode, int *rounds, int *iters, double *sigma_px, int *min_inliers, std::string *err)
{
    *mode = SVO_REFINE_OFF; *rounds = 4; *iters = 10; *sigma_px = 1.0; *min_inliers = 6;
    const std::string m = Config::Has("pose_refine") ? Config::Get<std::string>("pose_refine") : std::string("none");
    // (a value that does not parse as a number reads as 0)
    const int r = Config::Has("pose_refine_rounds") ? Config::Get<int>("pose_refine_rounds") : 4;
    const int it = Config::Has("pose_refine_iters") ? Config::Get<int>("pose_refine_iters") : 10;
    const double sg = Config::Has("pose_refine_sigma") ? Config::Get<double>("pose_refine_sigma") : 1.0;
    const int mi = Config::Has("pose_refine_min_inliers") ? Config::Get<int>("pose_refine_min_inliers") : 6;
    char msg[240] = "";
    if (m != "none" && m != "reproj" && m != "ba") snprintf(msg, sizeof(msg), "pose_refine: '%s' is neither 'none', 'reproj' nor 'ba'", m.c_str());
    else if (r < 1 || r > 16) snprintf(msg, sizeof(msg), "pose_refine_rounds: %d is outside 1..16", r);
    else if (it < 1 || it > 100) snprintf(msg, sizeof(msg), "pose_refine_iters: %d is outside 1..100", it);
    else if (!(std::isfinite(sg) && sg > 0.0)) snprintf(msg, sizeof(msg), "pose_refine_sigma: %g is not a finite number > 0", sg);
    else if (mi < 1) snprintf(msg, sizeof(msg), "pose_refine_min_inliers: %d is < 1", mi);
    if (msg[0]) { if (err) *err = msg; return false; }
    *mode = m == "reproj" ? SVO_REFINE_REPROJ : m == "ba" ? SVO_REFINE_BA : SVO_REFINE_OFF;
    *rounds = r; *iters = it; *sigma_px = sg; *min_inliers = mi;
    return true;
}

bool Tracking::ReadOrbMatcher(int *mode, int *th_stereo, int *th_track, double *ratio, double *radius, double *max_disparity, std::string *err)
{
    *mode = SVO_ORB_MATCHER_BRUTE; *th_stereo = 75; *th_track = 100; *ratio = 0.9; *radius = 0.0; *max_disparity = 0.0;
    const std::string m = Config::Has("orb_matcher") ? Config::Get<std::string>("orb_matcher") : std::string("brute");
    // (a value that does not parse as a number reads as 0)
    const int ts = Config::Has("orb_match_th_stereo") ? Config::Get<int>("orb_match_th_stereo") : 75;
    const int tt = Config::Has("orb_match_th_track") ? Config::Get<int>("orb_match_th_track") : 100;
    const double ra = Config::Has("orb_match_ratio") ? Config::Get<double>("orb_match_ratio") : 0.9;
    const double rd = Config::Has("orb_match_radius") ? Config::Get<double>("orb_match_radius") : 0.0;
    const double md = Config::Has("orb_max_disparity") ? Config::Get<double>("orb_max_disparity") : 0.0;
    char msg[240] = "";
    if (m != "brute" && m != "guided") snprintf(msg, sizeof(msg), "orb_matcher: '%s' is neither 'brute' nor 'guided'", m.c_str());
    else if (ts < 1 || ts > 256) snprintf(msg, sizeof(msg), "orb_match_th_stereo: %d is outside 1..256", ts);
    else if (tt < 1 || tt > 256) snprintf(msg, sizeof(msg), "orb_match_th_track: %d is outside 1..256", tt);
    else if (!(std::isfinite(ra) && ra > 0.0 && ra <= 1.0)) snprintf(msg, sizeof(msg), "orb_match_ratio: %g is outside (0, 1]", ra);
    else if (!(std::isfinite(rd) && rd >= 0.0)) snprintf(msg, sizeof(msg), "orb_match_radius: %g is not a finite number >= 0", rd);
    else if (!(std::isfinite(md) && md >= 0.0)) snprintf(msg, sizeof(msg), "orb_max_disparity: %g is not a finite number >= 0", md);
    else if (m == "guided" && !(Config::Has("track_mode") && Config::Get<std::string>("track_mode") == "ORB_stereof2f_pnp"))
        snprintf(msg, sizeof(msg), "orb_matcher: guided without track_mode ORB_stereof2f_pnp (the matcher switch is an ORB-mode option)");
    if (msg[0]) { if (err) *err = msg; return false; }
    *mode = m == "guided" ? SVO_ORB_MATCHER_GUIDED : SVO_ORB_MATCHER_BRUTE;
    *th_stereo = ts; *th_track = tt; *ratio = ra; *radius = rd; *max_disparity = md;
    return true;
}

bool Tracking::ReadTrackCarry(int *on, double *min_distance, int *max_age, std::string *err)
{
    *on = 0; *min_distance = 3.0; *max_age = 0;
    // (a value that does not parse as a number reads as 0)
    const int c = Config::Has("track_carry") ? Config::Get<int>("track_carry") : 0;
    const double md = Config::Has("track_carry_min_distance") ? Config::Get<double>("track_carry_min_distance") : 3.0;
    const int ma = Config::Has("track_carry_max_age") ? Config::Get<int>("track_carry_max_age") : 0;
    char msg[240] = "";
    if (c != 0 && c != 1) snprintf(msg, sizeof(msg), "track_carry: %d is neither 0 nor 1", c);
    else if (!(std::isfinite(md) && md >= 1.0 && md <= 256.0)) snprintf(msg, sizeof(msg), "track_carry_min_distance: %g is not a finite number in [1, 256]", md);
    else if (ma < 0) snprintf(msg, sizeof(msg), "track_carry_max_age: %d is < 0 (0 = unlimited)", ma);
    else if (c == 1 && Config::Has("track_mode") && Config::Get<std::string>("track_mode") == "ORB_stereof2f_pnp")
        snprintf(msg, sizeof(msg), "track_carry: 1 with track_mode ORB_stereof2f_pnp (track carry is an LK-mode option)");
    if (msg[0]) { if (err) *err = msg; return false; }
    *on = c; *min_distance = md; *max_age = ma;
    return true;
}

bool Tracking::ReadWindowBa(int *frames, int *rounds, int *iters, double *sigma, int *min_obs, std::string *err)
{
    *frames = 0; *rounds = 4; *iters = 5; *sigma = 1.0; *min_obs = 10;
    const int w = Config::Has("window_ba") ? Config::Get<int>("window_ba") : 0;
    const int r = Config::Has("window_ba_rounds") ? Config::Get<int>("window_ba_rounds") : 4;
    const int it = Config::Has("window_ba_iters") ? Config::Get<int>("window_ba_iters") : 5;
    const double sg = Config::Has("window_ba_sigma") ? Config::Get<double>("window_ba_sigma") : 1.0;
    const int mo = Config::Has("window_ba_min_obs") ? Config::Get<int>("window_ba_min_obs") : 10;
    const int carry = Config::Has("track_carry") ? Config::Get<int>("track_carry") : 0;
    char msg[240] = "";
    if (w != 0 && (w < 2 || w > SVO_WINDOW_MAX_FRAMES)) snprintf(msg, sizeof(msg), "window_ba: %d is neither 0 nor in 2..%d", w, SVO_WINDOW_MAX_FRAMES);
    else if (r < 1 || r > 16) snprintf(msg, sizeof(msg), "window_ba_rounds: %d is outside 1..16", r);
    else if (it < 1 || it > 100) snprintf(msg, sizeof(msg), "window_ba_iters: %d is outside 1..100", it);
    else if (!(std::isfinite(sg) && sg > 0.0)) snprintf(msg, sizeof(msg), "window_ba_sigma: %g is not a finite number > 0", sg);
    else if (mo < 1) snprintf(msg, sizeof(msg), "window_ba_min_obs: %d is < 1", mo);
    else if (w != 0 && carry != 1) snprintf(msg, sizeof(msg), "window_ba: %d without track_carry: 1 (the window is built from carried tracks)", w);
    if (msg[0]) { if (err) *err = msg; return false; }
    *frames = w; *rounds = r; *iters = it; *sigma = sg; *min_obs = mo;
    return true;
}

bool Tracking::ReadKeyframe(int *on, int *min_tracks, int *max_gap, std::string *err)
{
    *on = 0; *min_tracks = 60; *max_gap = 0;
    const int k = Config::Has("keyframe") ? Config::Get<int>("keyframe") : 0;
    const int g = Config::Has("keyframe_max_gap") ? Config::Get<int>("keyframe_max_gap") : 0;
    const int mt = Config::Has("num_features_needed_for_keyframe") ? Config::Get<int>("num_features_needed_for_keyframe") : 60;
    const int carry = Config::Has("track_carry") ? Config::Get<int>("track_carry") : 0;
    const int window = Config::Has("window_ba") ? Config::Get<int>("window_ba") : 0;
    char msg[240] = "";
    if (k != 0 && k != 1) snprintf(msg, sizeof(msg), "keyframe: %d is neither 0 nor 1", k);
    else if (g < 0 || g == 1) snprintf(msg, sizeof(msg), "keyframe_max_gap: %d is neither 0 (no limit) nor >= 2 (the smallest gap of a keyframe solve is 2)", g);
    else if (k == 1 && carry != 1) snprintf(msg, sizeof(msg), "keyframe: 1 without track_carry: 1 (the keyframe's points are found again by their carried ids)");
    else if (k == 1 && window != 0) snprintf(msg, sizeof(msg), "keyframe: 1 with window_ba: %d (both rewrite the step's pose: choose one)", window);
    else if (k == 1 && mt < 4) snprintf(msg, sizeof(msg), "keyframe: 1 with num_features_needed_for_keyframe: %d (a keyframe solve needs at least 4 tracks)", mt);
    if (msg[0]) { if (err) *err = msg; return false; }
    *on = k; *min_tracks = mt; *max_gap = g;
    return true;
}

bool Tracking::G2O_EstimatePose_PnP(const double projMatrl[12], const double projMatrr[12], const std::vector<cv::Point2f> &pointsLeft_t2,
                                    const std::vector<cv::Point2f> *pointsRight_t2, const std::vector<cv::Point3f> &points3D_t0,
                                    double rotation[3], double translation[3], svo_refine_result *result)
{
    const size_t n = points3D_t0.size();
    if (!ctx_ || pointsLeft_t2.size() != n || (pointsRight_t2 && pointsRight_t2->size() != n)) return false;
    static_assert(sizeof(cv::Point2f) == sizeof(svo_pt2f) && sizeof(cv::Point3f) == sizeof(svo_pt3f), "point layouts");
    // the stage call runs with the context's settings whatever its mode: EnsureContext has applied this object's keys
    svo_refine_result res;
    const int rc = svo_refine_pose(ctx_, (const svo_pt3f *)points3D_t0.data(), (const svo_pt2f *)pointsLeft_t2.data(),
                                   pointsRight_t2 ? (const svo_pt2f *)pointsRight_t2->data() : nullptr, (int)n, projMatrl, projMatrr, rotation,
                                   translation, &res, nullptr, SVO_MEM_HOST);
    if (rc != SVO_OK) {
        LZB_LOG("ERROR", "svo_refine_pose failed (%d): %s", rc, svo_last_error(ctx_));
        return false;
    }
    if (result) *result = res;
    for (int i = 0; i < 3; i++) { rotation[i] = res.rvec[i]; translation[i] = res.tvec[i]; }
    return res.status == SVO_REFINE_APPLIED;
}

Tracking::Tracking(System *system, Parameter::Ptr parameter, Sensors::Ptr sensors)
{
    sensors_ = sensors;
    system_ = system;
    parameter_ = parameter;
    memset(&last_, 0, sizeof(last_));
    Readparameter();
    // Config is a process-wide singleton (as in the reference, src/config.cpp:26): everything this object
    // needs from it is read NOW, so several System objects -- one per sequence -- can be built one after
    // the other and then run side by side
    max_keypoints_key_ = Config::Has("max_keypoints") ? Config::Get<int>("max_keypoints") : 0;
    // order of the float sums inside cv::calcOpticalFlowPyrLK (include/svo_abi.h): `exact` is independent of the
    // build; `sse2` / `simd128` / `sse2_legacy` add them in float in the lane orders of upstream's x86 SIMD code as restated in
    // oracle/lk.c (modes 2 / 4 / 3; recalled, not validated against an OpenCV binary) at about 1.9-2.2 x the LK kernel time
    fast_keep_strongest_ = Config::Has("fast_keep_strongest") ? Config::Get<int>("fast_keep_strongest") : 0;
    if (Config::Has("lk_accum")) {
        const std::string v = Config::Get<std::string>("lk_accum");
        if (v == "sse2") lk_accum_ = SVO_LK_ACCUM_SSE2;
        else if (v == "simd128") lk_accum_ = SVO_LK_ACCUM_SIMD128;
        else if (v == "sse2_legacy") lk_accum_ = SVO_LK_ACCUM_SSE2_LEGACY;
        else if (v != "exact") LZB_LOG("WARNING", "lk_accum: '%s' is none of 'exact', 'sse2', 'simd128', 'sse2_legacy'; using 'exact'", v.c_str());
    }
    if (!ReadImageScale(&image_scale_, &image_interp_, &config_error_)) image_scale_ = 1.0;     // the owner refuses to run (ConfigError)
    std::string bucket_error;
    if (!ReadFastBuckets(&bucket_w_, &bucket_h_, &bucket_keep_, &bucket_error) && config_error_.empty()) config_error_ = bucket_error;
    std::string detector_error;
    if (!ReadLkDetector(&lk_detector_, &gftt_num_, &gftt_quality_, &gftt_min_distance_, &detector_error) && config_error_.empty())
        config_error_ = detector_error;
    else if (lk_detector_ == SVO_DETECTOR_GFTT)
        LZB_LOG("INFO", "lk_detector: gftt (num_features %d, gftt_quality_level %g, gftt_min_distance %g)", gftt_num_, gftt_quality_,
                gftt_min_distance_);
    std::string refine_error;
    if (!ReadPoseRefine(&pose_refine_, &pose_refine_rounds_, &pose_refine_iters_, &pose_refine_sigma_, &pose_refine_min_inliers_,
                        &refine_error)) {
        if (config_error_.empty()) config_error_ = refine_error;
    } else if (pose_refine_ != SVO_REFINE_OFF)
        LZB_LOG("INFO", "pose_refine: %s (pose_refine_rounds %d, pose_refine_iters %d, pose_refine_sigma %g, pose_refine_min_inliers %d)",
                pose_refine_ == SVO_REFINE_BA ? "ba" : "reproj", pose_refine_rounds_, pose_refine_iters_, pose_refine_sigma_, pose_refine_min_inliers_);
    std::string carry_error;
    if (!ReadTrackCarry(&track_carry_, &track_carry_min_distance_, &track_carry_max_age_, &carry_error)) {
        if (config_error_.empty()) config_error_ = carry_error;
    } else if (track_carry_)
        LZB_LOG("INFO", "track_carry: 1 (track_carry_min_distance %g, track_carry_max_age %d)", track_carry_min_distance_, track_carry_max_age_);
    std::string window_error;
    if (!ReadWindowBa(&window_ba_, &window_ba_rounds_, &window_ba_iters_, &window_ba_sigma_, &window_ba_min_obs_, &window_error)) {
        if (config_error_.empty()) config_error_ = window_error;
    } else if (window_ba_)
        LZB_LOG("INFO", "window_ba: %d (window_ba_rounds %d, window_ba_iters %d, window_ba_sigma %g, window_ba_min_obs %d)", window_ba_,
                window_ba_rounds_, window_ba_iters_, window_ba_sigma_, window_ba_min_obs_);
    std::string keyframe_error;
    if (!ReadKeyframe(&keyframe_, &keyframe_min_tracks_, &keyframe_max_gap_, &keyframe_error)) {
        if (config_error_.empty()) config_error_ = keyframe_error;
    } else if (keyframe_)
        LZB_LOG("INFO", "keyframe: 1 (num_features_needed_for_keyframe %d, keyframe_max_gap %d)", keyframe_min_tracks_, keyframe_max_gap_);
    std::string matcher_error;
    if (!ReadOrbMatcher(&orb_matcher_, &orb_match_th_stereo_, &orb_match_th_track_, &orb_match_ratio_, &orb_match_radius_,
                        &orb_max_disparity_, &matcher_error)) {
        if (config_error_.empty()) config_error_ = matcher_error;
    } else if (orb_matcher_ == SVO_ORB_MATCHER_GUIDED)
        LZB_LOG("INFO", "orb_matcher: guided (orb_match_th_stereo %d, orb_match_th_track %d, orb_match_ratio %g, orb_match_radius %g, "
                "orb_max_disparity %g)", orb_match_th_stereo_, orb_match_th_track_, orb_match_ratio_, orb_match_radius_, orb_max_disparity_);
}

Tracking::~Tracking()
{
    if (ctx_) svo_destroy(ctx_);
}

void Tracking::Readparameter()
{
    num_features_init_ = parameter_->num_features_init_;
    num_features_ = parameter_->num_features_;
    num_features_tracking_bad_ = parameter_->num_features_tracking_bad_;
    num_features_needed_for_keyframe_ = parameter_->num_features_needed_for_keyframe_;
    init_landmarks_ = parameter_->init_landmarks_;
    feature_match_error_ = parameter_->feature_match_error_;
    track_mode_ = parameter_->track_mode_;
    num_features_tracking_ = parameter_->num_features_tracking_;
    inlier_rate_ = parameter_->inlier_rate_;
    iterationsCount_ = parameter_->iterationsCount_;
    reprojectionError_ = parameter_->reprojectionError_;
    confidence_ = parameter_->confidence_;
    maxmove_ = parameter_->maxmove_;
    minmove_ = parameter_->minmove_;
    nFeatures_ = parameter_->nFeatures_;
    fScaleFactor_ = parameter_->fScaleFactor_;
    nLevels_ = parameter_->nLevels_;
    fIniThFAST_ = parameter_->fIniThFAST_;
    fMinThFAST_ = parameter_->fMinThFAST_;
}

void Tracking::Set_vo(System *slam) { system_ = slam; }

bool Tracking::Reset()
{
    status_ = TrackingStatus::INITING;
    current_frame_ = nullptr; last_frame_ = nullptr;
    frame_pose_ = Pose4x4();
    Px_ = Py_ = Pz_ = 0;
    memset(&last_, 0, sizeof(last_));
    if (ctx_) svo_reset(ctx_);
    return true;
}

// The HIP context is sized by the first frame (the reference learns the size from cv::imread too).
bool Tracking::EnsureContext(int width, int height, int max_batch)
{
    if (ctx_ && width == ctx_w_ && height == ctx_h_ && max_batch <= ctx_batch_) return true;
    const bool resized = ctx_ && (width != ctx_w_ || height != ctx_h_);
    if (resized)
        LZB_LOG("WARNING", "frame size changed from %dx%d to %dx%d: the HIP context is rebuilt; this frame only "
                "re-initialises the tracker (no motion is estimated for it), the pose chain continues from frame_pose_",
                ctx_w_, ctx_h_, width, height);
    if (ctx_) { svo_destroy(ctx_); ctx_ = nullptr; }
    // image_scale: width x height is the SOURCE size the ingest stage takes; the context itself (and the default
    // max_keypoints below) has the working size, as cv::resize(..., Size(), f, f) makes it: cvRound(size * f)
    const int src_w = width, src_h = height;
    if (Ingest()) { width = (int)std::nearbyint(src_w * image_scale_); height = (int)std::nearbyint(src_h * image_scale_); }
    svo_config cfg;
    svo_default_config(&cfg, width, height);
    cfg.max_batch = keyframe_ && max_batch < 2 ? 2 : max_batch;      // keyframe: 1 solves on item 1 of the pose workspace (svo_set_keyframe)
    // cv::FAST is uncapped in the reference; the device buffers are not.  Capacity per image: the additive
    // YAML key max_keypoints, else one keypoint per 24 pixels (NMS keeps at most one corner per 3x3
    // block; textured KITTI frames hold 2-5 k, i.e. one per ~100-200 pixels), never less than 8192 or
    // than what the ORB extractor is asked for.  A frame that still exceeds it fails its pairs with
    // SVO_FAIL_CAPACITY, which is logged as an error below.
    {
        long cap = max_keypoints_key_ > 0 ? max_keypoints_key_ : (long)width * height / 24;
        if (cap < 8192) cap = 8192;
        if (cap < 2L * nFeatures_) cap = 2L * nFeatures_;
        if (track_mode_ == "ORB_stereof2f_pnp" && cap > 16384) cap = 16384;     // 16-bit indices in the ORB kernels
        if (cap > (1 << 20)) cap = 1 << 20;
        cfg.max_keypoints = (int)cap;
    }
    cfg.fast_threshold = 20;                                     // hard-coded, src/tracking.cpp:99
    cfg.num_features_tracking = num_features_tracking_;
    cfg.iterations = iterationsCount_;
    cfg.reproj_err = reprojectionError_;
    cfg.confidence = confidence_;
    cfg.feature_match_error = feature_match_error_;
    cfg.inlier_rate = inlier_rate_;
    cfg.lk_accum = lk_accum_;
    cfg.fast_keep_strongest = fast_keep_strongest_ > 0 ? fast_keep_strongest_ : 0;
    if (track_mode_ == "ORB_stereof2f_pnp") {
        // the shipped default (config/default.yaml:75): ORBextractor(nFeatures, fScaleFactor, nLevels,
        // fIniThFAST, fMinThFAST) (src/tracking.cpp:20) and the configured minmove / maxmove gate (:215)
        cfg.track_mode = SVO_MODE_ORB;
        cfg.orb_nfeatures = nFeatures_; cfg.orb_scale_factor = fScaleFactor_; cfg.orb_nlevels = nLevels_;
        cfg.orb_ini_th = fIniThFAST_; cfg.orb_min_th = fMinThFAST_;
        cfg.min_move2 = minmove_ * minmove_;
        cfg.max_move2 = maxmove_ * maxmove_;
    } else {
        cfg.track_mode = SVO_MODE_LK;
        cfg.min_move2 = 0.0005 * 0.0005;                         // LK mode, src/tracking.cpp:311
        cfg.max_move2 = 100.0;
    }
    memcpy(cfg.P1, sensors_->projMatr1_, sizeof(cfg.P1));
    memcpy(cfg.P2, sensors_->projMatr2_, sizeof(cfg.P2));
    if (Ingest() && (svo_scale_projection(sensors_->projMatr1_, image_scale_, image_scale_, image_interp_, cfg.P1) != SVO_OK ||
                     svo_scale_projection(sensors_->projMatr2_, image_scale_, image_scale_, image_interp_, cfg.P2) != SVO_OK)) {
        LZB_LOG("ERROR", "svo_scale_projection refused image_scale = %g", image_scale_);
        return false;
    }
    int rc = svo_create(&cfg, device_, &ctx_);
    if (rc != SVO_OK) {
        LZB_LOG("ERROR", "svo_create failed (%d): a HIP device is required, there is no CPU path", rc);
        ctx_ = nullptr;
        return false;
    }
    if (Ingest() && (rc = svo_ingest_create(ctx_, src_w, src_h, image_interp_, image_scale_, image_scale_)) != SVO_OK) {
        LZB_LOG("ERROR", "svo_ingest_create (image_scale %g, %dx%d -> %dx%d) failed (%d): %s", image_scale_, src_w, src_h, width, height,
                rc, svo_last_error(ctx_));
        svo_destroy(ctx_);
        ctx_ = nullptr;
        return false;
    }
    if (bucket_keep_ > 0 && (rc = svo_set_fast_buckets(ctx_, bucket_w_, bucket_h_, bucket_keep_)) != SVO_OK) {
        LZB_LOG("ERROR", "svo_set_fast_buckets (fast_bucket_width %d, fast_bucket_height %d, fast_bucket_keep %d at %dx%d) failed (%d): %s",
                bucket_w_, bucket_h_, bucket_keep_, width, height, rc, svo_last_error(ctx_));
        svo_destroy(ctx_);
        ctx_ = nullptr;
        return false;
    }
    if (lk_detector_ == SVO_DETECTOR_GFTT &&
        (rc = svo_set_lk_detector(ctx_, SVO_DETECTOR_GFTT, gftt_num_, gftt_quality_, gftt_min_distance_)) != SVO_OK) {
        LZB_LOG("ERROR", "svo_set_lk_detector (lk_detector gftt, num_features %d, gftt_quality_level %g, gftt_min_distance %g at %dx%d) "
                "failed (%d): %s", gftt_num_, gftt_quality_, gftt_min_distance_, width, height, rc, svo_last_error(ctx_));
        svo_destroy(ctx_);
        ctx_ = nullptr;
        return false;
    }
    // (also while the mode is none: svo_refine_pose, behind G2O_EstimatePose_PnP, runs with the context's settings; nothing is allocated then)
    rc = pose_refine_ == SVO_REFINE_BA
             ? svo_set_pose_refine_ba(ctx_, pose_refine_rounds_, pose_refine_iters_, pose_refine_sigma_, pose_refine_min_inliers_)
             : svo_set_pose_refine(ctx_, pose_refine_, pose_refine_rounds_, pose_refine_iters_, pose_refine_sigma_, pose_refine_min_inliers_);
    if (rc != SVO_OK) {
        LZB_LOG("ERROR", "%s (pose_refine %s, rounds %d, iters %d, sigma %g, min_inliers %d) failed (%d): %s",
                pose_refine_ == SVO_REFINE_BA ? "svo_set_pose_refine_ba" : "svo_set_pose_refine",
                pose_refine_ == SVO_REFINE_REPROJ ? "reproj" : pose_refine_ == SVO_REFINE_BA ? "ba" : "none", pose_refine_rounds_, pose_refine_iters_, pose_refine_sigma_, pose_refine_min_inliers_, rc, svo_last_error(ctx_));
        svo_destroy(ctx_);
        ctx_ = nullptr;
        return false;
    }
    if (orb_matcher_ == SVO_ORB_MATCHER_GUIDED &&
        (rc = svo_set_orb_matcher(ctx_, SVO_ORB_MATCHER_GUIDED, orb_match_th_stereo_, orb_match_th_track_, orb_match_ratio_, orb_match_radius_,
                                  orb_max_disparity_)) != SVO_OK) {
        LZB_LOG("ERROR", "svo_set_orb_matcher (orb_matcher guided, th_stereo %d, th_track %d, ratio %g, radius %g, max_disparity %g) failed (%d): %s",
                orb_match_th_stereo_, orb_match_th_track_, orb_match_ratio_, orb_match_radius_, orb_max_disparity_, rc, svo_last_error(ctx_));
        svo_destroy(ctx_);
        ctx_ = nullptr;
        return false;
    }
    if (track_carry_ && (rc = svo_set_track_carry(ctx_, 1, track_carry_min_distance_, track_carry_max_age_)) != SVO_OK) {
        LZB_LOG("ERROR", "svo_set_track_carry (track_carry 1, track_carry_min_distance %g, track_carry_max_age %d) failed (%d): %s",
                track_carry_min_distance_, track_carry_max_age_, rc, svo_last_error(ctx_));
        svo_destroy(ctx_);
        ctx_ = nullptr;
        return false;
    }
    if (window_ba_ && (rc = svo_set_window_ba(ctx_, window_ba_, window_ba_rounds_, window_ba_iters_, window_ba_sigma_, window_ba_min_obs_)) != SVO_OK) {
        LZB_LOG("ERROR", "svo_set_window_ba (window_ba %d) failed (%d): %s", window_ba_, rc, svo_last_error(ctx_));
        svo_destroy(ctx_);
        ctx_ = nullptr;
        return false;
    }
    if (keyframe_ && (rc = svo_set_keyframe(ctx_, 1, keyframe_min_tracks_, keyframe_max_gap_)) != SVO_OK) {
        LZB_LOG("ERROR", "svo_set_keyframe (keyframe 1, num_features_needed_for_keyframe %d, keyframe_max_gap %d) failed (%d): %s",
                keyframe_min_tracks_, keyframe_max_gap_, rc, svo_last_error(ctx_));
        svo_destroy(ctx_);
        ctx_ = nullptr;
        return false;
    }
    ctx_w_ = src_w; ctx_h_ = src_h; ctx_batch_ = max_batch;
    work_w_ = width; work_h_ = height;
    if (resized) svo_set_pose(ctx_, frame_pose_.m);          // the new context's first frame only initialises; the chain goes on
    return true;
}

bool Tracking::AddFrame(Frame::Ptr frame)
{
    current_frame_ = frame;
    bool ok = true;
    switch (status_) {
    case TrackingStatus::INITING:
        StereoInit_f2f();
        break;
    case TrackingStatus::TRACKING_GOOD:
        ok = Track();
        last_frame_ = current_frame_;          // on success AND failure (src/tracking.cpp:59-68)
        return ok;
    case TrackingStatus::LOST:
        break;
    }
    return true;
}

static bool feed(svo_ctx *ctx, bool ingest, Frame::Ptr f, svo_step_result *res, int *rc_out)
{
    const cv::Mat &L = f->left_img_, &R = f->right_img_;
    if (L.empty() || R.empty() || L.rows != R.rows || L.cols != R.cols || L.step != R.step) {
        LZB_LOG("ERROR", "stereo frame %lu has missing or mismatched images", f->id_);
        *rc_out = SVO_ERR_ARG;
        return false;
    }
    *rc_out = ingest ? svo_ingest_add_frame(ctx, L.data, R.data, (int)L.step, SVO_MEM_HOST, res)
                     : svo_add_frame(ctx, L.data, R.data, (int)L.step, SVO_MEM_HOST, res);
    if (*rc_out < 0) LZB_LOG("ERROR", "svo_add_frame: %s", svo_last_error(ctx));
    if (*rc_out == SVO_FAIL_CAPACITY)
        LZB_LOG("ERROR", "frame %lu: more keypoints than the context's capacity (YAML key max_keypoints); "
                "the pair was NOT tracked and the pose keeps its previous value", f->id_);
    return *rc_out == SVO_OK;
}

// Frame::features_left_ / features_right_ / *_Descriptors_ as the reference's detectors leave them
// (Detect_OpenCVFASTFeatures src/tracking.cpp:94-113, Detect_MyORBFeatures :502-532); optional
// because it costs a device-to-host copy and N heap allocations per frame.
void Tracking::FillFeatures()
{
    if (!fill_features_ || !ctx_ || !current_frame_) return;
    const bool orb = track_mode_ == "ORB_stereof2f_pnp";
    std::vector<svo_keypoint> kps(65536);
    std::vector<uint8_t> desc;
    if (orb) desc.resize(kps.size() * 32);
    for (int side = 0; side < (orb ? 2 : 1); side++) {
        int n = 0;
        if (svo_get_frame_keypoints(ctx_, side, kps.data(), orb ? desc.data() : nullptr, (int)kps.size(), &n) != SVO_OK) {
            LZB_LOG("ERROR", "svo_get_frame_keypoints: %s", svo_last_error(ctx_));
            return;
        }
        auto &dst = side == 0 ? current_frame_->features_left_ : current_frame_->features_right_;
        dst.clear();
        dst.reserve((size_t)n);
        for (int i = 0; i < n; i++) {
            cv::KeyPoint kp;
            kp.pt.x = kps[i].x; kp.pt.y = kps[i].y; kp.size = kps[i].size; kp.angle = kps[i].angle;
            kp.response = kps[i].response; kp.octave = kps[i].octave; kp.class_id = kps[i].class_id;
            Feature::Ptr f(new Feature(current_frame_, kp));
            f->is_on_left_image_ = side == 0;
            if (orb) { f->Descriptor_.create(1, 32); memcpy(f->Descriptor_.ptr(0), desc.data() + (size_t)i * 32, 32); }
            dst.push_back(f);
        }
        if (orb) {
            cv::Mat &D = side == 0 ? current_frame_->left_Descriptors_ : current_frame_->right_Descriptors_;
            D.create(n > 0 ? n : 1, 32);
            D.rows = n;
            for (int i = 0; i < n; i++) memcpy(D.ptr(i), desc.data() + (size_t)i * 32, 32);
        }
    }
}

bool Tracking::GetLastTracks(std::vector<cv::Point2f> &t1_left, std::vector<cv::Point2f> &t1_right,
                             std::vector<cv::Point2f> &t2_left, std::vector<unsigned char> &inlier)
{
    t1_left.clear(); t1_right.clear(); t2_left.clear(); inlier.clear();
    if (!ctx_) return false;
    const int cap = last_.n_tracked > 0 ? last_.n_tracked : 0;
    std::vector<svo_pt2f> a((size_t)cap + 1), b((size_t)cap + 1), c((size_t)cap + 1);
    inlier.resize((size_t)cap + 1);
    int n = 0;
    if (svo_get_last_tracks(ctx_, a.data(), b.data(), nullptr, c.data(), inlier.data(), cap, &n) != SVO_OK) return false;
    inlier.resize((size_t)n);
    for (int i = 0; i < n; i++) {
        t1_left.push_back(cv::Point2f{a[i].x, a[i].y});
        t1_right.push_back(cv::Point2f{b[i].x, b[i].y});
        t2_left.push_back(cv::Point2f{c[i].x, c[i].y});
    }
    return true;
}

bool Tracking::GetLastTrackIds(std::vector<int64_t> &ids, std::vector<int32_t> &ages)
{
    ids.clear(); ages.clear();
    if (!ctx_ || !track_carry_) return false;
    const int cap = last_.n_tracked > 0 ? last_.n_tracked : 0;
    ids.resize((size_t)cap + 1); ages.resize((size_t)cap + 1);
    int n = 0;
    if (svo_get_last_track_ids(ctx_, ids.data(), ages.data(), cap, &n) != SVO_OK) { ids.clear(); ages.clear(); return false; }
    ids.resize((size_t)n); ages.resize((size_t)n);
    return true;
}

bool Tracking::StereoInit_f2f()
{
    if (!EnsureContext(current_frame_->left_img_.cols, current_frame_->left_img_.rows)) return false;
    svo_reset(ctx_);
    int rc;
    feed(ctx_, Ingest(), current_frame_, &last_, &rc);
    FillFeatures();
    last_frame_ = current_frame_;
    status_ = TrackingStatus::TRACKING_GOOD;
    return rc >= 0;
}

bool Tracking::Track()
{
    if (track_mode_ == "LK_stereof2f_pnp") return LK_StereoF2F_PnP_Track();
    if (track_mode_ == "ORB_stereof2f_pnp") return ORB_StereoF2F_PnP_Track();
    return false;                               // any other string: Track() is always false (:127)
}

// Both modes are one svo_add_frame call; the context was created for the configured track_mode.
bool Tracking::LK_StereoF2F_PnP_Track() { return TrackOnGpu(); }
bool Tracking::ORB_StereoF2F_PnP_Track() { return TrackOnGpu(); }

bool Tracking::TrackOnGpu()
{
    if (!EnsureContext(current_frame_->left_img_.cols, current_frame_->left_img_.rows)) return false;
    int rc;
    bool ok = feed(ctx_, Ingest(), current_frame_, &last_, &rc);
    if (rc < 0) return false;
    FillFeatures();
    if (ok) {
        memcpy(frame_pose_.m, last_.pose, sizeof(frame_pose_.m));
        Px_ = frame_pose_.m[3]; Py_ = frame_pose_.m[7]; Pz_ = frame_pose_.m[11];
    }
    return ok;
}

// Batched equivalent of n_frames - 1 AddFrame calls on frames already in device buffer `buf`.
bool Tracking::TrackUploaded(int buf, int n_frames, std::vector<svo_step_result> &out)
{
    return TrackUploadedAsync(buf, n_frames) && CollectUploaded(out);
}

bool Tracking::TrackUploadedAsync(int buf, int n_frames, bool continue_chain)
{
    if (!ctx_ || n_frames < 2 || async_tail_ - async_head_ >= 2) return false;
    // a chunk that continues the chain starts with the previous chunk's last frame (the runner's and the stream's one-frame
    // halo): its features are carried over on the device instead of being extracted again
    int rc = svo_track_uploaded_async(ctx_, buf, n_frames, frame_pose_.m, continue_chain ? (SVO_CONTINUE_CHAIN | SVO_CONTINUE_CARRY_FRAME) : 0);
    if (rc < 0) {
        LZB_LOG("ERROR", "svo_track_uploaded_async: %s", svo_last_error(ctx_));
        return false;
    }
    async_pairs_[async_tail_ & 1] = n_frames - 1;
    async_tail_++;
    return true;
}

int Tracking::ResultsReady()
{
    int n = 0;
    if (!ctx_ || async_tail_ == async_head_ || svo_results_ready(ctx_, &n) != SVO_OK) return 0;
    return n;
}

bool Tracking::CollectUploaded(std::vector<svo_step_result> &out)
{
    if (!ctx_ || async_tail_ == async_head_) return false;
    const int n = async_pairs_[async_head_ & 1];
    const size_t first = out.size();
    out.resize(first + (size_t)n);
    int rc = svo_collect_results(ctx_, out.data() + first, n);
    if (rc < 0) {                                            // the context's ring did not advance either: stay in step with it
        LZB_LOG("ERROR", "svo_collect_results: %s", svo_last_error(ctx_));
        out.resize(first);
        return false;
    }
    async_head_++;
    for (size_t i = first; i < out.size(); i++)
        if (out[i].fail_stage == SVO_FAIL_CAPACITY)
            LZB_LOG("ERROR", "pair %zu of the batch: a frame has more keypoints than the context's capacity "
                    "(YAML key max_keypoints); the pair was NOT tracked", i - first);
    last_ = out.back();
    memcpy(frame_pose_.m, last_.pose, sizeof(frame_pose_.m));
    Px_ = frame_pose_.m[3]; Py_ = frame_pose_.m[7]; Pz_ = frame_pose_.m[11];
    status_ = TrackingStatus::TRACKING_GOOD;
    return true;
}

}  // namespace lzb_vio
