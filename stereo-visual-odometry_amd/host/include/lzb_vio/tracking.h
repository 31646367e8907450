// tracking.h -- host-side mirror of lzb_vio::Tracking (reference include/lzb_vio/tracking.h:29-154).
// The public surface is the reference's: Tracking(System*, Parameter::Ptr, Sensors::Ptr),
// AddFrame(Frame::Ptr), GetStatus(), Set_vo(System*).  The private OpenCV stages are replaced by
// ONE call into the HIP library per frame (svo_add_frame, include/svo_abi.h); there is no CPU
// implementation behind this class.  Additive API: GetPose(), LastResult().
#pragma once
#ifndef lzb_vio_TRACKING_H
#define lzb_vio_TRACKING_H

#include "lzb_vio/feature.h"
#include "lzb_vio/frame.h"
#include "lzb_vio/parameter.h"
#include "lzb_vio/sensors.h"
#include "svo_abi.h"

namespace lzb_vio {
class System;

enum class TrackingStatus { INITING, TRACKING_GOOD, LOST };

class Tracking {
public:
    typedef std::shared_ptr<Tracking> Ptr;
    Tracking(System *system, Parameter::Ptr parameter, Sensors::Ptr sensors);
    ~Tracking();
    void Set_vo(System *vo);
    bool AddFrame(Frame::Ptr frame);
    TrackingStatus GetStatus() const { return status_; }

    // private no-op in the reference (include/lzb_vio/tracking.h:46, src/tracking.cpp:662-665; its call
    // sites are commented out); public here and it does what the name says: back to INITING, identity pose
    bool Reset();

    // additive (the reference has no getter for frame_pose_)
    Pose4x4 GetPose() const { return frame_pose_; }
    const svo_step_result &LastResult() const { return last_; }
    void SetDevice(int device) { device_ = device; }         // HIP device of the context (before the first frame); default 0
    int Device() const { return device_; }
    void SetFillFeatures(bool on) { fill_features_ = on; }   // populate Frame::features_* / *_Descriptors_ (costs a D2H)
    // the matched tracks of the pair just tracked + RANSAC inlier flags (what displayTracking drew)
    bool GetLastTracks(std::vector<cv::Point2f> &t1_left, std::vector<cv::Point2f> &t1_right,
                       std::vector<cv::Point2f> &t2_left, std::vector<unsigned char> &inlier);

    // additive YAML keys image_scale / image_interp (reference src/System.cpp:93-97: cv::resize(img, img, Size(), f, f,
    // INTER_NEAREST) in front of AddFrame).  image_scale: f in (0, 1]; absent or 1: the frames are tracked as they come and no
    // ingest stage exists.  image_interp: nearest (default, the reference's choice) | linear.  With f < 1 the context is
    // created at the WORKING size cvRound(file size * f) with P1 / P2 passed through svo_scale_projection, and the frames
    // travel through the svo_ingest_* twins of the entry points (include/svo_abi.h); thresholds in pixels are the YAML's
    // values AT THE WORKING SIZE.  ReadImageScale reads and checks the two keys of the loaded YAML (false + a message that
    // names the key); ConfigError() is that message for this object's YAML (empty: fine).
    static bool ReadImageScale(double *scale, int *interp, std::string *err);
    const std::string &ConfigError() const { return config_error_; }
    // additive YAML keys fast_bucket_width / fast_bucket_height / fast_bucket_keep (svo_set_fast_buckets, include/svo_abi.h): LK
    // mode keeps the fast_bucket_keep strongest FAST corners of every width x height pixel cell.  All absent (or keep 0): off.
    // ReadFastBuckets reads and checks them for the loaded YAML: a keep value without both sizes, a size < 1, a negative keep
    // or ORB mode with keep > 0 is refused (false + a message that names the key).  The keys are applied right after svo_create.
    static bool ReadFastBuckets(int *cell_w, int *cell_h, int *keep, std::string *err);
    // additive YAML keys lk_detector: fast | gftt (absent: fast), gftt_quality_level (default 0.01) and gftt_min_distance
    // (default 20) -- the literals of the reference's dormant cv::GFTTDetector::create(num_features, 0.01, 20)
    // (src/tracking.cpp:18); the corner count is the existing key num_features (GFTTDetector_num_; absent: 500).
    // svo_set_lk_detector, include/svo_abi.h.  ReadLkDetector reads and checks them for the loaded YAML: an unknown detector, a
    // quality level that is not a finite number > 0, a negative or non-finite distance, and gftt together with ORB mode, the
    // FAST buckets or fast_keep_strongest are refused (false + a message that names the key).  Applied right after svo_create.
    static bool ReadLkDetector(int *detector, int *max_corners, double *quality_level, double *min_distance, std::string *err);
    // additive YAML keys pose_refine: none | reproj | ba (absent: none), pose_refine_rounds (4), pose_refine_iters (10),
    // pose_refine_sigma (1.0 px) and pose_refine_min_inliers (6): the robust two-view pose refinement after solvePnPRansac
    // (svo_set_pose_refine, include/svo_abi.h).  ReadPoseRefine reads and checks them for the loaded YAML: an unknown mode,
    // rounds outside 1..16, iterations outside 1..100, a sigma that is not a finite number > 0, min_inliers < 1 -> false, *err
    // names the key.  The values are checked even while the mode is none.
    static bool ReadPoseRefine(int *mode, int *rounds, int *iters, double *sigma_px, int *min_inliers, std::string *err);
    // additive YAML keys orb_matcher: brute | guided (absent: brute, the reference's matcher), orb_match_th_stereo (75),
    // orb_match_th_track (100), orb_match_ratio (0.9), orb_match_radius (0: the whole image) and orb_max_disparity (0: P1[0]):
    // the guided ORB matcher (svo_set_orb_matcher, include/svo_abi.h); Parameter carries them.  ReadOrbMatcher reads and checks
    // them for the loaded YAML: an unknown matcher, a threshold outside 1..256, a ratio outside (0, 1], a negative or
    // non-finite radius / disparity, and guided without track_mode ORB_stereof2f_pnp are refused (false + a message that
    // names the key).  Applied right after svo_create.
    static bool ReadOrbMatcher(int *mode, int *th_stereo, int *th_track, double *ratio, double *radius, double *max_disparity, std::string *err);
    // additive YAML keys track_carry: 0 | 1 (absent: 0), track_carry_min_distance (3.0 px) and track_carry_max_age (0 = unlimited):
    // LK tracks kept across frames under persistent ids (svo_set_track_carry, include/svo_abi.h); Parameter carries them.
    // ReadTrackCarry reads and checks them for the loaded YAML: a switch that is neither 0 nor 1, a distance that is not a finite
    // number in [1, 256], a negative age, and track_carry 1 with track_mode ORB_stereof2f_pnp are refused (false + a message that
    // names the key).  Applied right after svo_create.  It is a feature of the per-frame paths: System refuses it together with
    // batch_size > 1, stream_depth > 0 and --split-pairs.
    static bool ReadTrackCarry(int *on, double *min_distance, int *max_age, std::string *err);
    // additive YAML keys window_ba: W (absent / 0: off; 2..8) with window_ba_rounds (4), window_ba_iters (5), window_ba_sigma (1.0)
    // and window_ba_min_obs (10): the sliding-window bundle adjustment of the per-frame chain (svo_set_window_ba).  Refused like
    // the keys above: W outside 0, 2..8, values outside svo_set_window_ba's ranges, and window_ba without track_carry: 1.
    static bool ReadWindowBa(int *frames, int *rounds, int *iters, double *sigma, int *min_obs, std::string *err);
    // additive YAML keys keyframe: 0 | 1 (absent: 0) and keyframe_max_gap (0 = no limit; else >= 2): the keyframe-relative pose of
    // the per-frame chain (svo_set_keyframe); the tracks a solve needs come from the reference's own key
    // num_features_needed_for_keyframe.  Refused like the keys above: a switch that is neither 0 nor 1, a gap that is negative or
    // 1, keyframe: 1 without track_carry: 1 or together with window_ba (both rewrite the pose), or with
    // num_features_needed_for_keyframe < 4.  System refuses it together with batch_size > 1, stream_depth > 0, --split-pairs and
    // --interleave.
    static bool ReadKeyframe(int *on, int *min_tracks, int *max_gap, std::string *err);
    bool Keyframe() const { return keyframe_ != 0; }
    bool TrackCarry() const { return track_carry_ != 0; }
    // id and age at t1 of every track GetLastTracks returns, in its order (track carry on; false otherwise)
    bool GetLastTrackIds(std::vector<int64_t> &ids, std::vector<int32_t> &ages);
    // The stage the reference declares as Tracking::G2O_EstimatePose_PnP (include/lzb_vio/tracking.h:82; its body there is a copy
    // of the OpenCV one and it is never called): here it does what its name says, through svo_refine_pose -- a robust motion-only
    // bundle adjustment of (rotation, translation) on the points' t2 observations in the left and, when pointsRight_t2 is not null,
    // the right camera, with this object's pose_refine_* settings.  rotation (a rotation VECTOR) and translation go in as the
    // start and come out refined; false: the start pose stands (too few inliers, degenerate, or no device).  result, when not
    // null, receives the stage's record (information matrix, active count, status).  NOTE: nothing in host/ calls it -- the fused
    // path refines inside svo_add_frame / svo_track_* -- and no test exercises it; what it wraps, svo_refine_pose, is held against
    // the numpy reference by tests/test_gpu_refine.py.
    bool G2O_EstimatePose_PnP(const double projMatrl[12], const double projMatrr[12], const std::vector<cv::Point2f> &pointsLeft_t2,
                              const std::vector<cv::Point2f> *pointsRight_t2, const std::vector<cv::Point3f> &points3D_t0,
                              double rotation[3], double translation[3], svo_refine_result *result = nullptr);
    bool Ingest() const { return image_scale_ < 1.0; }
    double ImageScale() const { return image_scale_; }
    int ImageInterp() const { return image_interp_; }
    int WorkWidth() const { return work_w_; }               // the context's frame size (0 before the first frame)
    int WorkHeight() const { return work_h_; }

    // additive: batched tracking of host-resident frames.  The context is
    // (re)created for `max_batch` frame pairs per launch; frames travel with svo_upload_frames and
    // TrackUploaded runs svo_track_uploaded on device buffer `buf`, appends the n_frames - 1 step
    // records and advances frame_pose_ exactly as n_frames - 1 AddFrame calls would.
    bool EnsureBatchContext(int width, int height, int max_batch) { return EnsureContext(width, height, max_batch); }
    svo_ctx *Context() { return ctx_; }
    // pairs of the oldest outstanding async batch when its records are complete (CollectUploaded will not wait), else 0
    int ResultsReady();
    int Outstanding() const { return (int)(async_tail_ - async_head_); }
    bool TrackUploaded(int buf, int n_frames, std::vector<svo_step_result> &out);
    // the same in two halves: launch without waiting for the GPU, then (after the caller has decoded and
    // uploaded the next chunk, whose copy then overlaps this batch's kernels) collect the records
    // (up to two chunks may be outstanding, collected in launch order; continue_chain seeds the pose chain on
    // the device with the previous chunk's last pose, so a chunk can be launched before its predecessor's
    // records have come back)
    bool TrackUploadedAsync(int buf, int n_frames, bool continue_chain = false);
    bool CollectUploaded(std::vector<svo_step_result> &out);

private:
    bool StereoInit_f2f();
    bool Track();
    bool LK_StereoF2F_PnP_Track();
    bool ORB_StereoF2F_PnP_Track();
    bool TrackOnGpu();
    void FillFeatures();
    void Readparameter();
    bool EnsureContext(int width, int height, int max_batch = 1);

    TrackingStatus status_ = TrackingStatus::INITING;
    Frame::Ptr current_frame_ = nullptr, last_frame_ = nullptr;
    Sensors::Ptr sensors_ = nullptr;
    System *system_ = nullptr;
    Parameter::Ptr parameter_ = nullptr;
    Pose4x4 frame_pose_;
    double Px_ = 0, Py_ = 0, Pz_ = 0;

    svo_ctx *ctx_ = nullptr;
    int device_ = 0;
    long max_keypoints_key_ = 0;                             // additive YAML key max_keypoints, read once (0 = absent)
    int fast_keep_strongest_ = 0;                            // additive YAML key fast_keep_strongest (0 = every corner)
    int bucket_w_ = 0, bucket_h_ = 0, bucket_keep_ = 0;      // additive YAML keys fast_bucket_width / _height / _keep (keep 0 = off)
    int lk_detector_ = SVO_DETECTOR_FAST, gftt_num_ = 500;    // additive YAML keys lk_detector: fast (default) | gftt, num_features
    double gftt_quality_ = 0.01, gftt_min_distance_ = 20.0;  // additive YAML keys gftt_quality_level, gftt_min_distance
    int pose_refine_ = SVO_REFINE_OFF, pose_refine_rounds_ = 4, pose_refine_iters_ = 10, pose_refine_min_inliers_ = 6;   // pose_refine*
    double pose_refine_sigma_ = 1.0;
    int orb_matcher_ = SVO_ORB_MATCHER_BRUTE, orb_match_th_stereo_ = 75, orb_match_th_track_ = 100;                     // orb_matcher / orb_match_*
    double orb_match_ratio_ = 0.9, orb_match_radius_ = 0.0, orb_max_disparity_ = 0.0;
    int window_ba_ = 0, window_ba_rounds_ = 4, window_ba_iters_ = 5, window_ba_min_obs_ = 10; double window_ba_sigma_ = 1.0;   // additive YAML keys window_ba*
    int keyframe_ = 0, keyframe_min_tracks_ = 60, keyframe_max_gap_ = 0;     // additive YAML keys keyframe / keyframe_max_gap (+ num_features_needed_for_keyframe)
    int track_carry_ = 0, track_carry_max_age_ = 0;          // additive YAML keys track_carry / track_carry_max_age
    double track_carry_min_distance_ = 3.0;                  // ... and track_carry_min_distance
    int lk_accum_ = SVO_LK_ACCUM_EXACT;                      // additive YAML key lk_accum: exact (default) | sse2 | simd128
    double image_scale_ = 1.0;                               // additive YAML key image_scale (1 = no ingest stage)
    int image_interp_ = SVO_INTERP_NEAREST;                  // additive YAML key image_interp: nearest (default) | linear
    std::string config_error_;
    int ctx_w_ = 0, ctx_h_ = 0, ctx_batch_ = 0;              // the size the context was built FOR: the frames' (source) size
    int work_w_ = 0, work_h_ = 0;                            // the context's own size: cvRound(source * image_scale)
    int async_pairs_[2] = {0, 0};
    unsigned async_head_ = 0, async_tail_ = 0;
    svo_step_result last_;
    bool fill_features_ = false;

    // Readparameter()
    int num_features_ = 200, num_features_init_ = 100, num_features_tracking_ = 50;
    int num_features_tracking_bad_ = 20, num_features_needed_for_keyframe_ = 80, init_landmarks_ = 5;
    double feature_match_error_ = 10, inlier_rate_ = 0.5;
    int iterationsCount_ = 500;
    float reprojectionError_ = 0.5f, confidence_ = 0.999f;
    double minmove_ = 0.01, maxmove_ = 0.01;
    std::string track_mode_ = "stereoicp_f2f";
    int nFeatures_ = 0, nLevels_ = 0, fIniThFAST_ = 0, fMinThFAST_ = 0;
    float fScaleFactor_ = 0;
};

}  // namespace lzb_vio
#endif
