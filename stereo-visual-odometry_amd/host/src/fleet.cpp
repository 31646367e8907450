// fleet.cpp -- lzb_vio::Fleet and the interleaved runner on top of svo_streams_* (include/svo_abi.h).
#include "lzb_vio/fleet.h"
#include "lzb_vio/config.h"
#include <chrono>
#include <set>

namespace lzb_vio {

Fleet::Fleet(const std::string &config_path, int n_streams, int max_step)
{
    if (Config::SetParameterFile(config_path) == false) {
        fprintf(stderr, "unable to open %s\n", config_path.c_str());
        exit(-1);                                          // as System does (reference src/System.cpp:15-19)
    }
    parameter_ = Parameter::Ptr(new Parameter);
    sensors_ = Sensors::Ptr(new Sensors(parameter_));
    tracking_ = Tracking::Ptr(new Tracking(nullptr, parameter_, sensors_));
    if (!tracking_->ConfigError().empty()) {               // refused on the host, before a device is opened
        fprintf(stderr, "%s: %s\n", config_path.c_str(), tracking_->ConfigError().c_str());
        exit(2);
    }
    n_streams_ = n_streams < 1 ? 1 : n_streams;
    max_step_ = max_step < 1 || max_step > n_streams_ ? n_streams_ : max_step;
    poses_.assign((size_t)n_streams_, Pose4x4());
    svo_step_result zero;
    memset(&zero, 0, sizeof(zero));
    last_.assign((size_t)n_streams_, zero);
}

Fleet::~Fleet()
{
    for (int cam = 0; cam < 2; cam++) if (pin_[cam]) svo_host_free(nullptr, pin_[cam]);
}

std::vector<bool> Fleet::Step(const std::vector<std::pair<int, Frame::Ptr>> &frames)
{
    const int m = (int)frames.size();
    std::vector<bool> out((size_t)m, false);
    if (m == 0) return out;
    auto fail = [&](const char *what) { LZB_LOG("ERROR", "Fleet::Step: %s", what); failed_ = true; return out; };
    if (m > max_step_) return fail("more frames than max_step");
    for (const auto &e : frames) {
        const Frame::Ptr &f = e.second;
        if (!f || f->left_img_.empty() || f->right_img_.empty() || f->left_img_.rows != f->right_img_.rows ||
            f->left_img_.cols != f->right_img_.cols)
            return fail("a stereo frame has missing or mismatched images");
        if (w_ == 0) { w_ = f->left_img_.cols; h_ = f->left_img_.rows; }
        if (f->left_img_.cols != w_ || f->left_img_.rows != h_) return fail("the streams of a fleet share one frame size");
    }
    svo_ctx *ctx = tracking_->Context();
    if (!ctx) {
        // 2 m of the context's max_batch + 1 working frame slots per step (svo_streams_step)
        if (!tracking_->EnsureBatchContext(w_, h_, 2 * max_step_ - 1 < 1 ? 1 : 2 * max_step_ - 1)) return fail("no context");
        ctx = tracking_->Context();
        if (svo_streams_create(ctx, n_streams_) != SVO_OK) return fail(svo_last_error(ctx));
        pitch_ = (w_ + 255) / 256 * 256;                    // the library's staging pitch: one copy per camera
        for (int cam = 0; cam < 2; cam++)
            if (svo_host_alloc(ctx, (size_t)pitch_ * h_ * (size_t)max_step_, (void **)&pin_[cam]) != SVO_OK) return fail(svo_last_error(ctx));
    }
    const size_t fbytes = (size_t)pitch_ * h_;
    std::vector<int32_t> ids((size_t)m);
    for (int i = 0; i < m; i++) {
        ids[(size_t)i] = frames[(size_t)i].first;
        const cv::Mat *img[2] = {&frames[(size_t)i].second->left_img_, &frames[(size_t)i].second->right_img_};
        for (int cam = 0; cam < 2; cam++)
            for (int y = 0; y < h_; y++)
                memcpy(pin_[cam] + (size_t)i * fbytes + (size_t)y * pitch_, img[cam]->data + (size_t)y * img[cam]->step, (size_t)w_);
    }
    std::vector<svo_step_result> res((size_t)m);
    const int rc = (tracking_->Ingest() ? svo_ingest_streams_step : svo_streams_step)(ctx, ids.data(), m, pin_[0], pin_[1], pitch_, (int64_t)fbytes,
                                                                                      SVO_MEM_HOST, res.data(), SVO_MEM_HOST);
    if (rc != SVO_OK) return fail(svo_last_error(ctx));
    for (int i = 0; i < m; i++) {
        const svo_step_result &r = res[(size_t)i];
        last_[(size_t)ids[(size_t)i]] = r;
        memcpy(poses_[(size_t)ids[(size_t)i]].m, r.pose, sizeof(r.pose));
        if (r.fail_stage == SVO_FAIL_CAPACITY)
            LZB_LOG("ERROR", "stream %d: more keypoints than the context's capacity (YAML key max_keypoints); "
                    "the pair was NOT tracked and the pose keeps its previous value", ids[(size_t)i]);
        out[(size_t)i] = r.ok != 0;
    }
    return out;
}

Pose4x4 Fleet::Pose(int id) const { return id >= 0 && id < n_streams_ ? poses_[(size_t)id] : Pose4x4(); }

bool Fleet::Reset(int id)
{
    if (id < -1 || id >= n_streams_) return false;
    svo_ctx *ctx = tracking_->Context();
    if (ctx && svo_streams_reset(ctx, id) != SVO_OK) { LZB_LOG("ERROR", "svo_streams_reset: %s", svo_last_error(ctx)); return false; }
    for (int s = id < 0 ? 0 : id; s < (id < 0 ? n_streams_ : id + 1); s++) {
        poses_[(size_t)s] = Pose4x4();
        memset(&last_[(size_t)s], 0, sizeof(svo_step_result));
    }
    return true;
}

// ---- run_kitti_stereo a.yaml b.yaml ... --interleave ---------------------------------------------------------------------
static bool read_stereo(const std::string &dataset, int index, cv::Mat &left, cv::Mat &right)
{
    char name[32];
    const char *ext[2] = {"png", "pgm"};
    for (int cam = 0; cam < 2; cam++) {
        bool ok = false;
        for (int e = 0; e < 2 && !ok; e++) {
            snprintf(name, sizeof(name), "/image_%d/%06d.%s", cam, index, ext[e]);
            ok = ReadImageGray(dataset + name, cam == 0 ? left : right);
        }
        if (!ok) return false;
    }
    return true;
}

int RunInterleaved(const std::vector<std::string> &yamls, const std::vector<std::string> &pose_files, int device,
                   std::vector<SequenceReport> *report)
{
    const int n = (int)yamls.size();
    if (n < 1 || pose_files.size() != yamls.size()) return 2;
    static const std::set<std::string> per_sequence = {"dataset_path", "pose_file", "tracks_file", "batch_size", "decode_threads",
                                                       "stream_depth", "fill_features"};
    // everything that can be refused is refused here, on the host, before a context exists
    std::vector<std::string> dataset((size_t)n);
    std::vector<int> len((size_t)n, 0);
    std::map<std::string, std::string> first;
    int w = 0, h = 0;
    for (int s = 0; s < n; s++) {
        if (!Config::SetParameterFile(yamls[(size_t)s])) { fprintf(stderr, "--interleave: unable to open %s\n", yamls[(size_t)s].c_str()); return 2; }
        std::map<std::string, std::string> kv = Config::All();
        dataset[(size_t)s] = Config::Get<std::string>("dataset_path");
        for (const auto &k : per_sequence) kv.erase(k);
        if (s == 0) first = kv;
        else {
            for (const auto &e : first) {
                const auto it = kv.find(e.first);
                if (it == kv.end() || it->second != e.second) {
                    fprintf(stderr, "--interleave: %s and %s differ in key '%s' (%s / %s): the streams of one context share the "
                                    "camera, the rig, track_mode and the tracking parameters\n", yamls[0].c_str(), yamls[(size_t)s].c_str(),
                            e.first.c_str(), e.second.c_str(), it == kv.end() ? "<absent>" : it->second.c_str());
                    return 2;
                }
            }
            for (const auto &e : kv)
                if (!first.count(e.first)) {
                    fprintf(stderr, "--interleave: %s and %s differ in key '%s' (<absent> / %s)\n", yamls[0].c_str(),
                            yamls[(size_t)s].c_str(), e.first.c_str(), e.second.c_str());
                    return 2;
                }
        }
    }
    {
        // image_scale / image_interp are shared keys like every other (compared above); their values are checked here
        double scale; int interp; std::string err;
        if (!Tracking::ReadImageScale(&scale, &interp, &err)) { fprintf(stderr, "--interleave: %s: %s\n", yamls[0].c_str(), err.c_str()); return 2; }
        // ... and so are fast_bucket_width / fast_bucket_height / fast_bucket_keep
        int cw, ch, keep;
        if (!Tracking::ReadFastBuckets(&cw, &ch, &keep, &err)) { fprintf(stderr, "--interleave: %s: %s\n", yamls[0].c_str(), err.c_str()); return 2; }
        // ... and lk_detector / gftt_quality_level / gftt_min_distance
        int det, num; double q, md;
        if (!Tracking::ReadLkDetector(&det, &num, &q, &md, &err)) { fprintf(stderr, "--interleave: %s: %s\n", yamls[0].c_str(), err.c_str()); return 2; }
        // ... and pose_refine / pose_refine_rounds / _iters / _sigma / _min_inliers
        int rmode, rrounds, riters, rmin; double rsigma;
        if (!Tracking::ReadPoseRefine(&rmode, &rrounds, &riters, &rsigma, &rmin, &err)) { fprintf(stderr, "--interleave: %s: %s\n", yamls[0].c_str(), err.c_str()); return 2; }
        // ... and orb_matcher / orb_match_th_stereo / _th_track / _ratio / _radius / orb_max_disparity
        int mmode, mts, mtt; double mra, mrd, mmd;
        int con, cma; double cmd;
        if (!Tracking::ReadTrackCarry(&con, &cmd, &cma, &err)) { fprintf(stderr, "--interleave: %s: %s\n", yamls[0].c_str(), err.c_str()); return 2; }
        // ... and window_ba: the window belongs to the per-frame chain, stream sets have no table yet
        int wf, wr, wi, wm; double ws;
        if (!Tracking::ReadWindowBa(&wf, &wr, &wi, &ws, &wm, &err)) { fprintf(stderr, "--interleave: %s: %s\n", yamls[0].c_str(), err.c_str()); return 2; }
        if (wf) { fprintf(stderr, "--interleave: %s: window_ba: %d with --interleave (the sliding window works on the per-frame chain only)\n", yamls[0].c_str(), wf); return 2; }
        // ... and keyframe: like the window, the keyframe belongs to the per-frame chain
        int kon, kmt, kgap;
        if (!Tracking::ReadKeyframe(&kon, &kmt, &kgap, &err)) { fprintf(stderr, "--interleave: %s: %s\n", yamls[0].c_str(), err.c_str()); return 2; }
        if (kon) { fprintf(stderr, "--interleave: %s: keyframe: 1 with --interleave (keyframe mode works on the per-frame chain only)\n", yamls[0].c_str()); return 2; }
        if (!Tracking::ReadOrbMatcher(&mmode, &mts, &mtt, &mra, &mrd, &mmd, &err)) { fprintf(stderr, "--interleave: %s: %s\n", yamls[0].c_str(), err.c_str()); return 2; }
    }
    for (int s = 0; s < n; s++) {
        cv::Mat l, r;
        if (!read_stereo(dataset[(size_t)s], 0, l, r)) { fprintf(stderr, "--interleave: %s: cannot find images at index 0\n", yamls[(size_t)s].c_str()); return 2; }
        if (s == 0) { w = l.cols; h = l.rows; }
        if (l.cols != w || l.rows != h || r.cols != w || r.rows != h) {
            fprintf(stderr, "--interleave: %s and %s differ in frame size (%dx%d / %dx%d)\n", yamls[0].c_str(), yamls[(size_t)s].c_str(),
                    w, h, l.cols, l.rows);
            return 2;
        }
    }
    std::vector<FILE *> out((size_t)n, nullptr);
    std::vector<bool> alive((size_t)n, true), bad((size_t)n, false);
    for (int s = 0; s < n; s++) {
        if (pose_files[(size_t)s].empty()) continue;
        out[(size_t)s] = fopen(pose_files[(size_t)s].c_str(), "w");
        if (!out[(size_t)s]) {
            fprintf(stderr, "cannot open %s for writing: sequence %s is not run\n", pose_files[(size_t)s].c_str(), yamls[(size_t)s].c_str());
            alive[(size_t)s] = false; bad[(size_t)s] = true;
        }
    }
    const auto t0 = std::chrono::steady_clock::now();
    Fleet fleet(yamls[0], n);
    fleet.SetDevice(device);
    for (int t = 0;; t++) {
        std::vector<std::pair<int, Frame::Ptr>> step;
        for (int s = 0; s < n; s++) {
            if (!alive[(size_t)s]) continue;
            cv::Mat l, r;
            if (!read_stereo(dataset[(size_t)s], t, l, r)) { alive[(size_t)s] = false; continue; }     // the sequence has ended
            Frame::Ptr f = Frame::CreateFrame();
            f->left_img_ = l; f->right_img_ = r;
            step.emplace_back(s, f);
        }
        if (step.empty()) break;
        fleet.Step(step);
        if (fleet.Failed()) {
            for (const auto &e : step) { bad[(size_t)e.first] = true; alive[(size_t)e.first] = false; }
            break;
        }
        for (const auto &e : step) {
            const int s = e.first;
            len[(size_t)s]++;
            if (!out[(size_t)s]) continue;
            const Pose4x4 P = fleet.Pose(s);
            for (int i = 0; i < 12; i++) fprintf(out[(size_t)s], "%.9e%c", P.m[i], i == 11 ? '\n' : ' ');
        }
    }
    const double secs = std::chrono::duration_cast<std::chrono::duration<double>>(std::chrono::steady_clock::now() - t0).count();
    int failed = 0;
    for (int s = 0; s < n; s++) {
        if (out[(size_t)s]) fclose(out[(size_t)s]);
        if (bad[(size_t)s]) failed++;
        if (report) {
            SequenceReport r;
            r.yaml = yamls[(size_t)s]; r.device = device; r.worker = 0; r.frames = len[(size_t)s]; r.seconds = secs; r.ok = !bad[(size_t)s];
            report->push_back(r);
        }
    }
    return failed ? 1 : 0;
}

}  // namespace lzb_vio
