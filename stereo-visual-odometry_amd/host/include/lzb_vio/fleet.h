// fleet.h -- additive: many independent live stereo streams behind ONE HIP context (svo_streams_*, include/svo_abi.h).
//
// The reference feeds one camera: System::Step_ros(Frame::Ptr) hands a frame to Tracking::AddFrame and blocks until its pose
// exists (reference src/System.cpp:60-74).  A vehicle with several stereo rigs, or a server that plays N logs at wall-clock
// rate, would run N Systems and N one-pair steps, each a chain of latency-bound launches on an almost empty chip.  A Fleet
// keeps what N Tracking objects keep (last frame's features, frame_pose_, INITING / TRACKING) in ONE context's stream set and
// advances any subset of the streams by one frame each with one set of launches; every stream's poses are byte for byte
// what its own System would produce.  All streams share the YAML (camera, rig, track_mode, tracking parameters) and the
// frame size.  System and its reference-shaped surface are unchanged.
#pragma once
#ifndef lzb_vio_FLEET_H
#define lzb_vio_FLEET_H

#include "lzb_vio/System.h"

namespace lzb_vio {

class Fleet {
public:
    // max_step: the most streams one Step advances (0: all of them); the context is sized for it at the first Step
    Fleet(const std::string &config_path, int n_streams, int max_step = 0);
    ~Fleet();
    Fleet(const Fleet &) = delete;
    Fleet &operator=(const Fleet &) = delete;

    // One frame for each named stream (distinct ids, any order, any subset of at most max_step).  Returns, per entry, what
    // Step_ros returns for that frame on a System of its own: true for a stream's first frame and for a tracked pair, false
    // where Tracking::Track() returned false (the stream's pose then keeps its value).  A hard error (bad id, a frame of
    // another size, a HIP failure) makes every entry false and sets Failed().
    std::vector<bool> Step(const std::vector<std::pair<int, Frame::Ptr>> &frames);
    Pose4x4 Pose(int id) const;                              // frame_pose_ of the stream (identity before its first pair)
    bool Reset(int id = -1);                                 // that stream (-1: all) back to INITING, pose = identity
    const svo_step_result &LastResult(int id) const { return last_[(size_t)id]; }
    int Streams() const { return n_streams_; }
    int MaxStep() const { return max_step_; }
    bool Failed() const { return failed_; }
    void SetDevice(int device) { tracking_->SetDevice(device); }     // before the first Step; default 0

private:
    Parameter::Ptr parameter_ = nullptr;
    Sensors::Ptr sensors_ = nullptr;
    Tracking::Ptr tracking_ = nullptr;                       // owns the context; its own online state is not used
    int n_streams_ = 0, max_step_ = 0;
    int w_ = 0, h_ = 0, pitch_ = 0;
    uint8_t *pin_[2] = {nullptr, nullptr};                   // page-locked left / right frames of one Step
    bool failed_ = false;
    std::vector<Pose4x4> poses_;
    std::vector<svo_step_result> last_;
};

// `run_kitti_stereo a.yaml b.yaml ... --poses-dir DIR --interleave`: the listed sequences become the streams of ONE Fleet on
// one device and are stepped in lockstep -- frame t of every sequence that still has one; a sequence that ends drops out.
// The YAMLs must agree in everything but the per-sequence keys (dataset_path, pose_file, tracks_file, batch_size,
// decode_threads, stream_depth, fill_features) and the sequences in frame size: otherwise the key that differs is named
// and 2 is returned BEFORE any device is touched.  pose_files[i] (may be empty) receives sequence i's poses, byte for byte
// what `run_kitti_stereo <yaml i>` writes.  Returns 0, 1 when a sequence could not be run to its end, 2 on a refused set.
int RunInterleaved(const std::vector<std::string> &yamls, const std::vector<std::string> &pose_files, int device,
                   std::vector<SequenceReport> *report);

}  // namespace lzb_vio
#endif
