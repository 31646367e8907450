// chain_stages.h -- the stages that ride on svo_add_frame's online chain (internal): their state, the plan of a step and the
// record of the last launch.  A new follower stage adds its struct here, a flag to OnlineStep and to LastLaunch, and a column
// to chain_event's rule table (pipeline.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>
#include "../../include/svo_abi.h"

// A block of device memory that appears when a feature is first used and grows with the largest request: dev_reserve
// (svo_ctx.h; defined here because the stages below own such blocks).
struct DevScratch {
    uint8_t *base = nullptr;
    size_t bytes = 0;
};

// Each stage keeps its configuration, its device block and ONE lifecycle flag -- "the next step starts fresh" -- which only
// chain_event (pipeline.hip) sets and only the stage's fused step clears.

// Track carry (svo_set_track_carry / svo_carry_merge, carry.hip; off and nothing allocated until it is first enabled)
struct CarryStage {
    bool on = false;
    double min_distance = 3.0;
    int max_age = 0;
    uint8_t *buf = nullptr;                              // ONE block, cut into what follows
    long long *kp_id = nullptr; int *kp_age = nullptr;   // beside kp_xy / kp_resp: n_img frame slots x max_keypoints
    long long *trk_id = nullptr; int *trk_age = nullptr; // id / age-at-t1 of a pair's tracks, in the order of cmp[]: max_batch x max_keypoints
    int *sorted = nullptr; uint8_t *flag = nullptr, *dflag = nullptr;       // kernel scratch, max_batch x max_keypoints
    float2 *dxy = nullptr; float *dresp = nullptr;
    long long *next = nullptr;                           // the online chain's id counter, on the device
    bool ids[2] = {false, false};                        // the list in online ring slot 0 / 1 has ids
    bool restart = true;                                 // the online chain's ids start at 0 with its next carry launch
    DevScratch stage;                                    // svo_carry_merge: the caller's lists, the outputs and the scratch
};

// Sliding window (svo_set_window_ba / svo_window_update / svo_window_ba, window.hip): nothing allocated until it is first used
struct WindowStage {
    int frames = 0;                                      // W; 0: off
    int rounds = 4, iters = 5, min_obs = 10; double sigma = 1.0;
    DevScratch block;                                    // the online chain's table (two buffers, swapped per step) and the optimiser's scratch
    int cur = 0;                                         // which of the two tables is the chain's
    bool clear = true;                                   // the next step starts from a cleared table
    DevScratch update_stage;                             // svo_window_update: the caller's tables and tracks (HOST calls) and the kernel's prefix scratch
    DevScratch ba_stage;                                 // svo_window_ba's own: a growing stage call never frees what the other one's launch still reads
};

// Keyframe-relative pose (svo_set_keyframe / svo_keyframe_join, keyframe.hip; off and nothing allocated until it is first enabled)
struct KeyframeStage {
    bool on = false;
    int min_tracks = 60, max_gap = 0;
    uint8_t *buf = nullptr;                              // ONE block: the chain's state, its table, the joined lists, the result
    bool clear = true;                                   // the next step starts without a keyframe
    DevScratch stage;                                    // svo_keyframe_join: the caller's lists and the outputs (HOST calls)
};

// Which follower stages an online step runs behind its pair: built by pipeline_add_frame, handed down to the pose stage.
struct OnlineStep { bool window = false, keyframe = false; };

// What the last fused launch ran -- what the read-backs may return (read_back_ready, svo_abi.hip).  Written once per launch, by
// the pose stage (run_back, pipeline.hip) when everything is queued.  The follower fields speak of the last svo_add_frame step:
// a batch or a stream-set launch touches neither stage and leaves them alone.
struct LastLaunch {
    int pairs = 0;                                       // pairs of the launch
    bool carry = false;                                  // track carry ran on them
    int refine_mode = SVO_REFINE_OFF;                    // the refinement stage's mode (OFF: it did not run)
    int window_frames = 0;                               // the sliding window's W (0: it did not run)
    bool keyframe = false;                               // the keyframe stage ran
};
