// window.h -- argument block and launch entry point of the sliding window's table update (window.hip; internal).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/svo_abi.h"
#include "refine_device.h"

namespace svo {

constexpr int kWindowMaxFrames = 8;       // SVO_WINDOW_MAX_FRAMES: observation columns per row
constexpr int kWindowPose = 12;           // doubles per slot: R row-major, then t  (Y = R X + t)

// The landmark table as device pointers (svo_window_table of the ABI): counts = { n frames, m rows, rows needed, 0 }.
struct WindowTable {
    int *counts;
    double *poses;                        // kWindowMaxFrames x kWindowPose
    long long *ids;                       // m rows, strictly ascending
    double *X;                            // 3 per row, world
    uint32_t *seen, *active;              // bit s = slot s
    float2 *obs_left, *obs_right;         // kWindowMaxFrames per row
};

// One step with ok = 1 on pair a -> b: `in` (read only) + the pair's tracks -> `out`; the two must not overlap.
struct WindowUpdateArgs {
    int frames;                           // W, 2 .. kWindowMaxFrames
    int cap;                              // rows both tables have room for
    WindowTable in, out;
    // the pair's tracks in compact_kernel's order: ids strictly ascending
    const float2 *t1_left, *t1_right, *t2_left, *t2_right;
    const long long *ids;
    const float *tri;                     // 3 floats per track: the point triangulated in frame a
    int n_trk;
    const double *pose_a, *pose_b;        // 4 x 4 row-major, world from camera: frame_pose_ before the step, the record's pose
    // the fused step (all null / 0 in a stage call): the pair's track count on the device (clamped to n_trk), the record's ok
    // (0: the table is cleared, T1), `in` counts as cleared, pose_a handed over by value
    const int *n_trk_dev; const int *ok; int clear_in; int pose_a_by_value; double pose_a_value[16];
    // scratch: cap + 1 and n_trk + 1 ints
    int *pre_rows, *pre_new;
};
void launch_window_update(const WindowUpdateArgs &a, hipStream_t st);

// ---- the optimiser over a table (svo_window_ba)
constexpr int kWbaThreads = 1024;         // one workgroup; lanes stride the landmarks
constexpr int kWbaDim = 6 * (kWindowMaxFrames - 1);      // the reduced system at most: 42
constexpr int kWbaRow = 10 + 18 * (kWindowMaxFrames - 1);    // doubles a landmark keeps between the passes: L (6) y (3) ok | T_if (6 x 3) per slot >= 1

struct WindowBaArgs {
    WindowTable tab;                      // poses, X and active are overwritten when the outcome is SVO_REFINE_APPLIED
    int cap;                              // rows the table and the scratch have room for
    StereoCam cam;
    int rounds, iters, min_obs; double sigma;
    svo_window_result *res;
    double *Xa, *Xb;                      // the accepted and the trial points, swapped by pointer: 3 x cap doubles each
    double *sys;                          // cap x kWbaRow
    uint32_t *act;                        // the active mask of every row while the kernel runs
    double *record_pose;                  // null, or: the step record's 4 x 4 pose, overwritten with inverse(newest slot) when applied
};
void launch_window_ba(const WindowBaArgs &a, hipStream_t st);

}  // namespace svo
