// keyframe.h -- argument blocks and launch entry points of the keyframe kernels (keyframe.hip; internal).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/svo_abi.h"
#include "svo_kernels.h"

namespace svo {

constexpr int kKfTrip = 4096;             // table ids staged in LDS per trip (32 KB)

// The state of a chain's keyframe (rules K1-K8 of include/svo_abi.h); its table (ids, X) lies beside it.
struct KfState {
    int valid, kf_index, n_rows, _pad;
    double pose_K[16], inv_K[16];
};

// K2: the merge of the table's ids with a pair's track ids.  A count comes from the device where its pointer is set.
struct KeyframeJoinArgs {
    const long long *tab_ids; const float *tab_X; const int *tab_n; int n_rows, rows_cap;     // n_rows clamped to 0..rows_cap
    const long long *trk_ids; const float2 *trk_xy; const int *trk_n; int n_trk, trk_cap;     // likewise
    const int *valid; int clear;          // fused: the state's flag, and K1's clear decided on the host; not valid = no rows
    int min_tracks;                       // K3: counts[1] = n_join where it reaches min_tracks, else 0 (what the solve sees)
    float *o_X; float2 *o_xy; int *o_trk, *o_row; long long *o_id;      // o_id may be null
    int out_cap;
    int *counts;                          // [0] n_join, [1] (where min_tracks > 0) the solve's point count
};
void launch_keyframe_join(const KeyframeJoinArgs &a, hipStream_t st);

// K4-K6 on the step's record, the keyframe solve's record and the pair's lists.
struct KeyframeUpdateArgs {
    KfState *state; long long *tab_ids; float *tab_X;
    int clear, index_b, min_tracks, max_gap, cap;
    double pose_a[16];
    double inlier_rate, max_move2;
    svo_step_result *rec; const PnpRecord *pnp; const int *counts;
    const long long *trk_ids; const float *tri; const int *trk_n;
    svo_keyframe_result *res;
};
void launch_keyframe_update(const KeyframeUpdateArgs &a, hipStream_t st);

}  // namespace svo
