// carry.h -- argument block and launch entry point of the track-carry kernel (carry.hip; internal).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace svo {

constexpr int kCarryCells = 4096;         // grid cells at most: two LDS words each
constexpr int kCarryChunk = 128;          // items per launch (the per-item table is a kernel argument)

// One item = one pair: the previous frame's list (tracks) and the new frame's detections in, the new frame's list out.
// Item b of the step (b = item0 + workgroup) adds b * stride entries to every list pointer, b * n_stride to the count
// pointers and b * cap to the scratch and the per-track id / age lists.
struct CarryMergeArgs {
    int w, h;                             // image size: a tracked point outside [0, w-1] x [0, h-1] is no candidate
    int cell, cols, rows;                 // grid: cell >= min_distance pixels, cols * rows <= kCarryCells
    double min_d2;                        // min_distance^2
    int max_age;                          // 0: unlimited
    int cap, out_cap;                     // list capacity (a detection count above it: no detections), entries written at most
    int item0;
    int64_t stride, n_stride;
    // tracks: t2_left and the keep byte of the circular LK, the previous list's response / id / age
    const float2 *q; const uint8_t *keep;
    const float *p_resp; const long long *p_id; const int *p_age;
    const int *p_n; int n_trk;            // device count (clamped to cap), or null -> n_trk
    // detections
    const float2 *d_xy; const float *d_resp;
    const int *d_n; int n_det;            // device count, or null -> n_det
    // the merged list (o_xy / o_resp may be d_xy / d_resp: the detections are staged first)
    float2 *o_xy; float *o_resp; long long *o_id; int *o_age;
    int *o_src;                           // null, or: track index / n_trk + detection index per entry
    int *o_n, *o_carried;                 // list length; carried points (may be null)
    // ids and ages-at-t1 of the pair's tracks in compact_kernel's order (may be null)
    long long *trk_id; int *trk_age;
    // id counters: item t of the launch uses next_id[cnt[t]]; null: next0, nothing written back
    long long *next_id; long long next0;
    // scratch, cap entries per item
    int *sorted; uint8_t *flag, *dflag; float2 *s_dxy; float *s_dresp;
    int32_t cnt[kCarryChunk];
    uint8_t fresh[kCarryChunk];           // the previous list has no ids yet: numbered next_id.. in list order, age 0
    uint8_t restart[kCarryChunk];         // the counter restarts at 0 (first frame of a chain / after a reset)
};
// n_items <= kCarryChunk
void launch_carry_merge(const CarryMergeArgs &a, int n_items, hipStream_t st);
// the smallest integer cell size >= min_distance whose grid over w x h fits kCarryCells
void carry_grid(int w, int h, double min_distance, int *cell, int *cols, int *rows);

}  // namespace svo
