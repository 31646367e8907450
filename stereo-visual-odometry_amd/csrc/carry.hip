// carry.hip -- track carry (svo_set_track_carry / svo_carry_merge): the list a frame hands to the next pair is the points
// the circular LK has just tracked into it, under the ids they already have, followed by the frame's fresh detections
// that do not crowd them.  The rules (C1-C8 of include/svo_abi.h):
//
//   candidate  : keep byte set, t2_left inside the image, age + 1 <= max_age
//   near(a, b) : dx, dy in float, dx*dx + dy*dy in double < min_distance^2
//   carried    : candidate i with no candidate j < i near it (index rule: parallel, the older track wins)
//   detection  : kept unless a CARRIED point is near it
//   list       : carried points in track order (id kept, age + 1), then kept detections (new ids, age 0), cut at capacity
//
// One workgroup of 1024 lanes per item.  The candidates are binned into a grid whose cell is at least min_distance wide
// and small enough for LDS (a counting sort: count, scan, scatter), so both tests read 3 x 3 cells; the outputs leave in
// stable order through ballot-free block scans.  Nothing here is tuned: the kernel runs once per step on a few thousand
// points.
#include "carry.h"
#include "svo_device.h"

namespace svo {

__device__ inline bool carry_near(float2 a, float2 b, double min_d2)
{
    const float dx = a.x - b.x, dy = a.y - b.y;
    return (double)dx * (double)dx + (double)dy * (double)dy < min_d2;       // the products are exact: one rounding
}

// cell coordinate of a pixel coordinate, -1 .. n: exact integer arithmetic (a float quotient could round across a cell border)
__device__ inline int carry_cell(float v, int cell, int extent)
{
    const float lo = -(float)cell, hi = (float)(extent - 1 + cell);
    const float c = fminf(fmaxf(v, lo), hi);                                 // (a NaN lands on lo: it is near nothing anyway)
    return ((int)floorf(c) + cell) / cell - 1;
}

__global__ __launch_bounds__(1024) void carry_merge_kernel(CarryMergeArgs a)
{
    __shared__ int cell_start[kCarryCells];      // first entry of the cell in sorted[]
    __shared__ int cell_end[kCarryCells];        // counts, then the scatter cursor: one past the cell's last entry
    __shared__ int wave_tot[16];
    const int t = blockIdx.x, tid = threadIdx.x;
    if (t >= kCarryChunk) return;
    const int b = a.item0 + t;
    const int64_t o = (int64_t)b * a.stride, so = (int64_t)b * a.cap;
    int n_p = a.p_n ? a.p_n[(int64_t)b * a.n_stride] : a.n_trk;
    n_p = n_p < 0 ? 0 : (n_p > a.cap ? a.cap : n_p);                          // what the LK launch tracked
    int n_d = a.d_n ? a.d_n[(int64_t)b * a.n_stride] : a.n_det;
    if (n_d < 0 || n_d > a.cap) n_d = 0;                                     // C7: a truncated detection contributes nothing
    const bool fresh = a.fresh[t] != 0;
    long long next = a.next_id ? (a.restart[t] ? 0 : a.next_id[a.cnt[t]]) : a.next0;
    const long long id0 = next;                                              // fresh: track i has id id0 + i
    if (fresh) next += n_p;
    const int ncells = a.cols * a.rows;
    const float wm1 = (float)(a.w - 1), hm1 = (float)(a.h - 1);
    const float2 *q = a.q + o;
    const uint8_t *keep = a.keep + o;
    int *sorted = a.sorted + so;
    uint8_t *flag = a.flag + so, *dflag = a.dflag + so;
    float2 *s_dxy = a.s_dxy + so;
    float *s_dresp = a.s_dresp + so;

    // ---- stage the detections (the merged list may overwrite them), count the candidates per cell
    for (int c = tid; c < ncells; c += 1024) cell_end[c] = 0;
    for (int k = tid; k < n_d; k += 1024) { s_dxy[k] = a.d_xy[o + k]; s_dresp[k] = a.d_resp[o + k]; }
    __syncthreads();
    for (int i = tid; i < n_p; i += 1024) {
        const float2 p = q[i];
        const int age = fresh ? 0 : a.p_age[o + i];
        const bool cand = keep[i] != 0 && p.x >= 0.f && p.x <= wm1 && p.y >= 0.f && p.y <= hm1 && (a.max_age == 0 || age < a.max_age);
        flag[i] = cand ? 1 : 0;
        if (cand) atomicAdd(&cell_end[((int)p.y / a.cell) * a.cols + (int)p.x / a.cell], 1);
    }
    __syncthreads();
    {
        int v[4], sum = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) { const int c = 4 * tid + k; v[k] = c < ncells ? cell_end[c] : 0; sum += v[k]; }
        int total;
        int run = block1024_excl_scan(sum, wave_tot, total);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int c = 4 * tid + k;
            if (c < ncells) { cell_start[c] = run; cell_end[c] = run; }
            run += v[k];
        }
    }
    __syncthreads();
    for (int i = tid; i < n_p; i += 1024) {
        if (!flag[i]) continue;
        const float2 p = q[i];
        sorted[atomicAdd(&cell_end[((int)p.y / a.cell) * a.cols + (int)p.x / a.cell], 1)] = i;
    }
    __syncthreads();

    // ---- C3: carried = no earlier candidate near (whether that one is carried or not)
    for (int i = tid; i < n_p; i += 1024) {
        if (!flag[i]) continue;
        const float2 p = q[i];
        const int cx = (int)p.x / a.cell, cy = (int)p.y / a.cell;
        bool carried = true;
        for (int yy = max(cy - 1, 0); yy <= min(cy + 1, a.rows - 1); yy++)
            for (int xx = max(cx - 1, 0); xx <= min(cx + 1, a.cols - 1); xx++) {
                const int c = yy * a.cols + xx;
                for (int e = cell_start[c]; e < cell_end[c]; e++) {
                    const int j = sorted[e];
                    if (j < i && carry_near(q[j], p, a.min_d2)) carried = false;
                }
            }
        if (carried) flag[i] = 2;                 // (nobody reads another point's flag in this pass)
    }
    __syncthreads();

    // ---- C4: a detection stays unless a carried point is near it
    for (int k = tid; k < n_d; k += 1024) {
        const float2 d = s_dxy[k];
        const int cx = carry_cell(d.x, a.cell, a.w), cy = carry_cell(d.y, a.cell, a.h);
        bool kept = true;
        for (int yy = max(cy - 1, 0); yy <= min(cy + 1, a.rows - 1); yy++)
            for (int xx = max(cx - 1, 0); xx <= min(cx + 1, a.cols - 1); xx++) {
                const int c = yy * a.cols + xx;
                for (int e = cell_start[c]; e < cell_end[c]; e++) {
                    const int j = sorted[e];
                    if (flag[j] == 2 && carry_near(q[j], d, a.min_d2)) kept = false;
                }
            }
        dflag[k] = kept ? 1 : 0;
    }
    __syncthreads();

    // ---- C5: the carried points in track order; beside them the ids / ages of the pair's tracks in compact_kernel's order
    int n_carried = 0, n_tracks = 0;
    for (int start = 0; start < n_p; start += 1024) {
        const int i = start + tid;
        const bool in = i < n_p;
        const bool c = in && flag[i] == 2, k = in && keep[i] != 0;
        int tot_c, tot_k;
        const int rc = block1024_excl_scan(c ? 1 : 0, wave_tot, tot_c);
        const int rk = block1024_excl_scan(k ? 1 : 0, wave_tot, tot_k);
        if (k || c) {
            const long long id = fresh ? id0 + i : a.p_id[o + i];
            const int age = fresh ? 0 : a.p_age[o + i];
            if (k && a.trk_id) { a.trk_id[so + n_tracks + rk] = id; a.trk_age[so + n_tracks + rk] = age; }
            if (c) {
                const int dst = n_carried + rc;                     // < n_p <= out_cap
                a.o_xy[o + dst] = q[i]; a.o_resp[o + dst] = a.p_resp[o + i];
                a.o_id[o + dst] = id; a.o_age[o + dst] = age + 1;
                if (a.o_src) a.o_src[o + dst] = i;
            }
        }
        n_carried += tot_c; n_tracks += tot_k;
    }
    // ---- then the kept detections under new ids; what does not fit gets none
    int n_kept = 0;
    for (int start = 0; start < n_d; start += 1024) {
        const int k = start + tid;
        const bool kp = k < n_d && dflag[k] != 0;
        int tot;
        const int r = block1024_excl_scan(kp ? 1 : 0, wave_tot, tot);
        const int dst = n_carried + n_kept + r;
        if (kp && dst < a.out_cap) {
            a.o_xy[o + dst] = s_dxy[k]; a.o_resp[o + dst] = s_dresp[k];
            a.o_id[o + dst] = next + n_kept + r; a.o_age[o + dst] = 0;
            if (a.o_src) a.o_src[o + dst] = n_p + k;
        }
        n_kept += tot;
    }
    if (tid == 0) {
        const int n_out = min(n_carried + n_kept, a.out_cap);
        a.o_n[(int64_t)b * a.n_stride] = n_out;
        if (a.o_carried) a.o_carried[(int64_t)b * a.n_stride] = n_carried;
        if (a.next_id) a.next_id[a.cnt[t]] = next + (n_out - n_carried);
    }
}

void launch_carry_merge(const CarryMergeArgs &a, int n_items, hipStream_t st)
{
    if (n_items <= 0) return;
    hipLaunchKernelGGL(carry_merge_kernel, dim3(n_items), dim3(1024), 0, st, a);
}

void carry_grid(int w, int h, double min_distance, int *cell, int *cols, int *rows)
{
    int c = (int)min_distance;
    if ((double)c < min_distance) c++;
    if (c < 1) c = 1;
    while ((int64_t)((w + c - 1) / c) * ((h + c - 1) / c) > kCarryCells) c++;
    *cell = c; *cols = (w + c - 1) / c; *rows = (h + c - 1) / c;
}

}  // namespace svo
