// gftt.hip -- Shi-Tomasi corners, cv::goodFeaturesToTrack(img, maxCorners, qualityLevel, minDistance, noArray(), 3, false, 0.04)
// as cv::GFTTDetector::detect calls it (reference src/tracking.cpp:18 builds GFTTDetector::create(n, 0.01, 20) and never uses
// it), for gfx950.  The recipe is stated in include/svo_abi.h and DESIGN.md; tests/_gftt_ref.py is its numpy twin and every
// stage here equals it bit for bit.  Batched over the images of a step, three launches:
//   gftt_eigen_kernel  : one 64x16 pixel tile per 256-thread workgroup.  The image tile (+3: Sobel 1, box 1, local-max ring 1)
//       is staged in LDS once with the image's reflect-101 border applied; dx, dy are computed at IN-IMAGE positions of the
//       tile + 2 and kept in LDS; the three 3x3 box sums are taken out of LDS in double over the float products, the indices of
//       the PRODUCTS reflected (the box filter's border is that of the covariance maps, where dx keeps its sign); the minimal
//       eigenvalue of the tile + 1 stays in LDS for the 3x3 local-maximum test, which does not depend on the threshold.  To HBM
//       goes one float per pixel -- the eigenvalue where the pixel is an interior local maximum, -inf elsewhere -- and one
//       integer atomic max per workgroup (the image's largest eigenvalue, as an order-preserving unsigned key).
//   gftt_emit_kernel   : thr = float(double(max) * double(qualityLevel)); every map entry > thr is appended to the image's
//       candidate list as the 64-bit key (eigenvalue key << 32 | raster index) -- one global atomic per workgroup of eight
//       rows; the order of the list is free because the key is a total order.
//   gftt_select_kernel : one workgroup per image.  Bitonic sort of the keys, descending (eigenvalue descending, ties to the
//       larger raster index: 3.4's greaterThanPtr), in LDS up to 4096 keys, in the list itself above; then the greedy
//       minDistance pass by ONE wave with the grid of kept corners in LDS (device memory for large grids): 64 consecutive
//       candidates are tested against the grid in parallel, the survivors are resolved among themselves in order (ballot, the
//       lowest live lane is kept and retires the later lanes it is too close to).
#include <math.h>
#include "svo_device.h"
#include "svo_kernels.h"

namespace svo {

constexpr int kGTileW = 64, kGTileH = 16;
constexpr int kGRawW = kGTileW + 6, kGRawH = kGTileH + 6;      // 70 x 22: image, reflect-101
constexpr int kGDW = kGTileW + 4, kGDH = kGTileH + 4;          // 68 x 20: dx, dy
constexpr int kGEW = kGTileW + 2, kGEH = kGTileH + 2;          // 66 x 18: eigenvalues
constexpr int kGfttLdsKeys = 4096;                             // 32 KB
constexpr int kGfttLdsCells = 1536;                            // 24 KB
// Kept corners one grid cell can hold.  The cell side is cvRound(minDistance) <= minDistance + 0.5 pixels, so the integer
// coordinates of a cell span a square of side s <= minDistance - 0.5 < minDistance.  Cut it into four closed quadrants of
// side s / 2: two points of one quadrant are at most s / sqrt(2) < minDistance apart, so a quadrant holds at most one kept
// corner (kept corners are >= minDistance apart) and the cell at most FOUR.
constexpr int kGfttCellCap = 4;
constexpr unsigned kCellEmpty = 0xFFFFFFFFu;
// What kp_resp holds for a Shi-Tomasi corner: a value no FAST score (an 8-bit integer >= 0) can take, so a frame's list says
// which detector made it wherever it travels (the stream store, a carried frame).  svo_get_frame_keypoints turns it into the
// record GFTTDetector::detect makes (size 3, response 0).
constexpr float kGfttRespTag = -1.f;

// float -> unsigned, order preserving (and back)
__device__ __forceinline__ unsigned f2key(float f)
{
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key2f(unsigned k)
{
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

__global__ __launch_bounds__(256) void gftt_eigen_kernel(GfttArgs a)
{
    __shared__ uint8_t raw[kGRawH * kGRawW];
    __shared__ float sdx[kGDH * kGDW], sdy[kGDH * kGDW];
    __shared__ float seig[kGEH * kGEW];
    __shared__ unsigned s_max;
    const int b = blockIdx.z;
    const uint8_t *img = a.img + (int64_t)b * a.img_stride;
    float *map = a.map + (int64_t)b * a.map_stride;
    const int x0 = blockIdx.x * kGTileW, y0 = blockIdx.y * kGTileH;
    const int tid = threadIdx.x;
    const int w = a.w, h = a.h;
    if (tid == 0) s_max = 0u;
    // image tile + 3, border reflect-101 (positions further than one pixel outside the image are never used: clamped)
    for (int i = tid; i < kGRawH * kGRawW; i += 256) {
        const int ry = i / kGRawW, rx = i - ry * kGRawW;
        const int gx = min(w - 1, max(0, refl101(min(w, max(-1, x0 - 3 + rx)), w)));
        const int gy = min(h - 1, max(0, refl101(min(h, max(-1, y0 - 3 + ry)), h)));
        raw[i] = img[(int64_t)gy * a.pitch + gx];
    }
    __syncthreads();
    const float s = (float)(1.0 / (4.0 * 3.0 * 255.0));
    const float f0 = 2.f * s, f1 = s;
    // dx, dy at the in-image positions of tile + 2
    for (int i = tid; i < kGDH * kGDW; i += 256) {
        const int dyi = i / kGDW, dxi = i - dyi * kGDW;
        const int gx = x0 - 2 + dxi, gy = y0 - 2 + dyi;
        float vx = 0.f, vy = 0.f;
        if (gx >= 0 && gx < w && gy >= 0 && gy < h) {
            const uint8_t *p = &raw[(dyi + 1) * kGRawW + dxi + 1];
            const int r0 = (int)p[1] - (int)p[-1];
            const int rm = (int)p[-kGRawW + 1] - (int)p[-kGRawW - 1];
            const int rp = (int)p[kGRawW + 1] - (int)p[kGRawW - 1];
            const float t0 = (float)r0 * f0, t1 = (float)(rm + rp) * f1;
            vx = t0 + t1;
            const float qa0 = (float)(int)p[kGRawW] * f0, qa1 = (float)((int)p[kGRawW - 1] + (int)p[kGRawW + 1]) * f1;
            const float qb0 = (float)(int)p[-kGRawW] * f0, qb1 = (float)((int)p[-kGRawW - 1] + (int)p[-kGRawW + 1]) * f1;
            const float qa = qa0 + qa1, qb = qb0 + qb1;
            vy = qa - qb;
        }
        sdx[i] = vx; sdy[i] = vy;
    }
    __syncthreads();
    // minimal eigenvalue at the in-image positions of tile + 1 (-inf outside: such a neighbour never wins)
    unsigned kmax = 0u;
    for (int i = tid; i < kGEH * kGEW; i += 256) {
        const int ey = i / kGEW, ex = i - ey * kGEW;
        const int gx = x0 - 1 + ex, gy = y0 - 1 + ey;
        float e = -INFINITY;
        if (gx >= 0 && gx < w && gy >= 0 && gy < h) {
            // the order of a box filter: the three products of a row first, (p0 + p1) + p2, then the rows, (r0 + r1) + r2
            double sxx = 0.0, sxy = 0.0, syy = 0.0;
#pragma unroll
            for (int j = -1; j <= 1; j++) {
                const int ny = refl101(gy + j, h) - (y0 - 2);
                double rxx = 0.0, rxy = 0.0, ryy = 0.0;
#pragma unroll
                for (int k = -1; k <= 1; k++) {
                    const int nx = refl101(gx + k, w) - (x0 - 2);
                    const float vx = sdx[ny * kGDW + nx], vy = sdy[ny * kGDW + nx];
                    const float pxx = vx * vx, pxy = vx * vy, pyy = vy * vy;
                    rxx = k == -1 ? (double)pxx : rxx + (double)pxx;
                    rxy = k == -1 ? (double)pxy : rxy + (double)pxy;
                    ryy = k == -1 ? (double)pyy : ryy + (double)pyy;
                }
                sxx = j == -1 ? rxx : sxx + rxx; sxy = j == -1 ? rxy : sxy + rxy; syy = j == -1 ? ryy : syy + ryy;
            }
            const float fa = (float)sxx * 0.5f, fb = (float)sxy, fc = (float)syy * 0.5f;
            const float d = fa - fc;
            const float dd = d * d, bb = fb * fb;
            const float rad = dd + bb;
            const float ac = fa + fc;
            e = ac - sqrtf(rad);
            // the image's maximum is taken over the tile's own pixels (every pixel of the image belongs to one tile)
            if (ex >= 1 && ex <= kGTileW && ey >= 1 && ey <= kGTileH) kmax = max(kmax, f2key(e));
        }
        seig[i] = e;
    }
    for (int o = 32; o > 0; o >>= 1) kmax = max(kmax, (unsigned)__shfl_xor((int)kmax, o));
    __syncthreads();
    if ((tid & 63) == 0 && kmax) atomicMax(&s_max, kmax);
    // out: the whole map (svo_min_eigen_map), or the eigenvalue of interior local maxima and -inf elsewhere
#pragma unroll
    for (int j = 0; j < kGTileH / 4; j++) {
        const int lx = tid & 63, ly = (tid >> 6) + 4 * j;
        const int gx = x0 + lx, gy = y0 + ly;
        if (gx < w && gy < h) {
            const float *p = &seig[(ly + 1) * kGEW + lx + 1];
            float v = p[0];
            if (!a.full) {
                const bool cand = gx >= 1 && gx <= w - 2 && gy >= 1 && gy <= h - 2 &&
                                  v >= p[-1] && v >= p[1] && v >= p[-kGEW - 1] && v >= p[-kGEW] && v >= p[-kGEW + 1] &&
                                  v >= p[kGEW - 1] && v >= p[kGEW] && v >= p[kGEW + 1];
                if (!cand) v = -INFINITY;
            }
            map[(int64_t)gy * a.mpitch + gx] = v;
        }
    }
    __syncthreads();
    if (tid == 0 && s_max) atomicMax(&a.maxkey[b], s_max);
}

// kEmitRows image rows per 256-lane workgroup, two passes over them (the second one out of L2): count the candidates, reserve
// the workgroup's range of the image's list with ONE global atomic, then write with a running offset in LDS (one LDS atomic
// per wave and 256 pixels).  One atomic per wave on the image's counter instead -- ~5 000 returning atomics on one address per
// KITTI-size image -- made this kernel 4.7 ms of a 256-pair step; the list order is free either way.
constexpr int kEmitRows = 8;
__global__ __launch_bounds__(256) void gftt_emit_kernel(GfttArgs a)
{
    __shared__ int s_count, s_base;
    const int b = blockIdx.y, y0 = blockIdx.x * kEmitRows, y1 = min(a.h, y0 + kEmitRows);
    const int tid = threadIdx.x, lane = tid & 63;
    const float mx = key2f(a.maxkey[b]);
    const float thr = (float)((double)mx * a.quality);
    const float *map = a.map + (int64_t)b * a.map_stride;
    if (tid == 0) s_count = 0;
    __syncthreads();
    int mine = 0;
    for (int y = y0; y < y1; y++)
        for (int x = tid; x < a.w; x += 256) mine += map[(int64_t)y * a.mpitch + x] > thr ? 1 : 0;
    const int wsum = wave_sum_i32(mine);
    if (lane == 0 && wsum) atomicAdd(&s_count, wsum);
    __syncthreads();
    const int cnt = s_count;
    if (cnt == 0) return;                        // (the whole workgroup)
    __syncthreads();
    if (tid == 0) { s_base = atomicAdd(&a.n_cand[b], cnt); s_count = 0; }
    __syncthreads();
    const int base = s_base;
    unsigned long long *keys = a.keys + (int64_t)b * a.keys_stride;
    const int wpad = (a.w + 255) & ~255;         // every lane of a wave makes the same trips: the ballot sees whole waves
    for (int y = y0; y < y1; y++) {
        for (int x0 = 0; x0 < wpad; x0 += 256) {
            const int x = x0 + tid;
            const float v = x < a.w ? map[(int64_t)y * a.mpitch + x] : -INFINITY;
            const bool cand = v > thr;
            const unsigned long long m = __ballot(cand);
            if (m == 0) continue;
            int off = 0;
            if (lane == 0) off = atomicAdd(&s_count, __popcll(m));
            off = __builtin_amdgcn_readfirstlane(off);
            if (cand) {
                const int idx = base + off + __popcll(m & ((1ull << lane) - 1ull));
                if (idx < a.cap) keys[idx] = ((unsigned long long)f2key(v) << 32) | (unsigned)(y * a.w + x);
            }
        }
    }
}

template <bool kLdsCells>
__global__ __launch_bounds__(1024) void gftt_select_kernel(GfttArgs a)
{
    __shared__ unsigned long long lds_keys[kGfttLdsKeys];
    __shared__ unsigned lds_cells[kLdsCells ? kGfttCellCap * kGfttLdsCells : 4];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int n = a.n_cand[b];
    int *n_out = a.n_out + b;
    if (n > a.cap || n <= 0) {                   // over capacity: the count says so (SVO_FAIL_CAPACITY / SVO_ERR_ARG), no list
        if (tid == 0) *n_out = n;
        return;
    }
    int P = 64;
    while (P < n) P <<= 1;                       // <= keys_stride (a power of two >= cap)
    unsigned long long *gk = a.keys + (int64_t)b * a.keys_stride;
    unsigned long long *K = P <= kGfttLdsKeys ? lds_keys : gk;
    if (P <= kGfttLdsKeys) { for (int i = tid; i < P; i += 1024) lds_keys[i] = i < n ? gk[i] : 0ull; }
    else { for (int i = n + tid; i < P; i += 1024) gk[i] = 0ull; }
    unsigned *cells = kLdsCells ? lds_cells : (unsigned *)(a.cells + (int64_t)b * a.cells_stride);
    if (a.cell > 0) for (int c = tid; c < kGfttCellCap * a.ncells; c += 1024) cells[c] = kCellEmpty;
    __syncthreads();
    // bitonic sort, descending.  Padding keys are 0; every real key is nonzero (f2key of a non-NaN float is nonzero), so the
    // padding sorts behind the n real keys
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < P; i += 1024) {
                const int l = i ^ j;
                if (l > i) {
                    const unsigned long long u = K[i], v = K[l];
                    const bool desc = (i & k) == 0;
                    if (desc ? u < v : u > v) { K[i] = v; K[l] = u; }
                }
            }
            __syncthreads();
        }
    }
    if (tid >= 64) return;                       // (no barrier below)
    // greedy pass, one wave
    float2 *xy = a.kp_xy + (int64_t)b * a.kp_stride;
    float *resp = a.kp_resp + (int64_t)b * a.kp_stride;
    float *strength = a.strength ? a.strength + (int64_t)b * a.kp_stride : nullptr;
    const int maxc = a.max_corners;
    const unsigned long long below = (1ull << lane) - 1ull;
    auto cell_load = [&](int i) -> unsigned {
        return kLdsCells ? ((volatile unsigned *)cells)[i] : __hip_atomic_load(&cells[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    };
    auto cell_store = [&](int i, unsigned v) {
        if (kLdsCells) ((volatile unsigned *)cells)[i] = v;
        else __hip_atomic_store(&cells[i], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    };
    auto put = [&](int at, int x, int y, unsigned long long key) {
        xy[at] = make_float2((float)x, (float)y);
        resp[at] = kGfttRespTag;                 // marks the corner as Shi-Tomasi's (read back as size 3, response 0)
        if (strength) strength[at] = key2f((unsigned)(key >> 32));
    };
    int kept = 0;
    for (int base = 0; base < n && (maxc <= 0 || kept < maxc); base += 64) {
        const int i = base + lane;
        bool alive = i < n;
        const unsigned long long key = alive ? K[i] : 0ull;
        const unsigned idx = (unsigned)key;
        const int y = (int)(idx / (unsigned)a.w), x = (int)(idx - (unsigned)y * (unsigned)a.w);
        if (a.cell <= 0) {                       // minDistance < 1: no spacing, the first maxCorners of the order
            const unsigned long long m = __ballot(alive);
            const int at = kept + __popcll(m & below);
            if (alive && (maxc <= 0 || at < maxc)) put(at, x, y, key);
            kept += __popcll(m);
            if (maxc > 0 && kept > maxc) kept = maxc;
            continue;
        }
        if (!kLdsCells) __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");       // the cell words written for the previous 64
        const int cx = x / a.cell, cy = y / a.cell;
        if (alive) {
            const int x1 = max(0, cx - 1), x2 = min(a.gcols - 1, cx + 1), y1 = max(0, cy - 1), y2 = min(a.grows - 1, cy + 1);
            for (int yy = y1; yy <= y2 && alive; yy++)
                for (int xx = x1; xx <= x2 && alive; xx++)
                    for (int q = 0; q < kGfttCellCap; q++) {
                        const unsigned e = cell_load((yy * a.gcols + xx) * kGfttCellCap + q);
                        if (e == kCellEmpty) break;
                        const int ddx = x - (int)(e & 0xFFFFu), ddy = y - (int)(e >> 16);
                        if ((double)(ddx * ddx + ddy * ddy) < a.min_dist2) { alive = false; break; }
                    }
        }
        // the survivors among themselves, in order
        for (;;) {
            const unsigned long long m = __ballot(alive);
            if (m == 0) break;
            const int l = __ffsll((long long)m) - 1;
            const int xl = __shfl(x, l), yl = __shfl(y, l);
            if (lane == l) {
                put(kept, x, y, key);
                const int c0 = (cy * a.gcols + cx) * kGfttCellCap;
                for (int q = 0; q < kGfttCellCap; q++)                 // (a fifth corner cannot occur: kGfttCellCap)
                    if (cell_load(c0 + q) == kCellEmpty) { cell_store(c0 + q, (unsigned)x | ((unsigned)y << 16)); break; }
                alive = false;
            }
            // device-memory grid: the store is complete in L2 before a later kept corner of these 64 searches the same cell's slots
            if (!kLdsCells) __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");
            kept++;
            if (maxc > 0 && kept >= maxc) break;
            if (alive) {
                const int ddx = x - xl, ddy = y - yl;
                if ((double)(ddx * ddx + ddy * ddy) < a.min_dist2) alive = false;
            }
        }
    }
    if (lane == 0) *n_out = kept;
}

int gftt_lds_cells() { return kGfttLdsCells; }
float gftt_resp_tag() { return kGfttRespTag; }

hipError_t launch_gftt_eigen(const GfttArgs &a, int batch, hipStream_t st)
{
    const hipError_t e = hipMemsetAsync(a.maxkey, 0, sizeof(unsigned) * (size_t)batch, st);
    if (e != hipSuccess) return e;
    dim3 g((a.w + kGTileW - 1) / kGTileW, (a.h + kGTileH - 1) / kGTileH, batch);
    hipLaunchKernelGGL(gftt_eigen_kernel, g, dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_gftt_emit(const GfttArgs &a, int batch, hipStream_t st)
{
    const hipError_t e = hipMemsetAsync(a.n_cand, 0, sizeof(int) * (size_t)batch, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(gftt_emit_kernel, dim3((a.h + kEmitRows - 1) / kEmitRows, batch), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_gftt_select(const GfttArgs &a, int batch, hipStream_t st)
{
    if (a.cell <= 0 || a.ncells <= kGfttLdsCells) hipLaunchKernelGGL(gftt_select_kernel<true>, dim3(batch), dim3(1024), 0, st, a);
    else hipLaunchKernelGGL(gftt_select_kernel<false>, dim3(batch), dim3(1024), 0, st, a);
    return hipGetLastError();
}

// svo_gftt_detect: the structure-of-arrays list -> the records cv::GFTTDetector::detect makes
__global__ __launch_bounds__(256) void gftt_pack_kernel(const float2 *xy, const int *n_dev, int cap, svo_keypoint *out, int *n_out)
{
    const int i = blockIdx.x * 256 + threadIdx.x, n = *n_dev;
    if (i == 0 && n_out) *n_out = n;
    if (i < n && n <= cap) {                   // (more candidates than cap: the count says so, there is no list)
        svo_keypoint k;
        k.x = xy[i].x; k.y = xy[i].y; k.size = 3.f; k.angle = -1.f; k.response = 0.f; k.octave = 0; k.class_id = -1;
        out[i] = k;
    }
}
void launch_gftt_pack(const float2 *xy, const int *n_dev, int cap, svo_keypoint *out, int *n_out, hipStream_t st)
{
    hipLaunchKernelGGL(gftt_pack_kernel, dim3(cap / 256 + 1), dim3(256), 0, st, xy, n_dev, cap, out, n_out);
}

}  // namespace svo
