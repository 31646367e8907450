// resize.hip -- cv::resize for 8-bit gray frames (reference src/System.cpp:94-97, app/ros/robust-vslam/src/robust_vslam_ros.cpp:
// 86-89): the downscale in front of tracking, INTER_NEAREST (what the reference wrote) and INTER_LINEAR, bit for bit as
// include/svo_abi.h restates them.  One launch resizes every image of a call (grid.z = frame x eye).  The ORB pyramid
// (orb.hip) builds its INTER_LINEAR tables with resize_linear_tables too, and the levels its row-streaming kernel does not
// produce come from the table-driven kernel here (resize_shape + resize_launch_tab, under an LDS budget of its own).
//
//   - no double arithmetic on the device: the tap tables are built on the host (a source column and two 11-bit weights
//     per destination column, two source rows and two weights per destination row) and uploaded once per geometry;
//   - nearest / bilinear: a workgroup produces a tile of destination rows; the source row segments the tile samples are staged in
//     LDS with 16-byte loads of the aligned granules that hold them (any base address and pitch: the misalignment of a row is
//     added to the LDS offset, not taken out of the loads), the gather and the blend run from LDS, a lane makes 4 consecutive
//     destination bytes per row and stores them as one dword;
//   - INTER_LINEAR at exactly 2x is upstream's integer-area path, the rounded mean of a 2 x 2 block: no tables and no LDS, a lane
//     reads 16 + 16 source bytes and stores 8 destination bytes.
// The kernels are memory-bound: 4 source bytes read and 1 written per destination byte at 2x (nearest touches every other
// source row only).
#include <cmath>
#include <cstring>
#include <vector>
#include "svo_ctx.h"

namespace svo {

constexpr int kResizeMaxSrc = 8192;            // sw, sh <= 8192: a source column fits the 16-bit halves of a table entry
constexpr int kResizeMaxTabs = 64;             // distinct geometries cached per context
constexpr int kResizeLdsBytes = 48 * 1024;     // staged source rows of one workgroup at most

struct ResizeArgs {
    const uint8_t *src[2];
    uint8_t *dst[2];
    int64_t sstride, dstride;
    int spitch, dpitch;
    int dw, dh, eyes;
    const int2 *xt;
    const int4 *yt;
    int bx_shift, rpt, lds_pitch;
    int aligned;                               // tables: destination rows are dword-aligned; box: 16-byte loads, 8-byte stores
};

// SVO_INTERP_NEAREST (LINEAR = false): dst[dy][dx] = src[yt[dy].x][xt[dx].x & 0xFFFF].
// SVO_INTERP_LINEAR: cv::resize's two-pass 11-bit fixed point, as orb_resize_stream_kernel (orb.hip) and oracle/orb.c have it.
// STAGED = false (a reduction too steep for the LDS budget): the same gather straight from global memory.
template <bool LINEAR, bool STAGED>
__global__ __launch_bounds__(256) void resize_tab_kernel(ResizeArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t rz_rows[];        // lds_rows x lds_pitch
    const int tid = threadIdx.x, bx = 1 << a.bx_shift;
    const int tx = tid & (bx - 1), ty = tid >> a.bx_shift;
    const int rows_wg = (256 >> a.bx_shift) * a.rpt;
    const int f = blockIdx.z / a.eyes, eye = blockIdx.z - f * a.eyes;
    const uint8_t *src = a.src[eye] + f * a.sstride;
    uint8_t *dst = a.dst[eye] + f * a.dstride;
    const int dy0 = blockIdx.y * rows_wg, dy1 = min(dy0 + rows_wg, a.dh);
    const int dx_first = blockIdx.x * (bx * 4), dx_last = min(dx_first + bx * 4, a.dw) - 1;
    // source columns [s0, s_last] of the tile (the tables are monotone), source rows: bilinear [y_first, y_first + nsrc),
    // nearest the tile's own rows yt[dy0 + r].x
    const int s0 = a.xt[dx_first].x & 0xFFFF, span = (a.xt[dx_last].x >> 16) - s0 + 1;
    const int y_first = a.yt[dy0].x;
    const int nsrc = LINEAR ? a.yt[dy1 - 1].y - y_first + 1 : dy1 - dy0;
    if (STAGED) {
        const int n16 = a.lds_pitch >> 4;
        for (int i = tid; i < nsrc * n16; i += 256) {
            const int r = i / n16, c = i - r * n16;
            const int sy = LINEAR ? y_first + r : a.yt[dy0 + r].x;
            const uint8_t *p = src + (int64_t)sy * a.spitch + s0;
            const int m = (int)((uintptr_t)p & 15);
            // the aligned granule c of the row's segment, if it holds a byte of it (a granule that does is inside the image's
            // pages wherever it starts)
            if (16 * c < m + span) *(uint4 *)(rz_rows + r * a.lds_pitch + 16 * c) = *(const uint4 *)(p - m + 16 * c);
        }
        __syncthreads();
    }
    const int dx0 = dx_first + tx * 4;
    if (dx0 >= a.dw) return;
    int sx[4], sx1[4], a0[4], a1[4];
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int2 t = a.xt[min(dx0 + q, a.dw - 1)];
        sx[q] = t.x & 0xFFFF; sx1[q] = t.x >> 16; a0[q] = (short)(t.y & 0xFFFF); a1[q] = t.y >> 16;
    }
    // row `sy` of the source as the gather sees it: indexed by the source column
    auto row = [&](int sy, int r) {
        const uint8_t *p = src + (int64_t)sy * a.spitch;
        if constexpr (STAGED) return (const uint8_t *)(rz_rows + (r * a.lds_pitch + (int)((uintptr_t)(p + s0) & 15) - s0));
        else return p;
    };
    for (int k = 0; k < a.rpt; k++) {
        const int dy = dy0 + ty * a.rpt + k;
        if (dy >= dy1) break;
        const int4 t = a.yt[dy];                                            // y0, y1, b0, b1
        uint32_t out = 0;
        if (LINEAR) {
            const uint8_t *R0 = row(t.x, t.x - y_first), *R1 = row(t.y, t.y - y_first);
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int r0 = R0[sx[q]] * a0[q] + R0[sx1[q]] * a1[q];
                const int r1 = R1[sx[q]] * a0[q] + R1[sx1[q]] * a1[q];
                out |= (uint32_t)((((t.z * (r0 >> 4)) >> 16) + ((t.w * (r1 >> 4)) >> 16) + 2) >> 2) << (8 * q);
            }
        } else {
            const uint8_t *R0 = row(t.x, dy - dy0);
#pragma unroll
            for (int q = 0; q < 4; q++) out |= (uint32_t)R0[sx[q]] << (8 * q);
        }
        uint8_t *d = dst + (int64_t)dy * a.dpitch + dx0;
        if (a.aligned && dx0 + 4 <= a.dw) *(uint32_t *)d = out;
        else for (int q = 0; q < 4 && dx0 + q < a.dw; q++) d[q] = (uint8_t)(out >> (8 * q));
    }
}

// dst[y][x] = (s[2y][2x] + s[2y][2x+1] + s[2y+1][2x] + s[2y+1][2x+1] + 2) >> 2; 2 dw <= sw and 2 dh <= sh.
// Block (64, 4): a lane owns 8 destination columns of 4 rows.
constexpr int kBoxRows = 4;
__global__ __launch_bounds__(256) void resize_box2_kernel(ResizeArgs a)
{
    const int g = blockIdx.x * 64 + threadIdx.x;
    const int dx0 = g * 8;
    if (dx0 >= a.dw) return;
    const int f = blockIdx.z / a.eyes, eye = blockIdx.z - f * a.eyes;
    const uint8_t *src = a.src[eye] + f * a.sstride;
    uint8_t *dst = a.dst[eye] + f * a.dstride;
    const int dyb = (blockIdx.y * 4 + threadIdx.y) * kBoxRows;
    const bool wide = a.aligned && dx0 + 8 <= a.dw;
    // two bytes of one row summed in each 16-bit half, the rounded mean of two such rows packed into 16 bits
    auto hsum = [](uint32_t w) { return (w & 0x00FF00FFu) + ((w >> 8) & 0x00FF00FFu); };
    auto mean = [&](uint32_t w0, uint32_t w1) {
        const uint32_t v = ((hsum(w0) + hsum(w1) + 0x00020002u) >> 2) & 0x00FF00FFu;
        return (v & 0xFFu) | ((v >> 8) & 0xFF00u);
    };
    if (wide) {
        uint4 r0[kBoxRows], r1[kBoxRows];
#pragma unroll
        for (int k = 0; k < kBoxRows; k++) {
            const int dy = min(dyb + k, a.dh - 1);
            r0[k] = *(const uint4 *)(src + (int64_t)(2 * dy) * a.spitch + 2 * dx0);
            r1[k] = *(const uint4 *)(src + (int64_t)(2 * dy + 1) * a.spitch + 2 * dx0);
        }
#pragma unroll
        for (int k = 0; k < kBoxRows; k++) {
            if (dyb + k >= a.dh) break;
            uint2 o;
            o.x = mean(r0[k].x, r1[k].x) | (mean(r0[k].y, r1[k].y) << 16);
            o.y = mean(r0[k].z, r1[k].z) | (mean(r0[k].w, r1[k].w) << 16);
            *(uint2 *)(dst + (int64_t)(dyb + k) * a.dpitch + dx0) = o;
        }
        return;
    }
    for (int k = 0; k < kBoxRows && dyb + k < a.dh; k++) {
        const uint8_t *s0 = src + (int64_t)(2 * (dyb + k)) * a.spitch, *s1 = s0 + a.spitch;
        uint8_t *d = dst + (int64_t)(dyb + k) * a.dpitch;
        for (int dx = dx0; dx < dx0 + 8 && dx < a.dw; dx++)
            d[dx] = (uint8_t)((s0[2 * dx] + s0[2 * dx + 1] + s1[2 * dx] + s1[2 * dx + 1] + 2) >> 2);
    }
}

// ---- host: the geometry of one resize -----------------------------------------------------------------------------------

// cv::resize's scale: factor form (Size(), fx, fy: inv = f, dsize = cvRound(ssize * f)) or size form (inv = dsize / ssize)
static bool resize_scales(int sw, int sh, int dw, int dh, double fx, double fy, double *inv_x, double *inv_y)
{
    if (fx > 0 && fy > 0) {
        if ((int)nearbyint(sw * fx) != dw || (int)nearbyint(sh * fy) != dh) return false;      // cvRound: ties to even
        *inv_x = fx; *inv_y = fy;
    } else if (fx == 0 && fy == 0) {
        *inv_x = (double)dw / sw; *inv_y = (double)dh / sh;
    } else {
        return false;
    }
    return *inv_x > 0 && *inv_x <= 1 && *inv_y > 0 && *inv_y <= 1;
}

// cv::resize's INTER_LINEAR coordinate / weight tables (11-bit weights, scale = 1 / inv: orc_resize_linear_u8 of oracle/orb.c).
// x: clamped as upstream's xofs / alpha loop does, y: rows clamped to the source like upstream's vertical pass.
void resize_linear_tables(int sw, int sh, int dw, int dh, double inv_x, double inv_y, int2 *xt, int4 *yt)
{
    const double scale_x = 1. / inv_x, scale_y = 1. / inv_y;
    for (int dx = 0; dx < dw; dx++) {
        float fx = (float)((dx + 0.5) * scale_x - 0.5);
        int sx = (int)floorf(fx);
        fx -= sx;
        if (sx < 0) { fx = 0; sx = 0; }
        if (sx >= sw - 1) { fx = 0; sx = sw - 1; }
        const int a0 = (short)lrintf((1.f - fx) * 2048), a1 = (short)lrintf(fx * 2048);
        const int sx1 = sx + 1 < sw ? sx + 1 : sx;
        xt[dx] = make_int2(sx | (sx1 << 16), (a0 & 0xFFFF) | (a1 << 16));
    }
    for (int dy = 0; dy < dh; dy++) {
        float fy = (float)((dy + 0.5) * scale_y - 0.5);
        int sy = (int)floorf(fy);
        fy -= sy;
        const int b0 = (short)lrintf((1.f - fy) * 2048), b1 = (short)lrintf(fy * 2048);
        const int y0 = sy < 0 ? 0 : (sy >= sh ? sh - 1 : sy);
        const int y1 = sy + 1 < 0 ? 0 : (sy + 1 >= sh ? sh - 1 : sy + 1);
        yt[dy] = make_int4(y0, y1, b0, b1);
    }
}

static void resize_tables(const ResizeTab &t, std::vector<int2> &xt, std::vector<int4> &yt)
{
    xt.resize((size_t)t.dw); yt.resize((size_t)t.dh);
    if (t.interp == SVO_INTERP_LINEAR) {
        resize_linear_tables(t.sw, t.sh, t.dw, t.dh, t.inv_x, t.inv_y, xt.data(), yt.data());
        return;
    }
    const double scale_x = 1. / t.inv_x, scale_y = 1. / t.inv_y;
    for (int dx = 0; dx < t.dw; dx++) {
        int sx = (int)floor(dx * scale_x);
        sx = sx < t.sw - 1 ? sx : t.sw - 1;
        xt[(size_t)dx] = make_int2(sx | (sx << 16), 0);
    }
    for (int dy = 0; dy < t.dh; dy++) {
        int sy = (int)floor(dy * scale_y);
        sy = sy < t.sh - 1 ? sy : t.sh - 1;
        yt[(size_t)dy] = make_int4(sy, sy, 0, 0);
    }
}

// The workgroup shape and the LDS it needs, from the tables: exactly the tiles resize_tab_kernel forms.
ResizeShape resize_shape(int interp, int dw, int dh, const int2 *xt, const int4 *yt, size_t lds_budget)
{
    ResizeShape s;
    const int lanes = (dw + 3) / 4;
    s.bx_shift = lanes <= 64 ? 6 : (lanes <= 128 ? 7 : 8);
    const int tile_w = 4 << s.bx_shift;
    int span = 0;
    for (int x0 = 0; x0 < dw; x0 += tile_w) {
        const int x1 = (x0 + tile_w < dw ? x0 + tile_w : dw) - 1;
        const int n = (xt[x1].x >> 16) - (xt[x0].x & 0xFFFF) + 1;
        span = n > span ? n : span;
    }
    s.lds_pitch = ((span + 14) / 16 + 1) * 16;         // the segment's granules at the worst misalignment (15)
    if (s.lds_pitch % 256 == 0) s.lds_pitch += 16;      // rows of the tile on different banks
    // 8 rows per lane, or as many as the LDS budget allows (measured on 128 pairs 1920x1080 -> 960x540 nearest: 158 us at 4,
    // 139 at 8, 168 at 16; the ORB pyramid at 1.2 with the kernel forced on every level: 1.281 ms per 514 images where levels 1
    // and 5 fell from 8 to 4, 1.294 where all but one level did)
    for (s.rpt = 8; s.rpt >= 1; s.rpt--) {
        const int rows_wg = (256 >> s.bx_shift) * s.rpt;
        int nsrc = 0;
        for (int y0 = 0; y0 < dh; y0 += rows_wg) {
            const int y1 = (y0 + rows_wg < dh ? y0 + rows_wg : dh) - 1;
            const int n = interp == SVO_INTERP_LINEAR ? yt[y1].y - yt[y0].x + 1 : y1 - y0 + 1;
            nsrc = n > nsrc ? n : nsrc;
        }
        s.lds_rows = nsrc;
        if ((size_t)nsrc * s.lds_pitch <= lds_budget) return s;
    }
    s.rpt = 1; s.lds_rows = 0;                          // a reduction too steep to stage: gathered from global memory
    return s;
}

int resize_plan(svo_ctx *ctx, int sw, int sh, int dw, int dh, int interp, double fx, double fy, int *tab)
{
    SVO_ARG(interp == SVO_INTERP_NEAREST || interp == SVO_INTERP_LINEAR, "interp must be SVO_INTERP_NEAREST or SVO_INTERP_LINEAR");
    SVO_ARG(sw >= 1 && sh >= 1 && sw <= kResizeMaxSrc && sh <= kResizeMaxSrc, "source size must be in [1, 8192]");
    SVO_ARG(dw >= 1 && dh >= 1, "destination size must be >= 1");
    SVO_ARG(fx >= 0 && fy >= 0 && fx == fx && fy == fy, "fx / fy must be both > 0 (factor form) or both 0 (size form)");
    for (size_t i = 0; i < ctx->resize_tabs.size(); i++) {
        const ResizeTab &c = ctx->resize_tabs[i];
        if (c.sw == sw && c.sh == sh && c.dw == dw && c.dh == dh && c.interp == interp && c.fx == fx && c.fy == fy) { *tab = (int)i; return SVO_OK; }
    }
    ResizeTab t;
    t.sw = sw; t.sh = sh; t.dw = dw; t.dh = dh; t.interp = interp; t.fx = fx; t.fy = fy;
    SVO_ARG(resize_scales(sw, sh, dw, dh, fx, fy, &t.inv_x, &t.inv_y),
            "resize: factor form needs dsize = cvRound(ssize * f), and only 0 < scale <= 1 (downscale or identity) is supported");
    t.box = interp == SVO_INTERP_LINEAR && 1. / t.inv_x == 2.0 && 1. / t.inv_y == 2.0;
    if (t.box) {
        SVO_ARG(2 * dw <= sw && 2 * dh <= sh, "INTER_LINEAR at exactly 2x is the 2x2 mean: needs 2 * dw <= sw and 2 * dh <= sh");
    } else {
        SVO_ARG((int)ctx->resize_tabs.size() < kResizeMaxTabs, "more than 64 distinct resize geometries on one context");
        std::vector<int2> xt;
        std::vector<int4> yt;
        resize_tables(t, xt, yt);
        t.shape = resize_shape(interp, dw, dh, xt.data(), yt.data(), kResizeLdsBytes);
        SVO_HIP(hipSetDevice(ctx->device));
        if (dev_alloc(ctx, &t.xt, sizeof(int2) * xt.size()) != SVO_OK) return SVO_ERR_HIP;
        if (dev_alloc(ctx, &t.yt, sizeof(int4) * yt.size()) != SVO_OK) return SVO_ERR_HIP;
        SVO_HIP(hipMemcpy(t.xt, xt.data(), sizeof(int2) * xt.size(), hipMemcpyHostToDevice));
        SVO_HIP(hipMemcpy(t.yt, yt.data(), sizeof(int4) * yt.size(), hipMemcpyHostToDevice));
    }
    ctx->resize_tabs.push_back(t);
    *tab = (int)ctx->resize_tabs.size() - 1;
    return SVO_OK;
}

// What both kernels are told about a call's images; grid.z = frame x eye, so one launch takes 65535 images at most.
static int resize_args(svo_ctx *ctx, ResizeArgs &a, const uint8_t *src0, const uint8_t *src1, int spitch, int64_t sstride,
                       uint8_t *dst0, uint8_t *dst1, int dpitch, int64_t dstride, int dw, int dh, int n_frames)
{
    a.src[0] = src0; a.src[1] = src1; a.dst[0] = dst0; a.dst[1] = dst1;
    a.eyes = src1 ? 2 : 1;
    a.spitch = spitch; a.dpitch = dpitch;
    a.sstride = n_frames > 1 ? sstride : 0; a.dstride = n_frames > 1 ? dstride : 0;
    a.dw = dw; a.dh = dh;
    SVO_ARG(n_frames >= 1 && n_frames * a.eyes <= 65535, "resize: too many frames for one launch");
    return SVO_OK;
}

static bool resize_aligned(const ResizeArgs &a, int src_al, int dst_al)
{
    const uintptr_t s = (uintptr_t)a.src[0] | (uintptr_t)a.src[1] | (uintptr_t)a.spitch | (uintptr_t)a.sstride;
    const uintptr_t d = (uintptr_t)a.dst[0] | (uintptr_t)a.dst[1] | (uintptr_t)a.dpitch | (uintptr_t)a.dstride;
    return ((s & (uintptr_t)(src_al - 1)) | (d & (uintptr_t)(dst_al - 1))) == 0;
}

int resize_launch_tab(svo_ctx *ctx, const ResizeShape &sh, int interp, const int2 *xt, const int4 *yt, int dw, int dh,
                      const uint8_t *src0, const uint8_t *src1, int spitch, int64_t sstride,
                      uint8_t *dst0, uint8_t *dst1, int dpitch, int64_t dstride, int n_frames, hipStream_t st)
{
    ResizeArgs a{};
    const int rc = resize_args(ctx, a, src0, src1, spitch, sstride, dst0, dst1, dpitch, dstride, dw, dh, n_frames);
    if (rc) return rc;
    a.xt = xt; a.yt = yt;
    a.bx_shift = sh.bx_shift; a.rpt = sh.rpt; a.lds_pitch = sh.lds_pitch;
    a.aligned = resize_aligned(a, 1, 4);
    const int tile_w = 4 << sh.bx_shift, rows_wg = (256 >> sh.bx_shift) * sh.rpt;
    const dim3 grid((unsigned)((dw + tile_w - 1) / tile_w), (unsigned)((dh + rows_wg - 1) / rows_wg), (unsigned)(n_frames * a.eyes));
    const size_t lds = (size_t)sh.lds_rows * sh.lds_pitch;
    const bool lin = interp == SVO_INTERP_LINEAR;
    if (lds > 0) {
        if (lin) hipLaunchKernelGGL((resize_tab_kernel<true, true>), grid, dim3(256), lds, st, a);
        else hipLaunchKernelGGL((resize_tab_kernel<false, true>), grid, dim3(256), lds, st, a);
    } else {
        if (lin) hipLaunchKernelGGL((resize_tab_kernel<true, false>), grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL((resize_tab_kernel<false, false>), grid, dim3(256), 0, st, a);
    }
    SVO_HIP(hipGetLastError());
    return SVO_OK;
}

int resize_launch(svo_ctx *ctx, int tab, const uint8_t *src0, const uint8_t *src1, int spitch, int64_t sstride,
                  uint8_t *dst0, uint8_t *dst1, int dpitch, int64_t dstride, int n_frames, hipStream_t st)
{
    const ResizeTab &t = ctx->resize_tabs[(size_t)tab];
    if (!t.box)
        return resize_launch_tab(ctx, t.shape, t.interp, (const int2 *)t.xt, (const int4 *)t.yt, t.dw, t.dh, src0, src1, spitch, sstride,
                                 dst0, dst1, dpitch, dstride, n_frames, st);
    ResizeArgs a{};
    const int rc = resize_args(ctx, a, src0, src1, spitch, sstride, dst0, dst1, dpitch, dstride, t.dw, t.dh, n_frames);
    if (rc) return rc;
    a.aligned = resize_aligned(a, 16, 8);
    const dim3 grid((unsigned)((t.dw + 8 * 64 - 1) / (8 * 64)), (unsigned)((t.dh + 4 * kBoxRows - 1) / (4 * kBoxRows)), (unsigned)(n_frames * a.eyes));
    hipLaunchKernelGGL(resize_box2_kernel, grid, dim3(64, 4), 0, st, a);
    SVO_HIP(hipGetLastError());
    return SVO_OK;
}

}  // namespace svo

using namespace svo;

// P_out = S * P with S = [[inv_x, 0, ox], [0, inv_y, oy], [0, 0, 1]]: the projection matrix of the resized image.
extern "C" int svo_scale_projection(const double P[12], double inv_x, double inv_y, int interp, double P_out[12])
{
    if (!P || !P_out) return SVO_ERR_ARG;
    if (!(inv_x > 0 && inv_x <= 1 && inv_y > 0 && inv_y <= 1)) return SVO_ERR_ARG;
    if (interp != SVO_INTERP_NEAREST && interp != SVO_INTERP_LINEAR) return SVO_ERR_ARG;
    // nearest: destination pixel dx shows source pixel dx * scale; linear (both branches): pixel centres,
    // x_dst = (x_src + 0.5) * inv - 0.5
    const double ox = interp == SVO_INTERP_LINEAR ? 0.5 * (inv_x - 1) : 0.0, oy = interp == SVO_INTERP_LINEAR ? 0.5 * (inv_y - 1) : 0.0;
    double out[12];
    for (int c = 0; c < 4; c++) {
        out[c] = inv_x * P[c] + ox * P[8 + c];
        out[4 + c] = inv_y * P[4 + c] + oy * P[8 + c];
        out[8 + c] = P[8 + c];
    }
    memcpy(P_out, out, sizeof(out));
    return SVO_OK;
}

extern "C" int svo_resize(svo_ctx *ctx, const uint8_t *src, int sw, int sh, int spitch, int64_t sstride,
                          uint8_t *dst, int dw, int dh, int dpitch, int64_t dstride, int n_frames,
                          int interp, double fx, double fy, int mem)
{
    if (!ctx) return SVO_ERR_ARG;
    SVO_ARG(src && dst, "null image");
    SVO_ARG(mem == SVO_MEM_HOST || mem == SVO_MEM_DEVICE, "mem must be SVO_MEM_HOST or SVO_MEM_DEVICE");
    SVO_ARG(n_frames >= 1 && n_frames <= 32767, "n_frames must be in [1, 32767]");
    SVO_ARG(sw >= 1 && sh >= 1 && dw >= 1 && dh >= 1 && spitch >= sw && dpitch >= dw, "bad size / pitch");
    SVO_ARG(n_frames == 1 || (sstride >= (int64_t)spitch * sh && dstride >= (int64_t)dpitch * dh), "bad frame stride");
    SVO_HIP(hipSetDevice(ctx->device));
    int tab = -1;
    int rc = resize_plan(ctx, sw, sh, dw, dh, interp, fx, fy, &tab);
    if (rc) return rc;
    if (mem == SVO_MEM_DEVICE)
        return resize_launch(ctx, tab, src, nullptr, spitch, sstride, dst, nullptr, dpitch, dstride, n_frames, ctx->stream);
    // host images: tight 16-byte-aligned device copies of both sides; the destination's bytes beyond dw are never written
    const int sp = (sw + 15) & ~15, dp = (dw + 15) & ~15;
    const size_t sbytes = (size_t)sp * sh, dbytes = (size_t)dp * dh;
    if ((rc = dev_reserve(ctx, &ctx->resize_scratch[0], sbytes * (size_t)n_frames)) != SVO_OK) return rc;
    if ((rc = dev_reserve(ctx, &ctx->resize_scratch[1], dbytes * (size_t)n_frames)) != SVO_OK) return rc;
    uint8_t *d_src = ctx->resize_scratch[0].base, *d_dst = ctx->resize_scratch[1].base;
    for (int f = 0; f < n_frames; f++)
        SVO_HIP(hipMemcpy2DAsync(d_src + f * sbytes, (size_t)sp, src + (n_frames > 1 ? f * sstride : 0), (size_t)spitch,
                                 (size_t)sw, (size_t)sh, hipMemcpyHostToDevice, ctx->stream));
    rc = resize_launch(ctx, tab, d_src, nullptr, sp, (int64_t)sbytes, d_dst, nullptr, dp,
                       (int64_t)dbytes, n_frames, ctx->stream);
    if (rc) return rc;
    for (int f = 0; f < n_frames; f++)
        SVO_HIP(hipMemcpy2DAsync(dst + (n_frames > 1 ? f * dstride : 0), (size_t)dpitch, d_dst + f * dbytes, (size_t)dp,
                                 (size_t)dw, (size_t)dh, hipMemcpyDeviceToHost, ctx->stream));
    SVO_HIP(hipStreamSynchronize(ctx->stream));
    return SVO_OK;
}
