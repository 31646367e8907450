// abi_io.h -- how the entry points move a call's inputs, counts and outputs between the caller's memory and the device
// (internal).  Plain functions on the context: inputs go in with to_device, device counts come back through the pinned ints
// (count_fetch ... counts_wait, or count_read for a single one), outputs leave with from_device + io_done, and what is read
// back THROUGH pinned memory gets its place from pinned_block / pinned_records (pinned_layout.h) and nowhere else.
#pragma once
#include "svo_ctx.h"

namespace svo {
// ---- inputs: copies n items into the context's scratch (host) or aliases the caller's (device)
template <typename T>
inline int to_device(svo_ctx *ctx, const T *src, T *scratch, size_t n, int mem, const T **d)
{
    if (mem == SVO_MEM_DEVICE) { *d = src; return SVO_OK; }
    if (n > 0) SVO_HIP(hipMemcpyAsync(scratch, src, sizeof(T) * n, hipMemcpyHostToDevice, ctx->stream));
    *d = scratch;
    return SVO_OK;
}

// ---- outputs: n items from device memory into the caller's (or into pinned memory), enqueued on st (null: the context's
// stream).  SVO_MEM_HOST: a device-to-host copy, complete after io_done; SVO_MEM_DEVICE: a device-to-device copy, or nothing
// where the kernels wrote to dst themselves (dst == src).  A null dst or n == 0 copies nothing.
template <typename T>
inline int from_device(svo_ctx *ctx, T *dst, const T *src, size_t n, int mem, hipStream_t st = nullptr)
{
    if (!dst || n == 0 || dst == src) return SVO_OK;
    SVO_HIP(hipMemcpyAsync(dst, src, sizeof(T) * n, mem == SVO_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, st ? st : ctx->stream));
    return SVO_OK;
}

// host outputs are complete when the stream has drained; device outputs are complete in stream order
inline int io_done(svo_ctx *ctx, int mem, hipStream_t st = nullptr)
{
    if (mem == SVO_MEM_HOST) SVO_HIP(hipStreamSynchronize(st ? st : ctx->stream));
    return SVO_OK;
}

// ---- what a call reads back through pinned memory: `bytes` of the block / of the step records
template <typename T>
inline int pinned_range(svo_ctx *ctx, size_t at, size_t have, size_t bytes, T **p)
{
    if (bytes > have) { ctx->err = "internal: a read-back exceeds the pinned layout (pinned_layout.h)"; return SVO_ERR_STATE; }
    *p = (T *)((char *)ctx->h_pinned + at);
    return SVO_OK;
}
template <typename T> inline int pinned_block(svo_ctx *ctx, size_t bytes, T **p) { return pinned_range(ctx, ctx->pinned.block, ctx->pinned.block_bytes, bytes, p); }
template <typename T> inline int pinned_records(svo_ctx *ctx, size_t bytes, T **p) { return pinned_range(ctx, ctx->pinned.records, ctx->pinned.records_bytes, bytes, p); }

// ---- counts: k ints at device address d into the pinned ints [at, at + k), enqueued; counts_wait synchronises ONCE and hands
// the pinned ints back, whatever number of count_fetch calls went before
inline int count_fetch(svo_ctx *ctx, int at, const void *d, int k = 1, hipStream_t st = nullptr)
{
    int *h;
    SVO_TRY(pinned_range(ctx, ctx->pinned.ints, ctx->pinned.ints_bytes, sizeof(int) * (size_t)(at + k), &h));
    return from_device(ctx, h + at, (const int *)d, (size_t)k, SVO_MEM_HOST, st);
}

inline int counts_wait(svo_ctx *ctx, const int **h, hipStream_t st = nullptr)
{
    *h = (const int *)((char *)ctx->h_pinned + ctx->pinned.ints);
    return io_done(ctx, SVO_MEM_HOST, st);
}

inline int count_read(svo_ctx *ctx, const int *d, int *n)            // the usual case: one count, the context's stream
{
    const int *h;
    SVO_TRY(count_fetch(ctx, 0, d));
    SVO_TRY(counts_wait(ctx, &h));
    *n = h[0];
    return SVO_OK;
}

// ---- keypoint records of (xy, response) lists on the host: the cv::KeyPoint cv::FAST produces -- (pt, 7.f, -1, response, 0,
// -1) -- or the one cv::GFTTDetector makes (size 3, response 0) where the response carries the Shi-Tomasi tag, a value no FAST
// score takes (gftt.hip)
inline void format_keypoints(const float2 *xy, const float *resp, int n, svo_keypoint *out)
{
    const float tag = gftt_resp_tag();
    for (int i = 0; i < n; i++) {
        const bool gftt = resp[i] == tag;
        out[i].x = xy[i].x; out[i].y = xy[i].y; out[i].size = gftt ? 3.f : 7.f; out[i].angle = -1.f;
        out[i].response = gftt ? 0.f : resp[i]; out[i].octave = 0; out[i].class_id = -1;
    }
}
}  // namespace svo
