// orb_match.hip -- the guided ORB matcher (svo_set_orb_matcher; include/svo_abi.h states the arithmetic, DESIGN.md
// section 5f the mapping): the second ORB-mode matcher, off by default.
//
//   stage S (per frame, at ingest)   orbm_stereo_kernel : one wave per left keypoint, sixteen per workgroup -- the workgroup
//                                    stages the right keypoints' band rows, x and octave in LDS once (32 KB per 2048), every
//                                    wave tests 64 of them per trip and takes the packed (dist << 16 | j) minimum; then the
//                                    11-position SAD slide against a 21 x 11 strip of the right level in LDS, the parabola; the
//                                    keypoint's 11 x 11 patch goes to the frame's patch store in the same pass
//                                    orbm_median_kernel : one workgroup per frame -- element n/2 of the accepted SADs by
//                                    two 256-bin histogram passes (a SAD is < 2^16), then the 1.5 * 1.4 cut
//   stage T (per pair)               orbm_search_kernel : one wave per last-left keypoint -- best and second-best Hamming
//                                    distance over the current-left keypoints, ratio test, atomicMin of (b << 16 | i) per j
//                                    orbm_subpix_kernel : one wave per surviving keypoint -- 5 x 5 SADs against a 15 x 15
//                                    window of the current level in LDS, parabola per axis
//                                    orbm_emit_kernel   : one workgroup per pair -- ordered emission (as orb_filter_kernel)
//
// No launch depends on a host read-back: counts are read on the device, grids are sized by the extractor's quotas.
//
// Memory (allocated by the first svo_set_orb_matcher(GUIDED) / stage call; a context that never asks pays nothing), with
// cap = max_keypoints rounded up to 4: per frame slot 16 B header + cap * (128 B patch + float uR + int sad) -- 0.27 MB at
// max_keypoints 2048, 1.06 MB at the default 8192; x (max_batch + 1) frame slots: 68 MB / 273 MB at max_batch 256 -- and per
// pair cap * 20 B of scratch (match, key, winner, sub-pixel point): 10 MB / 40 MB at max_batch 256.  A stream set adds one
// frame block per stream.
#include <cmath>
#include <cstring>
#include "abi_io.h"

namespace svo {

constexpr int kOrbmWaves = 4;                          // waves (= keypoints) per workgroup of stage T's wave-per-keypoint kernels
constexpr int kOrbmSWaves = 16;                        // ... of stage S: sixteen left keypoints share one staging of the right keypoints
constexpr int kOrbmChunk = 2048;                       // right keypoints staged at a time (32 KB of LDS)

__device__ __forceinline__ int orbm_rnd(float x) { return (int)floorf(x + 0.5f); }

struct OrbmLevel { const uint8_t *p; int pitch, w, h; };
// unblurred level l of image slot b (counted from the slot `slots` points at); level 0 read in place is image zb of z
__device__ __forceinline__ OrbmLevel orbm_level(const OrbGeom &g, const OrbL0 &z, const uint8_t *slots, int64_t slot_stride, int b, int zb, int l)
{
    OrbmLevel v;
    v.w = g.w[l]; v.h = g.h[l];
    if (l == 0 && z.img) { v.p = orb_level0(z, zb); v.pitch = z.pitch; }
    else { v.p = slots + (int64_t)b * slot_stride + g.origin[l]; v.pitch = g.pitch[l]; }
    return v;
}

__device__ __forceinline__ int orbm_wave_sum(int v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}
__device__ __forceinline__ unsigned orbm_wave_min(unsigned v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = min(v, (unsigned)__shfl_xor((int)v, m, 64));
    return v;
}

__device__ __forceinline__ int orbm_hamming(const uint4 &a0, const uint4 &a1, const uint8_t *d)
{
    const uint4 b0 = ((const uint4 *)d)[0], b1 = ((const uint4 *)d)[1];
    return __popc(a0.x ^ b0.x) + __popc(a0.y ^ b0.y) + __popc(a0.z ^ b0.z) + __popc(a0.w ^ b0.w) +
           __popc(a1.x ^ b1.x) + __popc(a1.y ^ b1.y) + __popc(a1.z ^ b1.z) + __popc(a1.w ^ b1.w);
}

// delta of the parabola through (-1, d1), (0, d2), (1, d3)
__device__ __forceinline__ float orbm_parabola(int i1, int i2, int i3)
{
    const float d1 = (float)i1, d2 = (float)i2, d3 = (float)i3;
    const float den = 2.0f * ((d1 + d3) - 2.0f * d2);
    return den == 0.0f ? 0.0f : (d1 - d3) / den;
}

// A frame's block: header {epoch, n, 0, 0}, uR[kc], sad[kc], patches[kc][128]
struct OrbmFrame { int *hdr; float *uR; int *sad; uint8_t *patch; };
__host__ __device__ __forceinline__ OrbmFrame orbm_frame(uint8_t *base, int64_t frame_bytes, int kc, int f)
{
    uint8_t *p = base + (int64_t)f * frame_bytes;
    OrbmFrame r;
    r.hdr = (int *)p; r.uR = (float *)(p + 16); r.sad = (int *)(p + 16 + (size_t)kc * 4); r.patch = p + 16 + (size_t)kc * 8;
    return r;
}

// ---- stage S ------------------------------------------------------------------------------------------------------------
struct OrbmStereoArgs {
    OrbGeom g; OrbL0 z;
    const uint8_t *slots; int64_t slot_stride;                 // image slot of the launch's first left image
    const svo_keypoint *kps; const uint8_t *desc; const int *n; int cap;      // the same image's lists
    uint8_t *frames; int64_t frame_bytes; int kc;              // block of the launch's first frame
    float maxd; int th, epoch, wg_per_frame;
};

__global__ __launch_bounds__(64 * kOrbmSWaves) void orbm_stereo_kernel(OrbmStereoArgs a)
{
    __shared__ float4 s_R[kOrbmChunk];                         // right keypoints of the chunk: band low / high row, x, octave
    __shared__ int s_T[kOrbmSWaves][128];
    __shared__ uint8_t s_J[kOrbmSWaves][11 * 21 + 1];
    const int f = blockIdx.x / a.wg_per_frame, blk = blockIdx.x - f * a.wg_per_frame;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int i = blk * kOrbmSWaves + wv;
    const int nL = min(a.n[2 * f], a.cap), nR = min(a.n[2 * f + 1], a.cap);
    const OrbmFrame fr = orbm_frame(a.frames, a.frame_bytes, a.kc, f);
    if (blk == 0 && threadIdx.x == 0) { fr.hdr[0] = a.epoch; fr.hdr[1] = nL; fr.hdr[2] = 0; fr.hdr[3] = 0; }
    if (blk * kOrbmSWaves >= nL) return;                       // (workgroup-uniform: nothing below is reached by a part of a workgroup)
    const bool act = i < nL;                                   // (wave-uniform) a wave without a keypoint only helps staging
    const svo_keypoint *kL = a.kps + (size_t)(2 * f) * a.cap, *kR = a.kps + (size_t)(2 * f + 1) * a.cap;
    const uint8_t *dL = a.desc + ((size_t)(2 * f) * a.cap + (act ? i : 0)) * 32, *dR = a.desc + (size_t)(2 * f + 1) * a.cap * 32;
    const float uL = act ? kL[i].x : 0.f, vL = act ? kL[i].y : 0.f;
    const int oL = act ? kL[i].octave : 0;
    const float inv = 1.0f / a.g.scale[oL];
    const OrbmLevel IL = orbm_level(a.g, a.z, a.slots, a.slot_stride, 2 * f, 2 * f, oL);
    const OrbmLevel IR = orbm_level(a.g, a.z, a.slots, a.slot_stride, 2 * f + 1, 2 * f + 1, oL);
    const int pu = orbm_rnd(uL * inv), pv = orbm_rnd(vL * inv);
    const bool valid = act && pu >= 5 && pu < IL.w - 5 && pv >= 5 && pv < IL.h - 5;
    // the patch: raw bytes to the store (zeros where it leaves the level), differences to its centre in LDS
    if (act) {
        const int c = valid ? IL.p[(int64_t)pv * IL.pitch + pu] : 0;
#pragma unroll
        for (int q = 0; q < 2; q++) {
            const int p = lane + 64 * q;
            int v = 0;
            if (valid && p < 121) v = IL.p[(int64_t)(pv + p / 11 - 5) * IL.pitch + pu + p % 11 - 5];
            fr.patch[(size_t)i * 128 + p] = (uint8_t)v;
            s_T[wv][p] = v - c;
        }
    }
    // candidates of the row band: the workgroup stages the right keypoints once for its sixteen left keypoints, a wave tests 64 per trip
    const uint4 q0 = ((const uint4 *)dL)[0], q1 = ((const uint4 *)dL)[1];
    const float tv = truncf(vL), xlo = uL - a.maxd;
    unsigned best = 0xFFFFFFFFu;
    for (int c0 = 0; c0 < nR; c0 += kOrbmChunk) {              // (nR is the frame's: the barriers are workgroup-uniform)
        const int cn = min(kOrbmChunk, nR - c0);
        __syncthreads();
        for (int t = threadIdx.x; t < cn; t += 64 * kOrbmSWaves) {
            const float yj = kR[c0 + t].y;
            const int oj = kR[c0 + t].octave;
            const float rj = 2.0f * a.g.scale[oj];
            s_R[t] = make_float4(floorf(yj - rj), ceilf(yj + rj), kR[c0 + t].x, __int_as_float(oj));
        }
        __syncthreads();
        if (act)
            for (int t = lane; t < cn; t += 64) {
                const float4 e = s_R[t];
                if (e.x <= tv && tv <= e.y && abs(__float_as_int(e.w) - oL) <= 1 && xlo <= e.z && e.z <= uL) {
                    const unsigned j = (unsigned)(c0 + t);
                    best = min(best, ((unsigned)orbm_hamming(q0, q1, dR + (size_t)j * 32) << 16) | j);
                }
            }
    }
    best = orbm_wave_min(best);
    float uR = -1.0f;
    int sad = -1;
    bool go = act && best != 0xFFFFFFFFu && (int)(best >> 16) < a.th && valid;
    int sr = 0;
    if (go) {
        sr = orbm_rnd(kR[best & 0xFFFFu].x * inv);
        go = sr - 10 >= 0 && sr + 11 < IR.w;
    }
    if (go) {                                                  // (wave-uniform)
        // rows pv-5 .. pv+5, columns sr-10 .. sr+10 of the right level
        for (int p = lane; p < 11 * 21; p += 64)
            s_J[wv][p] = IR.p[(int64_t)(pv - 5 + p / 21) * IR.pitch + sr - 10 + p % 21];
        wave_lds_fence();
        int d[11];
#pragma unroll
        for (int k = 0; k < 11; k++) d[k] = 0;
#pragma unroll
        for (int q = 0; q < 2; q++) {
            const int p = lane + 64 * q;
            if (p < 121) {
                const int dy = p / 11, dx = p % 11, t = s_T[wv][p];
#pragma unroll
                for (int k = 0; k < 11; k++)
                    d[k] += abs(t - ((int)s_J[wv][dy * 21 + dx + k] - (int)s_J[wv][5 * 21 + 5 + k]));
            }
        }
        int kb = 0, dmin = 0x7FFFFFFF;
#pragma unroll
        for (int k = 0; k < 11; k++) {
            d[k] = orbm_wave_sum(d[k]);
            if (d[k] < dmin) { dmin = d[k]; kb = k; }          // first minimum
        }
        if (kb != 0 && kb != 10) {
            int dm = 0, dp = 0;
#pragma unroll
            for (int k = 1; k < 10; k++) if (k == kb) { dm = d[k - 1]; dp = d[k + 1]; }
            const float delta = orbm_parabola(dm, dmin, dp);
            float u = a.g.scale[oL] * (((float)sr + (float)(kb - 5)) + delta);
            const float disp = uL - u;
            if (disp >= 0.0f && disp < a.maxd) {
                if (disp <= 0.0f) u = uL - 0.01f;
                uR = u; sad = dmin;
            }
        }
    }
    if (act && lane == 0) { fr.uR[i] = uR; fr.sad[i] = sad; }
}

struct OrbmMedianArgs { uint8_t *frames; int64_t frame_bytes; int kc; };
__global__ __launch_bounds__(256) void orbm_median_kernel(OrbmMedianArgs a)
{
    __shared__ int s_hist[256];
    __shared__ int s_sel, s_rank, s_n;
    const int tid = threadIdx.x;
    const OrbmFrame fr = orbm_frame(a.frames, a.frame_bytes, a.kc, blockIdx.x);
    const int n = fr.hdr[1];
    // element n_acc / 2 of the accepted SADs in ascending order: the high byte's histogram, then the low byte's
    s_hist[tid] = 0;
    if (tid == 0) s_n = 0;
    __syncthreads();
    int mine = 0;
    for (int i = tid; i < n; i += 256)
        if (fr.uR[i] >= 0.0f) { atomicAdd(&s_hist[(fr.sad[i] >> 8) & 255], 1); mine++; }
    if (mine) atomicAdd(&s_n, mine);
    __syncthreads();
    const int n_acc = s_n;
    if (n_acc == 0) return;
    if (tid == 0) {
        int rank = n_acc / 2, b = 0;
        while (rank >= s_hist[b]) { rank -= s_hist[b]; b++; }
        s_sel = b; s_rank = rank;
    }
    __syncthreads();
    const int hi = s_sel;
    __syncthreads();
    s_hist[tid] = 0;
    __syncthreads();
    for (int i = tid; i < n; i += 256)
        if (fr.uR[i] >= 0.0f && ((fr.sad[i] >> 8) & 255) == hi) atomicAdd(&s_hist[fr.sad[i] & 255], 1);
    __syncthreads();
    if (tid == 0) {
        int rank = s_rank, b = 0;
        while (rank >= s_hist[b]) { rank -= s_hist[b]; b++; }
        s_sel = (hi << 8) | b;
    }
    __syncthreads();
    const float thr = (1.5f * 1.4f) * (float)s_sel;
    for (int i = tid; i < n; i += 256)
        if (fr.uR[i] >= 0.0f && (float)fr.sad[i] >= thr) { fr.uR[i] = -1.0f; fr.sad[i] = -1; }
}

// ---- stage T ------------------------------------------------------------------------------------------------------------
struct OrbmTrackArgs {
    OrbGeom g; OrbL0 z; int z_slot0;                           // z names image slot b as orb_level0(z, b - z_slot0)
    const uint8_t *slots; int64_t slot_stride;                 // image slot 0
    const svo_keypoint *kps; const uint8_t *desc; const int *n; int cap;
    uint8_t *frames; int64_t frame_bytes; int kc;              // frame slot 0
    int fp0, fc0, fstep;
    int th, epoch; float ratio, radius;
    int *mj; unsigned *mkey, *win; float2 *t2; int64_t m_stride;      // per pair
    float2 *t1l, *t1r, *t2l; int64_t out_stride; int *m_out;
    int *idx_prev, *idx_cur;                                   // stage call only (null: not wanted)
    int wg_per_pair;
};

__global__ __launch_bounds__(64 * kOrbmWaves) void orbm_search_kernel(OrbmTrackArgs a)
{
    const int pr = blockIdx.x / a.wg_per_pair, blk = blockIdx.x - pr * a.wg_per_pair;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int i = blk * kOrbmWaves + wv;
    const int fp = a.fp0 + pr * a.fstep, fc = a.fc0 + pr * a.fstep;
    const int nP = min(a.n[2 * fp], a.cap), nC = min(a.n[2 * fc], a.cap);
    if (i >= nP) return;
    const OrbmFrame fr = orbm_frame(a.frames, a.frame_bytes, a.kc, fp);
    int *mj = a.mj + (int64_t)pr * a.m_stride;
    // a frame stored before the matcher was selected has no stereo data: nothing to track from it
    const bool has = fr.hdr[0] == a.epoch && i < fr.hdr[1] && fr.uR[i] >= 0.0f;
    if (!has) { if (lane == 0) mj[i] = -1; return; }
    const svo_keypoint *kP = a.kps + (size_t)(2 * fp) * a.cap, *kC = a.kps + (size_t)(2 * fc) * a.cap;
    const uint8_t *dP = a.desc + ((size_t)(2 * fp) * a.cap + i) * 32, *dC = a.desc + (size_t)(2 * fc) * a.cap * 32;
    const float xi = kP[i].x, yi = kP[i].y;
    const int oi = kP[i].octave;
    const uint4 q0 = ((const uint4 *)dP)[0], q1 = ((const uint4 *)dP)[1];
    unsigned best = 0xFFFFFFFFu;
    int second = 0x7FFFFFFF, ncand = 0;
    for (int j0 = 0; j0 < nC; j0 += 64) {
        const int j = j0 + lane;
        bool c = false;
        if (j < nC) {
            c = abs(kC[j].octave - oi) <= 1;
            if (a.radius > 0.0f) c = c && fabsf(kC[j].x - xi) <= a.radius && fabsf(kC[j].y - yi) <= a.radius;
            if (c) {
                const int dist = orbm_hamming(q0, q1, dC + (size_t)j * 32);
                const unsigned key = ((unsigned)dist << 16) | (unsigned)j;
                if (key < best) { if (best != 0xFFFFFFFFu) second = (int)(best >> 16); best = key; }
                else if (dist < second) second = dist;
            }
        }
        ncand += __popcll(__ballot(c));
    }
    const unsigned gbest = orbm_wave_min(best);
    // the second smallest distance: every lane's best except the winner's, and every lane's runner-up
    unsigned s = (unsigned)second;
    if (best != gbest && best != 0xFFFFFFFFu) s = min(s, best >> 16);
    s = orbm_wave_min(s);
    const int b = (int)(gbest >> 16), j = (int)(gbest & 0xFFFFu);
    const bool keep = ncand > 0 && b <= a.th && (ncand == 1 || (float)b < a.ratio * (float)(int)s);
    if (lane == 0) {
        const unsigned key = ((unsigned)b << 16) | (unsigned)i;
        mj[i] = keep ? j : -1;
        a.mkey[(int64_t)pr * a.m_stride + i] = key;
        if (keep) atomicMin(&a.win[(int64_t)pr * a.m_stride + j], key);       // smallest b, then lowest i
    }
}

__global__ __launch_bounds__(64 * kOrbmWaves) void orbm_subpix_kernel(OrbmTrackArgs a)
{
    __shared__ uint8_t s_J[kOrbmWaves][15 * 15 + 3];
    const int pr = blockIdx.x / a.wg_per_pair, blk = blockIdx.x - pr * a.wg_per_pair;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int i = blk * kOrbmWaves + wv;
    const int fp = a.fp0 + pr * a.fstep, fc = a.fc0 + pr * a.fstep;
    const int nP = min(a.n[2 * fp], a.cap);
    if (i >= nP) return;
    int *mj = a.mj + (int64_t)pr * a.m_stride;
    const int j = mj[i];
    if (j < 0) return;                                         // (wave-uniform)
    bool ok = a.win[(int64_t)pr * a.m_stride + j] == a.mkey[(int64_t)pr * a.m_stride + i];
    const svo_keypoint *kP = a.kps + (size_t)(2 * fp) * a.cap, *kC = a.kps + (size_t)(2 * fc) * a.cap;
    const int o = kP[i].octave;
    const float inv = 1.0f / a.g.scale[o];
    // (level 0 read in place: the extraction that ingested frame fc counted its images from z_slot0)
    const OrbmLevel J = orbm_level(a.g, a.z, a.slots, a.slot_stride, 2 * fc, 2 * fc - a.z_slot0, o);
    const int cu = orbm_rnd(kC[j].x * inv), cv = orbm_rnd(kC[j].y * inv);
    ok = ok && cu >= 7 && cu < J.w - 7 && cv >= 7 && cv < J.h - 7;
    float2 t2 = make_float2(0.f, 0.f);
    if (ok) {
        const OrbmFrame fr = orbm_frame(a.frames, a.frame_bytes, a.kc, fp);
        const uint8_t *pt = fr.patch + (size_t)i * 128;
        for (int p = lane; p < 225; p += 64) s_J[wv][p] = J.p[(int64_t)(cv - 7 + p / 15) * J.pitch + cu - 7 + p % 15];
        wave_lds_fence();
        const int c = pt[60];
        int D[25];
#pragma unroll
        for (int k = 0; k < 25; k++) D[k] = 0;
#pragma unroll
        for (int q = 0; q < 2; q++) {
            const int p = lane + 64 * q;
            if (p < 121) {
                const int dy = p / 11, dx = p % 11, t = (int)pt[p] - c;
#pragma unroll
                for (int k = 0; k < 25; k++) {
                    const int oy = k / 5, ox = k % 5;               // window centre (cv + oy - 2, cu + ox - 2)
                    D[k] += abs(t - ((int)s_J[wv][(dy + oy) * 15 + dx + ox] - (int)s_J[wv][(5 + oy) * 15 + 5 + ox]));
                }
            }
        }
        int kb = 0, dmin = 0x7FFFFFFF;
#pragma unroll
        for (int k = 0; k < 25; k++) {
            D[k] = orbm_wave_sum(D[k]);
            if (D[k] < dmin) { dmin = D[k]; kb = k; }          // first minimum in raster order
        }
        const int by = kb / 5, bx = kb % 5;
        ok = by >= 1 && by <= 3 && bx >= 1 && bx <= 3;
        if (ok) {
            int xm = 0, xp = 0, ym = 0, yp = 0;
#pragma unroll
            for (int k = 6; k < 19; k++) if (k == kb) { xm = D[k - 1]; xp = D[k + 1]; ym = D[k - 5]; yp = D[k + 5]; }
            const float ddx = orbm_parabola(xm, dmin, xp), ddy = orbm_parabola(ym, dmin, yp);
            const float sc = a.g.scale[o];
            t2 = make_float2(sc * (((float)cu + (float)(bx - 2)) + ddx), sc * (((float)cv + (float)(by - 2)) + ddy));
        }
    }
    if (lane == 0) {
        if (ok) a.t2[(int64_t)pr * a.m_stride + i] = t2;
        else mj[i] = -1;
    }
}

__global__ __launch_bounds__(256) void orbm_emit_kernel(OrbmTrackArgs a)
{
    __shared__ int s_base, s_wave[4];
    const int pr = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int fp = a.fp0 + pr * a.fstep;
    const int nP = min(a.n[2 * fp], a.cap);
    const OrbmFrame fr = orbm_frame(a.frames, a.frame_bytes, a.kc, fp);
    const svo_keypoint *kP = a.kps + (size_t)(2 * fp) * a.cap;
    const int *mj = a.mj + (int64_t)pr * a.m_stride;
    const float2 *t2 = a.t2 + (int64_t)pr * a.m_stride;
    const int64_t o = (int64_t)pr * a.out_stride;
    if (tid == 0) s_base = 0;
    __syncthreads();
    for (int start = 0; start < nP; start += 256) {
        const int i = start + tid;
        const bool k = i < nP && mj[i] >= 0;
        const unsigned long long m = __ballot(k);
        const int rank = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) s_wave[wv] = __popcll(m);
        __syncthreads();
        int pre = 0, tot = 0;
        for (int q = 0; q < 4; q++) { if (q < wv) pre += s_wave[q]; tot += s_wave[q]; }
        if (k) {
            const int dst = s_base + pre + rank;
            a.t1l[o + dst] = make_float2(kP[i].x, kP[i].y);
            a.t1r[o + dst] = make_float2(fr.uR[i], kP[i].y);
            a.t2l[o + dst] = t2[i];
            if (a.idx_prev) { a.idx_prev[o + dst] = i; a.idx_cur[o + dst] = mj[i]; }
        }
        __syncthreads();
        if (tid == 0) s_base += tot;
        __syncthreads();
    }
    if (tid == 0) a.m_out[pr] = s_base;
}

// ---- host side ------------------------------------------------------------------------------------------------------------
int orbm_alloc(svo_ctx *ctx)
{
    int rc = orb_alloc(ctx);
    if (rc) return rc;
    if (!ctx->orbm_frames) {
        const int kc = (ctx->orb_kp_cap + 3) & ~3;
        const size_t fb = 16 + (size_t)kc * 136, B = (size_t)ctx->cfg.max_batch, ms = (size_t)kc;
        uint8_t *frames = nullptr, *scratch = nullptr;
        if (dev_alloc(ctx, &frames, fb * (size_t)ctx->n_img) != SVO_OK) return SVO_ERR_HIP;
        if (dev_alloc(ctx, &scratch, B * ms * 20) != SVO_OK) return SVO_ERR_HIP;
        SVO_HIP(hipMemsetAsync(frames, 0, fb * (size_t)ctx->n_img, ctx->stream));      // epoch 0: no frame has stereo data
        ctx->orbm_kc = kc; ctx->orbm_frame_bytes = fb;
        ctx->orbm_t2 = (float2 *)scratch;
        ctx->orbm_mj = (int *)(scratch + B * ms * 8);
        ctx->orbm_mkey = (unsigned *)(scratch + B * ms * 12);
        ctx->orbm_win = (unsigned *)(scratch + B * ms * 16);
        ctx->orbm_frames = frames;
    }
    // a stream set made before the matcher was selected gets its store of frame blocks now
    StreamSet &ss = ctx->streams;
    if (ss.n > 0 && !ss.seg[4]) {
        const size_t bytes = ctx->orbm_frame_bytes * (size_t)ss.n + 16;
        if (dev_alloc(ctx, &ss.seg[4], bytes) != SVO_OK) return SVO_ERR_HIP;
        SVO_HIP(hipMemsetAsync(ss.seg[4], 0, bytes, ctx->stream));
        ss.seg_bytes[4] = ctx->orbm_frame_bytes;
    }
    return SVO_OK;
}

static float orbm_maxd(const svo_ctx *ctx) { return ctx->orbm_max_disparity > 0.0 ? (float)ctx->orbm_max_disparity : (float)ctx->cfg.P1[0]; }

// Stage S on n_frames frames whose images were just extracted into image slots slot0 .. (frame f: 2f left, 2f + 1 right)
int orbm_stereo_frames(svo_ctx *ctx, int slot0, int n_frames, hipStream_t st)
{
    OrbmStereoArgs a{};
    a.g = ctx->orb_geom; a.z = ctx->orb_l0;
    a.slots = ctx->orb_slots + (size_t)slot0 * a.g.slot_bytes; a.slot_stride = a.g.slot_bytes;
    a.kps = (const svo_keypoint *)ctx->orb_kps + (size_t)slot0 * ctx->orb_kp_cap;
    a.desc = ctx->orb_desc + (size_t)slot0 * ctx->orb_kp_cap * 32;
    a.n = ctx->orb_n + slot0; a.cap = ctx->orb_kp_cap;
    a.frame_bytes = (int64_t)ctx->orbm_frame_bytes; a.kc = ctx->orbm_kc;
    a.frames = ctx->orbm_frames + (size_t)(slot0 / 2) * ctx->orbm_frame_bytes;
    a.maxd = orbm_maxd(ctx); a.th = ctx->orbm_th_stereo; a.epoch = ctx->orbm_epoch;
    a.wg_per_frame = (orb_max_keypoints(ctx) + kOrbmSWaves - 1) / kOrbmSWaves;
    hipLaunchKernelGGL(orbm_stereo_kernel, dim3(a.wg_per_frame * n_frames), dim3(64 * kOrbmSWaves), 0, st, a);
    const OrbmMedianArgs m{a.frames, a.frame_bytes, a.kc};
    hipLaunchKernelGGL(orbm_median_kernel, dim3(n_frames), dim3(256), 0, st, m);
    timing_mark(ctx, "orb_stereo");
    return SVO_OK;
}

// Stage T for n_pairs pairs: pair p = (frame fp0 + p*fstep, frame fc0 + p*fstep); writes cmp[0] = t1_left, cmp[1] = t1_right,
// cmp[3] = t2_left, m_out -- what orb_match_pairs writes
int orbm_track_pairs(svo_ctx *ctx, int n_pairs, int fp0, int fc0, int fstep, hipStream_t st, int *idx_prev, int *idx_cur)
{
    OrbmTrackArgs a{};
    a.g = ctx->orb_geom; a.z = ctx->orb_l0; a.z_slot0 = ctx->orb_l0_slot0;
    a.slots = ctx->orb_slots; a.slot_stride = a.g.slot_bytes;
    a.kps = (const svo_keypoint *)ctx->orb_kps; a.desc = ctx->orb_desc; a.n = ctx->orb_n; a.cap = ctx->orb_kp_cap;
    a.frames = ctx->orbm_frames; a.frame_bytes = (int64_t)ctx->orbm_frame_bytes; a.kc = ctx->orbm_kc;
    a.fp0 = fp0; a.fc0 = fc0; a.fstep = fstep;
    a.th = ctx->orbm_th_track; a.epoch = ctx->orbm_epoch; a.ratio = (float)ctx->orbm_ratio; a.radius = (float)ctx->orbm_radius;
    a.mj = ctx->orbm_mj; a.mkey = ctx->orbm_mkey; a.win = ctx->orbm_win; a.t2 = ctx->orbm_t2; a.m_stride = ctx->orbm_kc;
    a.t1l = ctx->cmp[0]; a.t1r = ctx->cmp[1]; a.t2l = ctx->cmp[3]; a.out_stride = ctx->cfg.max_keypoints; a.m_out = ctx->m_out;
    a.idx_prev = idx_prev; a.idx_cur = idx_cur;
    a.wg_per_pair = (orb_max_keypoints(ctx) + kOrbmWaves - 1) / kOrbmWaves;
    SVO_HIP(hipMemsetAsync(a.win, 0xFF, sizeof(unsigned) * (size_t)a.m_stride * n_pairs, st));
    hipLaunchKernelGGL(orbm_search_kernel, dim3(a.wg_per_pair * n_pairs), dim3(64 * kOrbmWaves), 0, st, a);
    hipLaunchKernelGGL(orbm_subpix_kernel, dim3(a.wg_per_pair * n_pairs), dim3(64 * kOrbmWaves), 0, st, a);
    hipLaunchKernelGGL(orbm_emit_kernel, dim3(n_pairs), dim3(256), 0, st, a);
    return SVO_OK;
}

}  // namespace svo

using namespace svo;

extern "C" int svo_set_orb_matcher(svo_ctx *ctx, int mode, int th_stereo, int th_track, double ratio, double radius, double max_disparity)
{
    if (!ctx) return SVO_ERR_ARG;
    SVO_ARG(ctx->cfg.track_mode == SVO_MODE_ORB, "the matcher switch is an ORB-mode option");
    SVO_ARG(mode == SVO_ORB_MATCHER_BRUTE || mode == SVO_ORB_MATCHER_GUIDED, "mode must be SVO_ORB_MATCHER_BRUTE or SVO_ORB_MATCHER_GUIDED");
    SVO_ARG(th_stereo >= 1 && th_stereo <= 256 && th_track >= 1 && th_track <= 256, "thresholds outside 1..256");
    SVO_ARG(std::isfinite(ratio) && ratio > 0.0 && ratio <= 1.0, "ratio outside (0, 1]");
    SVO_ARG(std::isfinite(radius) && radius >= 0.0, "radius must be finite and >= 0");
    SVO_ARG(std::isfinite(max_disparity) && max_disparity >= 0.0, "max_disparity must be finite and >= 0");
    if (mode == SVO_ORB_MATCHER_GUIDED) {
        SVO_HIP(hipSetDevice(ctx->device));
        const int rc = orbm_alloc(ctx);
        if (rc) return rc;                                   // (the setting is what it was)
        // frames stored so far carry no stereo data of this selection: a new epoch disowns them
        if (ctx->orbm_mode != SVO_ORB_MATCHER_GUIDED) ctx->orbm_epoch++;
    }
    ctx->orbm_mode = mode; ctx->orbm_th_stereo = th_stereo; ctx->orbm_th_track = th_track;
    ctx->orbm_ratio = ratio; ctx->orbm_radius = radius; ctx->orbm_max_disparity = max_disparity;
    return SVO_OK;
}

extern "C" int svo_get_orb_matcher(const svo_ctx *ctx, int *mode, int *th_stereo, int *th_track, double *ratio, double *radius, double *max_disparity)
{
    if (!ctx) return SVO_ERR_ARG;
    if (mode) *mode = ctx->orbm_mode;
    if (th_stereo) *th_stereo = ctx->orbm_th_stereo;
    if (th_track) *th_track = ctx->orbm_th_track;
    if (ratio) *ratio = ctx->orbm_ratio;
    if (radius) *radius = ctx->orbm_radius;
    if (max_disparity) *max_disparity = ctx->orbm_max_disparity;
    return SVO_OK;
}

// uR / sad of frame slot `frame`'s block and (kps != null) its left keypoints, to host memory
static int orbm_read_frame(svo_ctx *ctx, int frame, svo_keypoint *kps, float *uR, int *sad, int cap, int *n_out)
{
    enum { kEpoch = 0, kN = 1, kOverflow = 4 };              // positions in the pinned ints: the block's header (4 ints), the two eyes' flags
    const int *h;
    const OrbmFrame fr = orbm_frame(ctx->orbm_frames, (int64_t)ctx->orbm_frame_bytes, ctx->orbm_kc, frame);
    SVO_TRY(count_fetch(ctx, kEpoch, fr.hdr, 4));
    SVO_TRY(count_fetch(ctx, kOverflow, ctx->orb_overflow + 2 * frame, 2));
    SVO_TRY(counts_wait(ctx, &h));
    SVO_ARG(h[kEpoch] == ctx->orbm_epoch, "the frame was stored before the guided matcher was selected: it has no stereo data");
    SVO_ARG(!h[kOverflow] && !h[kOverflow + 1], "ORB: keypoints / candidates exceed the context's capacity");
    const int n = h[kN];
    *n_out = n;
    SVO_ARG(n <= cap, "capacity too small");
    if (n == 0) return SVO_OK;
    SVO_TRY(from_device(ctx, kps, (const svo_keypoint *)ctx->orb_kps + (size_t)(2 * frame) * ctx->orb_kp_cap, (size_t)n, SVO_MEM_HOST));
    SVO_TRY(from_device(ctx, uR, (const float *)fr.uR, (size_t)n, SVO_MEM_HOST));
    SVO_TRY(from_device(ctx, sad, (const int *)fr.sad, (size_t)n, SVO_MEM_HOST));
    return io_done(ctx, SVO_MEM_HOST);
}

extern "C" int svo_orb_stereo_frame(svo_ctx *ctx, const uint8_t *left, const uint8_t *right, int pitch, int mem, int slot,
                                    svo_keypoint *kps, float *uR, int32_t *sad, int cap, int *n_out)
{
    if (!ctx) return SVO_ERR_ARG;
    SVO_ARG(ctx->cfg.track_mode == SVO_MODE_ORB, "an ORB-mode call");
    SVO_ARG(left && right && n_out && cap >= 0, "null pointer / negative capacity");
    SVO_ARG(slot == 0 || slot == 1, "slot must be 0 or 1");
    SVO_ARG(mem == SVO_MEM_HOST || mem == SVO_MEM_DEVICE, "mem must be SVO_MEM_HOST or SVO_MEM_DEVICE");
    SVO_ARG(pitch >= ctx->cfg.width, "pitch < width");
    SVO_HIP(hipSetDevice(ctx->device));
    if (svo_wait_results(ctx) != SVO_OK) return SVO_ERR_HIP;
    int rc = orbm_alloc(ctx);
    if (rc) return rc;
    if (ctx->orbm_epoch == 0) ctx->orbm_epoch = 1;
    ctx->carry_slot = -1; ctx->online_frames = 0;              // the call writes frame slots 0 / 1: neither the online ring nor a carried frame survives
    const uint8_t *dl = left, *dr = right;
    int dp = pitch;
    if (mem == SVO_MEM_HOST) {
        rc = stage_host_image(ctx, left, pitch, 0, &dl, &dp);
        if (rc) return rc;
        rc = stage_host_image(ctx, right, pitch, 1, &dr, &dp);
        if (rc) return rc;
    }
    rc = orb_extract_batch(ctx, dl, dr, dp, 0, 2 * slot, 2, ctx->stream);      // level 0 copied: the levels stay in the slots for stage T
    if (rc) return rc;
    rc = orbm_stereo_frames(ctx, 2 * slot, 1, ctx->stream);
    if (rc) return rc;
    SVO_HIP(hipGetLastError());
    return orbm_read_frame(ctx, slot, kps, uR, sad, cap, n_out);
}

extern "C" int svo_orb_track_frames(svo_ctx *ctx, int slot_prev, int slot_cur, svo_pt2f *t1_left, svo_pt2f *t1_right, svo_pt2f *t2_left,
                                    int32_t *idx_prev, int32_t *idx_cur, int cap, int *n_out)
{
    if (!ctx) return SVO_ERR_ARG;
    SVO_ARG(ctx->cfg.track_mode == SVO_MODE_ORB, "an ORB-mode call");
    SVO_ARG((slot_prev == 0 || slot_prev == 1) && (slot_cur == 0 || slot_cur == 1) && slot_prev != slot_cur, "slots must be 0 and 1");
    SVO_ARG(n_out && cap >= 0, "null pointer / negative capacity");
    if (!ctx->orbm_frames || ctx->orb_l0.img) { ctx->err = "svo_orb_stereo_frame has not filled the stage slots"; return SVO_ERR_STATE; }
    SVO_HIP(hipSetDevice(ctx->device));
    if (svo_wait_results(ctx) != SVO_OK) return SVO_ERR_HIP;
    const size_t kc = (size_t)ctx->orb_kp_cap;
    int *d_idx = (int *)ctx->pts_in;                           // max_keypoints float2 (the LK stage calls' input list): two int lists fit
    int rc = orbm_track_pairs(ctx, 1, slot_prev, slot_cur, 0, ctx->stream, d_idx, d_idx + kc);
    if (rc) return rc;
    SVO_HIP(hipGetLastError());
    SVO_TRY(count_read(ctx, ctx->m_out, n_out));
    const int m = *n_out;
    SVO_ARG(m <= cap, "capacity too small");
    if (m == 0) return SVO_OK;
    svo_pt2f *dst[3] = {t1_left, t1_right, t2_left};
    const float2 *src[3] = {ctx->cmp[0], ctx->cmp[1], ctx->cmp[3]};
    for (int k = 0; k < 3; k++) SVO_TRY(from_device(ctx, (float2 *)dst[k], src[k], (size_t)m, SVO_MEM_HOST));
    SVO_TRY(from_device(ctx, idx_prev, (const int32_t *)d_idx, (size_t)m, SVO_MEM_HOST));
    SVO_TRY(from_device(ctx, idx_cur, (const int32_t *)d_idx + kc, (size_t)m, SVO_MEM_HOST));
    return io_done(ctx, SVO_MEM_HOST);
}

extern "C" int svo_get_frame_stereo(svo_ctx *ctx, float *uR, int32_t *sad, int cap, int *n_out)
{
    if (!ctx) return SVO_ERR_ARG;
    SVO_ARG(n_out && cap >= 0, "null output");
    SVO_ARG(ctx->online_frames > 0, "no frame has been added");
    SVO_ARG(ctx->orbm_mode == SVO_ORB_MATCHER_GUIDED && ctx->orbm_frames, "the guided matcher is off (svo_set_orb_matcher)");
    SVO_HIP(hipSetDevice(ctx->device));
    if (svo_wait_results(ctx) != SVO_OK) return SVO_ERR_HIP;
    return orbm_read_frame(ctx, ctx->online_cur, nullptr, uR, sad, cap, n_out);
}
