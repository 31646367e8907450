// window.hip -- the sliding window over carried tracks: window_update_kernel (svo_window_update, below) and window_ba_kernel
// (svo_window_ba, further down).  The landmark table first: the frames of a fixed-lag window and, per track
// id, one world point with its stereo observations in every frame that saw it.  The rules (T2-T7 of include/svo_abi.h,
// DESIGN.md section 5i), for one step with ok = 1 on pair a -> b:
//
//   n = 0      : slot 0 is frame a, pose inverse(pose_a); the table has no rows
//   n = W      : slide -- slot 0 leaves, masks and observation columns move down by one, rows nobody sees any more leave
//   then       : frame b is the newest slot, pose inverse(pose_b)
//   tracks     : usable = four observations and the float32 triangulated point finite.  The newest slot gets (t2_left,
//                t2_right); the slot before it gets (t1_left, t1_right) unless the row has it already; an id without a row
//                gets one, X = Ra^T (X_tri - ta) with slot a's pose
//
// Rows and tracks are both ascending by id, so the update is a merge: a row's place is its rank among the surviving rows plus
// the new tracks below its id (a binary search in the track list), a new track's place is its rank among the new tracks plus
// the surviving rows below its id (a binary search in the row list).  One workgroup of 1024 lanes; the ranks come from block
// scans whose prefixes stay in device scratch.  Nothing is written to `out` before the row count is known to fit.
#include <cstring>
#include "pose_device.h"
#include "refine_device.h"
#include "window.h"

namespace svo {

// first index in [0, n) whose id is >= id (n: none)
__device__ inline int window_lower_bound(const long long *ids, int n, long long id)
{
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (ids[mid] < id) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__device__ inline bool window_finite2(float2 p) { return isfinite(p.x) && isfinite(p.y); }

__device__ inline bool window_usable(const WindowUpdateArgs &a, int k)
{
    const float *X = a.tri + 3 * (int64_t)k;
    return window_finite2(a.t1_left[k]) && window_finite2(a.t1_right[k]) && window_finite2(a.t2_left[k]) && window_finite2(a.t2_right[k]) &&
           isfinite(X[0]) && isfinite(X[1]) && isfinite(X[2]);
}

__global__ __launch_bounds__(1024) void window_update_kernel(WindowUpdateArgs a)
{
    __shared__ int wave_tot[16];
    __shared__ double pose[kWindowMaxFrames * kWindowPose];
    const int tid = threadIdx.x;
    if (blockIdx.x != 0) return;
    const int W = a.frames;
    if (a.ok && *a.ok == 0) {                                                // T1: a failed step clears the window
        if (tid < 4) a.out.counts[tid] = 0;
        return;
    }
    int nt = a.n_trk;
    if (a.n_trk_dev) { const int d = *a.n_trk_dev; nt = d < 0 ? 0 : (d < nt ? d : nt); }
    const double *pose_a = a.pose_a_by_value ? a.pose_a_value : a.pose_a;
    int n = a.clear_in ? 0 : a.in.counts[0], m = a.in.counts[1];
    n = n < 0 ? 0 : (n > W ? W : n);
    m = (n == 0 || m < 0) ? 0 : (m > a.cap ? a.cap : m);
    const int shift = n == W ? 1 : 0;
    const int prev = (n == 0 ? 1 : n - shift) - 1, cur = prev + 1;           // frame a's slot, frame b's slot: cur <= W - 1
    if (tid < kWindowMaxFrames * kWindowPose) {
        const int slot = tid / kWindowPose, e = tid % kWindowPose;
        double v = 0.0;
        if (slot < cur) v = n == 0 ? pose_inv_t4_elem(pose_a, e) : a.in.poses[(slot + shift) * kWindowPose + e];
        else if (slot == cur) v = pose_inv_t4_elem(a.pose_b, e);
        pose[tid] = v;
    }

    // ---- the surviving rows and their ranks
    int n_rows = 0;
    for (int start = 0; start < m; start += 1024) {
        const int r = start + tid;
        const bool s = r < m && (a.in.seen[r] >> shift) != 0;
        int tot;
        const int ex = block1024_excl_scan(s ? 1 : 0, wave_tot, tot);
        if (r < m) a.pre_rows[r] = n_rows + ex;
        n_rows += tot;
    }
    if (tid == 0) a.pre_rows[m] = n_rows;
    // ---- the tracks that make a row and their ranks
    int n_new = 0;
    for (int start = 0; start < nt; start += 1024) {
        const int k = start + tid;
        bool fresh = false;
        if (k < nt && window_usable(a, k)) {
            const long long id = a.ids[k];
            const int r = window_lower_bound(a.in.ids, m, id);
            fresh = !(r < m && a.in.ids[r] == id && (a.in.seen[r] >> shift) != 0);
        }
        int tot;
        const int ex = block1024_excl_scan(fresh ? 1 : 0, wave_tot, tot);
        if (k < nt) a.pre_new[k] = n_new + ex;
        n_new += tot;
    }
    if (tid == 0) a.pre_new[nt] = n_new;
    __syncthreads();                                                         // the prefixes, and pose[]
    const int m_out = n_rows + n_new;
    if (m_out > a.cap) {                                                     // T7: nothing but the counts is written
        if (tid < 4) a.out.counts[tid] = tid == 2 ? m_out : 0;
        return;
    }
    if (tid < kWindowMaxFrames * kWindowPose) a.out.poses[tid] = pose[tid];

    // ---- surviving rows: moved down, joined with their track
    for (int r = tid; r < m; r += 1024) {
        uint32_t seen = a.in.seen[r] >> shift;
        if (seen == 0) continue;
        const long long id = a.in.ids[r];
        const int k = window_lower_bound(a.ids, nt, id);
        const int64_t dst = a.pre_rows[r] + a.pre_new[k];                    // < n_rows + n_new = m_out <= cap
        const bool joined = k < nt && a.ids[k] == id && window_usable(a, k);
        a.out.ids[dst] = id;
        for (int j = 0; j < 3; j++) a.out.X[3 * dst + j] = a.in.X[3 * (int64_t)r + j];
        a.out.active[dst] = a.in.active[r] >> shift;
        for (int j = 0; j < kWindowMaxFrames; j++) {
            const int src = j + shift;
            float2 l = make_float2(0.f, 0.f), q = l;
            if (src < kWindowMaxFrames) { l = a.in.obs_left[(int64_t)r * kWindowMaxFrames + src]; q = a.in.obs_right[(int64_t)r * kWindowMaxFrames + src]; }
            if (joined && j == cur) { l = a.t2_left[k]; q = a.t2_right[k]; }
            if (joined && j == prev && !(seen >> prev & 1u)) { l = a.t1_left[k]; q = a.t1_right[k]; }
            a.out.obs_left[dst * kWindowMaxFrames + j] = l; a.out.obs_right[dst * kWindowMaxFrames + j] = q;
        }
        if (joined) seen |= 1u << prev | 1u << cur;
        a.out.seen[dst] = seen;
    }
    // ---- new rows
    const double *Ra = pose + prev * kWindowPose, *ta = Ra + 9;
    for (int k = tid; k < nt; k += 1024) {
        if (a.pre_new[k + 1] == a.pre_new[k]) continue;
        const long long id = a.ids[k];
        const int64_t dst = a.pre_rows[window_lower_bound(a.in.ids, m, id)] + a.pre_new[k];    // < m_out
        const float *Xt = a.tri + 3 * (int64_t)k;
        const double d0 = (double)Xt[0] - ta[0], d1 = (double)Xt[1] - ta[1], d2 = (double)Xt[2] - ta[2];
        a.out.ids[dst] = id;
        for (int j = 0; j < 3; j++) a.out.X[3 * dst + j] = (Ra[j] * d0 + Ra[3 + j] * d1) + Ra[6 + j] * d2;
        a.out.seen[dst] = 1u << prev | 1u << cur;
        a.out.active[dst] = 0u;
        for (int j = 0; j < kWindowMaxFrames; j++) {
            float2 l = make_float2(0.f, 0.f), q = l;
            if (j == cur) { l = a.t2_left[k]; q = a.t2_right[k]; }
            if (j == prev) { l = a.t1_left[k]; q = a.t1_right[k]; }
            a.out.obs_left[dst * kWindowMaxFrames + j] = l; a.out.obs_right[dst * kWindowMaxFrames + j] = q;
        }
    }
    if (tid < 4) a.out.counts[tid] = tid == 0 ? cur + 1 : (tid == 3 ? 0 : m_out);
}

void launch_window_update(const WindowUpdateArgs &a, hipStream_t st)
{
    hipLaunchKernelGGL(window_update_kernel, dim3(1), dim3(1024), 0, st, a);
}

// ---- window_ba_kernel: the optimiser over a table (W1-W8 of include/svo_abi.h; the numpy twin is tests/_window_ref.py solve()) ---
// ONE workgroup of 1024 lanes; lanes stride the landmarks, and every lane takes the same accept / reject / round decisions
// from sums that are complete in LDS.  A landmark is eliminated by the 3 x 3 Cholesky factor of its own block; what the later
// passes need of it -- L, y and T_if = W_if L^-T per slot -- waits in a device-memory row (kWbaRow doubles).  One LM iteration:
//   wba_build     per landmark: (re-)classification, V, g_x, L, y, T_if; the cost and the counts
//   wba_block     per pair of slots f <= e: the 6 x 6 block of the reduced system (36 sums a lane, + g_f and diag U_f on the
//                 diagonal), wave butterfly, wave totals summed in wave order through LDS
//   wba_chol      the (up to) 42 x 42 factorisation in LDS, column by column; the two triangular solves by one lane
//   wba_trial     back-substitution, the trial points, the cost at the trial estimate
// Sums run in a fixed order and there are no floating-point atomics: the same input gives the same bytes (W8).
// The per-view math, the Huber weight, the 3 x 3 elimination and the cost pair are refine_device.h's, as in refine.hip and ba.hip.
constexpr int kWbaAcc = 48;              // sums a lane carries through one reduction
constexpr int kWbaWaves = kWbaThreads / 64;
constexpr double kWbaTau = 9.488;         // chi-square 95 % point, 4 degrees of freedom: one stereo observation

struct WbaObs { double r[4], A[4][3], Y[3]; bool proj; };

// one observation: Y = R X + t, residuals (left u, v, right u, v), d pixel / dY, projectable (R3)
__device__ inline void wba_eval(const WindowBaArgs &a, const double (&X)[3], const double *P, float2 ol, float2 orr, WbaObs &p)
{
    for (int k = 0; k < 3; k++) p.Y[k] = ((X[0] * P[k * 3] + X[1] * P[k * 3 + 1]) + X[2] * P[k * 3 + 2]) + P[9 + k];
    p.proj = refine_project(a.cam, false, p.Y, ol, p.r, p.A);
    p.proj = refine_project(a.cam, true, p.Y, orr, p.r + 2, p.A + 2) && p.proj;
}

__device__ inline double wba_chi(const WbaObs &p, double s2)
{
    return (((p.r[0] * p.r[0] + p.r[1] * p.r[1]) + p.r[2] * p.r[2]) + p.r[3] * p.r[3]) / s2;
}

// Jx = A R (d residual / dX), Jp = A [I | -[Y]x] (d residual / d xi)
__device__ inline void wba_jx(const WbaObs &p, const double *R, double (&Jx)[4][3])
{
#pragma unroll
    for (int k = 0; k < 4; k++)
        for (int j = 0; j < 3; j++) Jx[k][j] = (p.A[k][0] * R[j] + p.A[k][1] * R[3 + j]) + p.A[k][2] * R[6 + j];
}
__device__ inline void wba_jp(const WbaObs &p, double (&Jp)[4][6])
{
#pragma unroll
    for (int k = 0; k < 4; k++) refine_pose_row(p.A[k], p.Y, Jp[k]);
}

// The first K sums of every lane -> out[0 .. K), complete for every lane on return: wave butterfly, then the wave totals in
// wave order.  pair: acc[0], acc[1] are a (sum, remainder) cost pair and are added as one.
template <int K>
__device__ inline void wba_reduce(double (&acc)[kWbaAcc], bool pair, double *red, double *out)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    __syncthreads();                                        // red and out may still be read from the previous pass
    if (pair) {
        double cs = acc[0], ce = acc[1];
        refine_wave_cost(cs, ce);
        if (lane == 0) { red[wave * kWbaAcc] = cs; red[wave * kWbaAcc + 1] = ce; }
    }
#pragma unroll
    for (int k = 0; k < K; k++) {
        if (pair && k < 2) continue;
        const double ws = wave_allsum_f64(acc[k]);
        if (lane == 0) red[wave * kWbaAcc + k] = ws;
    }
    __syncthreads();
    const int k = threadIdx.x;
    if (pair && k == 0) {
        refine_block_cost(red, kWbaAcc, 1, kWbaWaves, out[0], out[1]);
    } else if (k < K && !(pair && k == 1)) {
        double s = red[k];
        for (int w = 1; w < kWbaWaves; w++) s += red[w * kWbaAcc + k];
        out[k] = s;
    }
    __syncthreads();
}

enum { kWbaInit = 0, kWbaReclass = 1, kWbaKeep = 2 };
// S of wba_build: cost | cost tail | usable landmarks | seen observations | active observations per slot (8)
constexpr int kWbaUsable = 2, kWbaSeen = 3, kWbaFrame = 4, kWbaBuildSums = 12;

struct WbaShared {
    double H[kWbaDim * kWbaDim], A[kWbaDim * kWbaDim], g[kWbaDim], dU[kWbaDim], xi[kWbaDim];
    double P[kWindowMaxFrames * kWindowPose], Pn[kWindowMaxFrames * kWindowPose];
    double red[kWbaWaves * kWbaAcc], S[kWbaAcc], Sn[kWbaAcc];
};

// Per landmark at the accepted estimate (sh.P, Xc) and damping lam: the active mask (kWbaInit: every projectable seen
// observation; kWbaReclass: projectable and c <= tau; kWbaKeep: as it stands; below two active observations the landmark has
// none and returns to its X at entry), then V, g_x, L, y and T_if into its scratch row.  sh.S: the sums listed above.
__device__ void wba_build(const WindowBaArgs &a, WbaShared &sh, int n, int m, double *Xc, int mode, bool robust, double s2, double lam)
{
    double acc[kWbaAcc];
    for (int k = 0; k < kWbaAcc; k++) acc[k] = 0.0;
    const double is2 = 1.0 / s2;
    const uint32_t slots = (1u << n) - 1u;
    for (int i = threadIdx.x; i < m; i += kWbaThreads) {
        const uint32_t seen = a.tab.seen[i] & slots;
        const float2 *ol = a.tab.obs_left + (int64_t)i * kWindowMaxFrames, *orr = a.tab.obs_right + (int64_t)i * kWindowMaxFrames;
        double X[3];
        for (int k = 0; k < 3; k++) X[k] = Xc[3 * (int64_t)i + k];
        acc[kWbaSeen] += (double)__popc(seen);
        uint32_t am = a.act[i];
        if (mode != kWbaKeep) {
            am = 0u;
#pragma unroll 1
            for (int f = 0; f < n; f++) {
                if (!(seen >> f & 1u)) continue;
                WbaObs p;
                wba_eval(a, X, sh.P + f * kWindowPose, ol[f], orr[f], p);
                if (p.proj && (mode == kWbaInit || wba_chi(p, s2) <= kWbaTau)) am |= 1u << f;
            }
            if (__popc(am) < 2) {
                am = 0u;
                for (int k = 0; k < 3; k++) Xc[3 * (int64_t)i + k] = a.tab.X[3 * (int64_t)i + k];
            }
            a.act[i] = am;
        }
        if (am == 0u) continue;
        acc[kWbaUsable] += 1.0;
        double V[6] = {0, 0, 0, 0, 0, 0}, gx[3] = {0, 0, 0};      // V: 00 10 11 20 21 22
#pragma unroll 1
        for (int f = 0; f < n; f++) {
            if (!(am >> f & 1u)) continue;
            WbaObs p;
            wba_eval(a, X, sh.P + f * kWindowPose, ol[f], orr[f], p);
            double w, rho, Jx[4][3];
            refine_huber(robust, wba_chi(p, s2), kWbaTau, w, rho);
            refine_dd_add(acc[0], acc[1], rho, 0.0);
            acc[kWbaFrame + f] += 1.0;
            const double ws = w * is2;
            wba_jx(p, sh.P + f * kWindowPose, Jx);
            int q = 0;
#pragma unroll
            for (int r = 0; r < 3; r++) {
#pragma unroll
                for (int c = 0; c <= r; c++, q++)
                    V[q] += ws * (((Jx[0][r] * Jx[0][c] + Jx[1][r] * Jx[1][c]) + Jx[2][r] * Jx[2][c]) + Jx[3][r] * Jx[3][c]);
                gx[r] += ws * (((Jx[0][r] * p.r[0] + Jx[1][r] * p.r[1]) + Jx[2][r] * p.r[2]) + Jx[3][r] * p.r[3]);
            }
        }
        double L[6];
        const bool ok = refine_chol3(V, lam, L);
        double *row = a.sys + (int64_t)i * kWbaRow;
        for (int k = 0; k < 6; k++) row[k] = L[k];
        refine_fwd3(L, gx, ok, row + 6);
        row[9] = ok ? 1.0 : 0.0;
#pragma unroll 1
        for (int f = 1; f < n; f++) {
            if (!(am >> f & 1u)) continue;
            WbaObs p;
            wba_eval(a, X, sh.P + f * kWindowPose, ol[f], orr[f], p);
            double w, rho, Jx[4][3], Jp[4][6];
            refine_huber(robust, wba_chi(p, s2), kWbaTau, w, rho);
            const double ws = w * is2;
            wba_jx(p, sh.P + f * kWindowPose, Jx);
            wba_jp(p, Jp);
            double *T = row + 10 + 18 * (f - 1);
#pragma unroll
            for (int q = 0; q < 6; q++) {
                double Wq[3];
                for (int j = 0; j < 3; j++) Wq[j] = ws * (((Jp[0][q] * Jx[0][j] + Jp[1][q] * Jx[1][j]) + Jp[2][q] * Jx[2][j]) + Jp[3][q] * Jx[3][j]);
                refine_fwd3(L, Wq, ok, T + q * 3);
            }
        }
    }
    wba_reduce<kWbaBuildSums>(acc, true, sh.red, sh.S);
}

// Block (f, e), 1 <= f <= e < n, of the reduced system into sh.H (both triangles): -sum T_if T_ie^T, on the diagonal + sum U_f,
// with g_f = sum (g_pf - T_if y_i) and diag sum U_f.  The rows of wba_build must be complete (a barrier lies between).
__device__ void wba_block(const WindowBaArgs &a, WbaShared &sh, int m, const double *Xc, int f, int e, bool robust, double s2)
{
    double acc[kWbaAcc];
    for (int k = 0; k < kWbaAcc; k++) acc[k] = 0.0;
    const double is2 = 1.0 / s2;
    const uint32_t need = 1u << f | 1u << e;
    for (int i = threadIdx.x; i < m; i += kWbaThreads) {
        const uint32_t am = a.act[i];
        if ((am & need) != need) continue;
        const double *row = a.sys + (int64_t)i * kWbaRow;
        const double *Tf = row + 10 + 18 * (f - 1), *Te = row + 10 + 18 * (e - 1);
#pragma unroll
        for (int q = 0; q < 6; q++)
#pragma unroll
            for (int c = 0; c < 6; c++) acc[q * 6 + c] -= (Tf[q * 3] * Te[c * 3] + Tf[q * 3 + 1] * Te[c * 3 + 1]) + Tf[q * 3 + 2] * Te[c * 3 + 2];
        if (f != e) continue;
        double X[3];
        for (int k = 0; k < 3; k++) X[k] = Xc[3 * (int64_t)i + k];
        WbaObs p;
        wba_eval(a, X, sh.P + f * kWindowPose, a.tab.obs_left[(int64_t)i * kWindowMaxFrames + f], a.tab.obs_right[(int64_t)i * kWindowMaxFrames + f], p);
        double w, rho, Jp[4][6];
        refine_huber(robust, wba_chi(p, s2), kWbaTau, w, rho);
        const double ws = w * is2;
        wba_jp(p, Jp);
#pragma unroll
        for (int q = 0; q < 6; q++) {
#pragma unroll
            for (int c = 0; c < 6; c++) {
                const double u = ws * (((Jp[0][q] * Jp[0][c] + Jp[1][q] * Jp[1][c]) + Jp[2][q] * Jp[2][c]) + Jp[3][q] * Jp[3][c]);
                acc[q * 6 + c] += u;
                if (c == q) acc[42 + q] += u;
            }
            const double gp = ws * (((Jp[0][q] * p.r[0] + Jp[1][q] * p.r[1]) + Jp[2][q] * p.r[2]) + Jp[3][q] * p.r[3]);
            acc[36 + q] += gp - ((Tf[q * 3] * row[6] + Tf[q * 3 + 1] * row[7]) + Tf[q * 3 + 2] * row[8]);
        }
    }
    wba_reduce<kWbaAcc>(acc, false, sh.red, sh.Sn);
    const int k = threadIdx.x;
    if (k < 36) {
        const int q = k / 6, c = k % 6;
        sh.H[(6 * (f - 1) + q) * kWbaDim + 6 * (e - 1) + c] = sh.Sn[k];
        if (f != e) sh.H[(6 * (e - 1) + c) * kWbaDim + 6 * (f - 1) + q] = sh.Sn[k];
    } else if (k < 42 && f == e) sh.g[6 * (f - 1) + k - 36] = sh.Sn[k];
    else if (k < 48 && f == e) sh.dU[6 * (f - 1) + k - 42] = sh.Sn[k];
    __syncthreads();
}

__device__ void wba_system(const WindowBaArgs &a, WbaShared &sh, int n, int m, const double *Xc, bool robust, double s2)
{
    for (int f = 1; f < n; f++)
        for (int e = f; e < n; e++) wba_block(a, sh, m, Xc, f, e, robust, s2);
}

// sh.A = sh.H + lam diag(sh.dU), factored in place (lower triangle) column by column; false unless every pivot is > 0.
// Every lane returns the same answer.
__device__ bool wba_chol(WbaShared &sh, int D, double lam)
{
    for (int idx = threadIdx.x; idx < D * D; idx += kWbaThreads) {
        const int i = idx / D, j = idx % D;
        sh.A[i * kWbaDim + j] = sh.H[i * kWbaDim + j] + (i == j ? lam * sh.dU[i] : 0.0);
    }
    bool ok = true;
    for (int k = 0; k < D; k++) {
        __syncthreads();
        const double piv = sh.A[k * kWbaDim + k];
        ok = ok && piv > 0.0;
        const double d = sqrt(piv > 0.0 ? piv : 1.0);
        __syncthreads();
        const int t = threadIdx.x;
        if (t == k) sh.A[k * kWbaDim + k] = d;
        else if (t > k && t < D) sh.A[t * kWbaDim + k] = sh.A[t * kWbaDim + k] / d;
        __syncthreads();
        for (int idx = threadIdx.x; idx < D * D; idx += kWbaThreads) {
            const int i = idx / D, j = idx % D;
            if (j > k && i >= j) sh.A[i * kWbaDim + j] -= sh.A[i * kWbaDim + k] * sh.A[j * kWbaDim + k];
        }
    }
    __syncthreads();
    return ok;
}

// sh.xi = -(L L^T)^-1 sh.g by one lane; complete for every lane on return
__device__ void wba_solve(WbaShared &sh, int D)
{
    if (threadIdx.x == 0) {
        for (int i = 0; i < D; i++) {
            double s = -sh.g[i];
            for (int k = 0; k < i; k++) s -= sh.A[i * kWbaDim + k] * sh.xi[k];
            sh.xi[i] = s / sh.A[i * kWbaDim + i];
        }
        for (int i = D - 1; i >= 0; i--) {
            double s = sh.xi[i];
            for (int k = i + 1; k < D; k++) s -= sh.A[k * kWbaDim + i] * sh.xi[k];
            sh.xi[i] = s / sh.A[i * kWbaDim + i];
        }
    }
    __syncthreads();
}

// A trial step: dX_i = -L^-T (y_i + sum_f T_if^T xi_f) from the rows of wba_build, the trial points to Xt (EVERY row), the
// cost at (sh.Pn, Xt) over the standing masks.  sh.Sn: cost | tail | active observations not projectable there | largest |dX|^2.
__device__ void wba_trial(const WindowBaArgs &a, WbaShared &sh, int n, int m, const double *Xc, double *Xt, bool robust, double s2)
{
    double acc[kWbaAcc];
    for (int k = 0; k < 4; k++) acc[k] = 0.0;
    double step = 0.0;
    for (int i = threadIdx.x; i < m; i += kWbaThreads) {
        const uint32_t am = a.act[i];
        double X[3];
        for (int k = 0; k < 3; k++) X[k] = Xc[3 * (int64_t)i + k];
        if (am != 0u) {
            const double *row = a.sys + (int64_t)i * kWbaRow;
            double z[3] = {row[6], row[7], row[8]};
#pragma unroll 1
            for (int f = 1; f < n; f++) {
                if (!(am >> f & 1u)) continue;
                const double *T = row + 10 + 18 * (f - 1), *xi = sh.xi + 6 * (f - 1);
                for (int j = 0; j < 3; j++) {
                    double v = T[j] * xi[0];
                    for (int q = 1; q < 6; q++) v += T[q * 3 + j] * xi[q];
                    z[j] += v;
                }
            }
            double dX[3];
            refine_back3(row, z, row[9] != 0.0, dX);
            for (int k = 0; k < 3; k++) X[k] = X[k] + dX[k];
            step = fmax(step, (dX[0] * dX[0] + dX[1] * dX[1]) + dX[2] * dX[2]);
        }
        for (int k = 0; k < 3; k++) Xt[3 * (int64_t)i + k] = X[k];
#pragma unroll 1
        for (int f = 0; f < n; f++) {
            if (!(am >> f & 1u)) continue;
            WbaObs p;
            wba_eval(a, X, sh.Pn + f * kWindowPose, a.tab.obs_left[(int64_t)i * kWindowMaxFrames + f], a.tab.obs_right[(int64_t)i * kWindowMaxFrames + f], p);
            if (!p.proj) { acc[2] += 1.0; continue; }
            double w, rho;
            refine_huber(robust, wba_chi(p, s2), kWbaTau, w, rho);
            refine_dd_add(acc[0], acc[1], rho, 0.0);
        }
    }
#pragma unroll
    for (int mk = 1; mk < 64; mk <<= 1) step = fmax(step, __shfl_xor(step, mk, 64));
    wba_reduce<3>(acc, true, sh.red, sh.Sn);
    // the largest step: wave maxima through red (free again after the reduction's last barrier)
    if ((threadIdx.x & 63) == 0) sh.red[threadIdx.x >> 6] = step;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = sh.red[0];
        for (int w = 1; w < kWbaWaves; w++) s = fmax(s, sh.red[w]);
        sh.Sn[3] = s;
    }
    __syncthreads();
}

__global__ __launch_bounds__(kWbaThreads) void window_ba_kernel(WindowBaArgs a)
{
    __shared__ WbaShared sh;
    const int tid = threadIdx.x;
    if (blockIdx.x != 0) return;
    svo_window_result *res = a.res;
    int n = a.tab.counts[0], m = a.tab.counts[1];
    n = n < 0 ? 0 : (n > kWindowMaxFrames ? kWindowMaxFrames : n);
    m = m < 0 ? 0 : (m > a.cap ? a.cap : m);
    const int D = 6 * (n - 1);
    for (int k = tid; k < kWbaDim * kWbaDim; k += kWbaThreads) { res->info[k] = 0.0; sh.H[k] = 0.0; }
    if (n < 2) {
        if (tid == 0) {
            res->status = SVO_REFINE_SKIPPED; res->n_frames = n; res->n_landmarks = m; res->n_usable = 0; res->n_obs = 0; res->n_active = 0;
            res->iters = 0; res->_pad = 0; res->cost_first = 0.0; res->cost_last = 0.0;
            for (int f = 0; f < kWindowMaxFrames; f++) res->frame_active[f] = 0;
        }
        return;
    }
    if (tid < kWindowMaxFrames * kWindowPose) { sh.P[tid] = a.tab.poses[tid]; sh.Pn[tid] = sh.P[tid]; }
    if (tid < kWbaDim) { sh.g[tid] = 0.0; sh.dU[tid] = 0.0; sh.xi[tid] = 0.0; }
    double *Xc = a.Xa, *Xt = a.Xb;
    for (int i = tid; i < m; i += kWbaThreads) {
        for (int k = 0; k < 3; k++) Xc[3 * (int64_t)i + k] = a.tab.X[3 * (int64_t)i + k];
        a.act[i] = 0u;
    }
    __syncthreads();
    const double s2 = a.sigma * a.sigma;
    int total = 0;
    double cost_first = 0.0, cost = 0.0, cost_lo = 0.0;
    for (int rd = 0; rd < a.rounds; rd++) {
        const bool robust = rd < 2;
        double lam = 1e-4;
        for (int k = 0; k < a.iters; k++) {
            total++;
            wba_build(a, sh, n, m, Xc, k > 0 ? kWbaKeep : (rd == 0 ? kWbaInit : kWbaReclass), robust, s2, lam);
            if (k == 0) {
                cost = sh.S[0]; cost_lo = sh.S[1];
                if (rd == 0) cost_first = cost;
            }
            wba_system(a, sh, n, m, Xc, robust, s2);
            bool accepted = false;
            double nx = 0.0, step2 = 0.0;
            if (wba_chol(sh, D, lam)) {
                wba_solve(sh, D);
                if (tid >= 1 && tid < n) {                  // slot tid: (R, t) <- exp(xi) (R, t)
                    double xi[6], E[9], Vr[3], R[9], t[3], Rn[9], Et[3];
                    for (int q = 0; q < 6; q++) xi[q] = sh.xi[6 * (tid - 1) + q];
                    for (int q = 0; q < 9; q++) R[q] = sh.P[tid * kWindowPose + q];
                    for (int q = 0; q < 3; q++) t[q] = sh.P[tid * kWindowPose + 9 + q];
                    refine_se3_exp(xi, E, Vr);
                    refine_mm3(E, R, Rn);
                    refine_mv3(E, t, Et);
                    for (int q = 0; q < 9; q++) sh.Pn[tid * kWindowPose + q] = Rn[q];
                    for (int q = 0; q < 3; q++) sh.Pn[tid * kWindowPose + 9 + q] = Et[q] + Vr[q];
                }
                __syncthreads();
                wba_trial(a, sh, n, m, Xc, Xt, robust, s2);
                accepted = sh.Sn[2] == 0.0 && (sh.Sn[0] < cost || (sh.Sn[0] == cost && sh.Sn[1] < cost_lo));
                for (int q = 0; q < D; q++) nx += sh.xi[q] * sh.xi[q];
                step2 = sh.Sn[3];
            }
            if (accepted) {
                cost = sh.Sn[0]; cost_lo = sh.Sn[1];
                __syncthreads();                            // everybody has read Sn and P
                if (tid < kWindowMaxFrames * kWindowPose) sh.P[tid] = sh.Pn[tid];
                { double *sw = Xc; Xc = Xt; Xt = sw; }
                __syncthreads();
                lam = lam / 10.0 > 1e-12 ? lam / 10.0 : 1e-12;
                if (sqrt(nx) < 1e-10 && sqrt(step2) < 1e-9) break;
            } else {
                lam *= 10.0;
                if (lam > 1e10) break;
            }
        }
    }
    // the last re-classification; info = the reduced H at lam = 0 over the active set; the outcome (W7)
    wba_build(a, sh, n, m, Xc, kWbaReclass, false, s2, 0.0);
    wba_system(a, sh, n, m, Xc, false, s2);
    const bool pd = wba_chol(sh, D, 0.0);
    bool fin = refine_finite(cost_first) && refine_finite(cost);
    for (int k = tid; k < D * D; k += kWbaThreads) fin = fin && refine_finite(sh.H[(k / D) * kWbaDim + k % D]);
    if (tid < n * kWindowPose) fin = fin && refine_finite(sh.P[tid]);
    for (int i = tid; i < m; i += kWbaThreads)
        for (int k = 0; k < 3; k++) fin = fin && refine_finite(Xc[3 * (int64_t)i + k]);
    fin = __syncthreads_and(fin ? 1 : 0) != 0;
    bool fed = true;
    int n_active = 0;
    for (int f = 0; f < n; f++) {
        const int c = (int)sh.S[kWbaFrame + f];
        n_active += c;
        if (f >= 1) fed = fed && c >= a.min_obs;
    }
    const bool applied = fed && pd && fin;
    for (int k = tid; k < D * D; k += kWbaThreads) res->info[(k / D) * kWbaDim + k % D] = sh.H[(k / D) * kWbaDim + k % D];
    if (applied) {
        if (tid < n * kWindowPose) a.tab.poses[tid] = sh.P[tid];
        for (int i = tid; i < m; i += kWbaThreads) {
            for (int k = 0; k < 3; k++) a.tab.X[3 * (int64_t)i + k] = Xc[3 * (int64_t)i + k];
            a.tab.active[i] = a.act[i];
        }
    }
    if (applied && a.record_pose && tid < 16) {           // the step's pose: world from camera of the newest slot
        const double *R = sh.P + (n - 1) * kWindowPose, *t = R + 9;
        const int i = tid >> 2, j = tid & 3;
        double v = i == 3 ? (j == 3 ? 1.0 : 0.0) : R[j * 3 + i];
        if (i < 3 && j == 3) v = -((R[i] * t[0] + R[3 + i] * t[1]) + R[6 + i] * t[2]);
        a.record_pose[tid] = v;
    }
    if (tid == 0) {
        res->status = applied ? SVO_REFINE_APPLIED : SVO_REFINE_KEPT_PNP;
        res->n_frames = n; res->n_landmarks = m; res->n_usable = (int)sh.S[kWbaUsable]; res->n_obs = (int)sh.S[kWbaSeen];
        res->n_active = n_active; res->iters = total; res->_pad = 0;
        for (int f = 0; f < kWindowMaxFrames; f++) res->frame_active[f] = f < n ? (int)sh.S[kWbaFrame + f] : 0;
        res->cost_first = cost_first; res->cost_last = cost;
    }
}

void launch_window_ba(const WindowBaArgs &a, hipStream_t st)
{
    hipLaunchKernelGGL(window_ba_kernel, dim3(1), dim3(kWbaThreads), 0, st, a);
}

// ---- the landmark table on the host side.  Its eight columns, in WindowTable's (and svo_window_table's) order, are defined
// HERE and nowhere else: bytes per table and bytes per row, and one bit each for the calls that move only some of them.
constexpr size_t kTabBytes[8][2] = {{sizeof(int) * 4, 0}, {sizeof(double) * kWindowMaxFrames * kWindowPose, 0}, {0, sizeof(long long)},
                                    {0, sizeof(double) * 3}, {0, sizeof(uint32_t)}, {0, sizeof(uint32_t)},
                                    {0, sizeof(float2) * kWindowMaxFrames}, {0, sizeof(float2) * kWindowMaxFrames}};
enum : unsigned { kTabCounts = 1, kTabPoses = 2, kTabIds = 4, kTabX = 8, kTabActive = 32, kTabAll = 255 };     // bit k = column k
struct TableCols { uint8_t *p[8]; };

template <typename Table>                                     // svo_window_table or WindowTable: the same eight members
static TableCols window_cols(const Table &t)
{
    return TableCols{{(uint8_t *)t.counts, (uint8_t *)t.poses, (uint8_t *)t.ids, (uint8_t *)t.X, (uint8_t *)t.seen, (uint8_t *)t.active,
                      (uint8_t *)t.obs_left, (uint8_t *)t.obs_right}};
}
static WindowTable window_table_of(const TableCols &c)
{
    return WindowTable{(int *)c.p[0], (double *)c.p[1], (long long *)c.p[2], (double *)c.p[3], (uint32_t *)c.p[4], (uint32_t *)c.p[5],
                       (float2 *)c.p[6], (float2 *)c.p[7]};
}
static size_t window_col_bytes(int k, size_t rows) { return kTabBytes[k][0] + kTabBytes[k][1] * rows; }

// room for the columns `cols` of a table of `rows` rows (a column outside `cols` gets none): their offsets
static void window_table_cut(BlockCut &cut, size_t rows, unsigned cols, size_t (&at)[8])
{
    for (int k = 0; k < 8; k++) at[k] = cut.add(cols >> k & 1u ? window_col_bytes(k, rows) : 0);
}
static WindowTable window_table_at(uint8_t *s, const size_t (&at)[8])
{
    TableCols c;
    for (int k = 0; k < 8; k++) c.p[k] = s + at[k];
    return window_table_of(c);
}
// the caller's columns `cols`, `rows` rows of them, into the scratch at s + at[] (HOST) or as they are (DEVICE), in column
// order; a column outside `cols` keeps the caller's pointer
static int window_table_in(svo_ctx *ctx, const svo_window_table &t, uint8_t *s, const size_t (&at)[8], size_t rows, unsigned cols, int mem,
                           WindowTable *d)
{
    TableCols c = window_cols(t);
    for (int k = 0; k < 8; k++) {
        if (!(cols >> k & 1u)) continue;
        const uint8_t *p;
        SVO_TRY(to_device(ctx, (const uint8_t *)c.p[k], s + at[k], window_col_bytes(k, rows), mem, &p));
        c.p[k] = (uint8_t *)p;
    }
    *d = window_table_of(c);
    return SVO_OK;
}
// `rows` rows of the device table's columns `cols` into the caller's, in column order; a null column is left out
static int window_table_out(svo_ctx *ctx, const svo_window_table &t, const WindowTable &d, size_t rows, unsigned cols, int mem)
{
    const TableCols dst = window_cols(t), src = window_cols(d);
    for (int k = 0; k < 8; k++)
        if (cols >> k & 1u) SVO_TRY(from_device(ctx, dst.p[k], (const uint8_t *)src.p[k], window_col_bytes(k, rows), mem));
    return SVO_OK;
}

// ---- the fused step (svo_set_window_ba): the online chain's table, two buffers swapped per step, and both kernels on it
struct WindowCut { size_t tab[2][8], pre_rows, pre_new, Xa, Xb, sys, act, res, end; };
static WindowCut window_cut(int frames, int kcap)
{
    const size_t rows = (size_t)(frames - 1) * (size_t)kcap;
    BlockCut cut;
    WindowCut c;
    for (int t = 0; t < 2; t++) window_table_cut(cut, rows, kTabAll, c.tab[t]);
    c.pre_rows = cut.add(sizeof(int) * (rows + 1)); c.pre_new = cut.add(sizeof(int) * ((size_t)kcap + 1));
    c.Xa = cut.add(sizeof(double) * 3 * rows); c.Xb = cut.add(sizeof(double) * 3 * rows); c.sys = cut.add(sizeof(double) * kWbaRow * rows);
    c.act = cut.add(sizeof(uint32_t) * rows); c.res = cut.add(sizeof(svo_window_result)); c.end = cut.total();
    return c;
}

int window_alloc(svo_ctx *ctx, int frames)
{
    SVO_HIP(hipSetDevice(ctx->device));
    if (dev_reserve(ctx, &ctx->win.block, window_cut(frames, ctx->cfg.max_keypoints).end) != SVO_OK) return SVO_ERR_HIP;
    return SVO_OK;
}

// after launch_finalize_chain of an online step, on its stream: the update on the pair's tracks, then the optimiser on the new table
int window_fused_step(svo_ctx *ctx, const double *pose0_host, hipStream_t st)
{
    const int W = ctx->win.frames, K = ctx->cfg.max_keypoints;
    const WindowCut c = window_cut(W, K);
    uint8_t *s = ctx->win.block.base;
    const int in = ctx->win.cur, out = in ^ 1;
    WindowUpdateArgs u{};
    u.frames = W; u.cap = (W - 1) * K;
    u.in = window_table_at(s, c.tab[in]); u.out = window_table_at(s, c.tab[out]);
    u.t1_left = ctx->cmp[0]; u.t1_right = ctx->cmp[1]; u.t2_right = ctx->cmp[2]; u.t2_left = ctx->cmp[3];
    u.ids = ctx->carry.trk_id; u.tri = ctx->X3; u.n_trk = K; u.n_trk_dev = ctx->m_out;
    u.ok = &ctx->d_results[0].ok; u.clear_in = ctx->win.clear ? 1 : 0;
    u.pose_a_by_value = 1;
    memcpy(u.pose_a_value, pose_from_host(pose0_host).m, sizeof(u.pose_a_value));
    u.pose_b = ctx->d_results[0].pose;
    u.pre_rows = (int *)(s + c.pre_rows); u.pre_new = (int *)(s + c.pre_new);
    launch_window_update(u, st);
    timing_mark(ctx, "win_update");
    WindowBaArgs b{};
    b.tab = u.out; b.cap = u.cap;
    b.cam = stereo_cam(ctx->cfg.P1, ctx->cfg.P2);
    b.rounds = ctx->win.rounds; b.iters = ctx->win.iters; b.min_obs = ctx->win.min_obs; b.sigma = ctx->win.sigma;
    b.Xa = (double *)(s + c.Xa); b.Xb = (double *)(s + c.Xb); b.sys = (double *)(s + c.sys); b.act = (uint32_t *)(s + c.act);
    b.res = (svo_window_result *)(s + c.res);
    b.record_pose = ctx->d_results[0].pose;
    launch_window_ba(b, st);
    timing_mark(ctx, "win_ba");
    ctx->win.cur = out; ctx->win.clear = false;
    return SVO_OK;
}

// read-backs of the online chain's table and of the last step's outcome (HOST)
int window_read(svo_ctx *ctx, const svo_window_table *out, int cap)
{
    const WindowCut c = window_cut(ctx->last.window_frames, ctx->cfg.max_keypoints);
    const WindowTable t = window_table_at(ctx->win.block.base, c.tab[ctx->win.cur]);
    SVO_TRY(window_table_out(ctx, *out, t, 0, kTabCounts, SVO_MEM_HOST));
    SVO_TRY(io_done(ctx, SVO_MEM_HOST));
    const int m = out->counts[1];
    if (!out->ids && !out->X && !out->seen && !out->active && !out->obs_left && !out->obs_right && !out->poses) return SVO_OK;
    SVO_ARG(m <= cap, "row capacity too small");
    SVO_TRY(window_table_out(ctx, *out, t, (size_t)m, kTabAll & ~kTabCounts, SVO_MEM_HOST));
    return io_done(ctx, SVO_MEM_HOST);
}

int window_read_result(svo_ctx *ctx, svo_window_result *res)
{
    const WindowCut c = window_cut(ctx->last.window_frames, ctx->cfg.max_keypoints);
    SVO_TRY(from_device(ctx, res, (const svo_window_result *)(ctx->win.block.base + c.res), (size_t)1, SVO_MEM_HOST));
    return io_done(ctx, SVO_MEM_HOST);
}

// ---- svo_window_update: the kernel on a caller's tables
int stage_window_update(svo_ctx *ctx, int frames, const svo_window_table *in, const svo_window_table *out, int cap, const svo_pt2f *t1_left,
                        const svo_pt2f *t1_right, const svo_pt2f *t2_left, const svo_pt2f *t2_right, const int64_t *ids, const svo_pt3f *tri,
                        int n_trk, const double *pose_a, const double *pose_b, int mem)
{
    SVO_ARG(frames >= 2 && frames <= kWindowMaxFrames, "frames outside 2..SVO_WINDOW_MAX_FRAMES");
    SVO_ARG(cap >= 1 && cap <= (1 << 21), "cap outside 1..2^21");
    SVO_ARG(n_trk >= 0 && n_trk <= (1 << 20), "bad n_trk");
    SVO_ARG(in && out && in->counts && out->counts && in->poses && out->poses, "null table");
    SVO_ARG(in->ids && in->X && in->seen && in->active && in->obs_left && in->obs_right, "null input table column");
    SVO_ARG(out->ids && out->X && out->seen && out->active && out->obs_left && out->obs_right, "null output table column");
    SVO_ARG(n_trk == 0 || (t1_left && t1_right && t2_left && t2_right && ids && tri), "null track list");
    SVO_ARG(pose_a && pose_b, "null pose");
    SVO_ARG(mem == SVO_MEM_HOST || mem == SVO_MEM_DEVICE, "mem must be SVO_MEM_HOST or SVO_MEM_DEVICE");
    const bool host = mem == SVO_MEM_HOST;
    size_t m_in = 0;
    if (host) {
        SVO_ARG(in->counts[0] >= 0 && in->counts[0] <= frames, "the table holds more frames than `frames`");
        SVO_ARG(in->counts[1] >= 0 && in->counts[1] <= cap, "the table holds more rows than `cap`");
        m_in = in->counts[0] > 0 ? (size_t)in->counts[1] : 0;
    }
    const size_t nt = (size_t)n_trk, nc = (size_t)cap, hm = host ? m_in : 0, ht = host ? nt : 0;
    BlockCut cut;
    const size_t s_rows = cut.add(sizeof(int) * (nc + 1)), s_new = cut.add(sizeof(int) * (nt + 1));
    size_t at[2][8];                                          // HOST: the two tables' scratch, m_in and cap rows
    window_table_cut(cut, hm, host ? kTabAll : 0u, at[0]);
    window_table_cut(cut, nc, host ? kTabAll : 0u, at[1]);
    const size_t i_t1l = cut.add(sizeof(float2) * ht), i_t1r = cut.add(sizeof(float2) * ht), i_t2l = cut.add(sizeof(float2) * ht),
                 i_t2r = cut.add(sizeof(float2) * ht), i_ids = cut.add(sizeof(long long) * ht), i_tri = cut.add(sizeof(float) * 3 * ht),
                 i_pa = cut.add(host ? sizeof(double) * 16 : 0), i_pb = cut.add(host ? sizeof(double) * 16 : 0);
    SVO_HIP(hipSetDevice(ctx->device));
    if (dev_reserve(ctx, &ctx->win.update_stage, cut.total()) != SVO_OK) return SVO_ERR_HIP;
    uint8_t *s = ctx->win.update_stage.base;
    WindowUpdateArgs a{};
    a.frames = frames; a.cap = cap; a.n_trk = n_trk;
    a.pre_rows = (int *)(s + s_rows); a.pre_new = (int *)(s + s_new);
    SVO_TRY(window_table_in(ctx, *in, s, at[0], hm, kTabAll, mem, &a.in));
    a.out = host ? window_table_at(s, at[1]) : window_table_of(window_cols(*out));
    SVO_TRY(to_device(ctx, (const float2 *)t1_left, (float2 *)(s + i_t1l), nt, mem, &a.t1_left));
    SVO_TRY(to_device(ctx, (const float2 *)t1_right, (float2 *)(s + i_t1r), nt, mem, &a.t1_right));
    SVO_TRY(to_device(ctx, (const float2 *)t2_left, (float2 *)(s + i_t2l), nt, mem, &a.t2_left));
    SVO_TRY(to_device(ctx, (const float2 *)t2_right, (float2 *)(s + i_t2r), nt, mem, &a.t2_right));
    SVO_TRY(to_device(ctx, (const long long *)ids, (long long *)(s + i_ids), nt, mem, &a.ids));
    SVO_TRY(to_device(ctx, (const float *)tri, (float *)(s + i_tri), 3 * nt, mem, &a.tri));
    SVO_TRY(to_device(ctx, pose_a, (double *)(s + i_pa), (size_t)16, mem, &a.pose_a));
    SVO_TRY(to_device(ctx, pose_b, (double *)(s + i_pb), (size_t)16, mem, &a.pose_b));
    launch_window_update(a, ctx->stream);
    SVO_HIP(hipGetLastError());
    if (!host) return SVO_OK;
    const int *h;
    SVO_TRY(count_fetch(ctx, 0, a.out.counts, 4));
    SVO_TRY(counts_wait(ctx, &h));
    for (int k = 0; k < 4; k++) out->counts[k] = h[k];
    if (h[2] > cap) { ctx->err = "bad argument: cap is too small for the updated table (rows needed: " + std::to_string(h[2]) + ")"; return SVO_ERR_ARG; }
    SVO_TRY(window_table_out(ctx, *out, a.out, (size_t)h[1], kTabAll & ~kTabCounts, mem));
    return io_done(ctx, mem);
}

// ---- svo_window_ba: the optimiser on a caller's table
int stage_window_ba(svo_ctx *ctx, const svo_window_table *tab, int cap, const double *P1, const double *P2, int rounds, int iters,
                    double sigma_px, int min_obs, svo_window_result *res, int mem)
{
    SVO_ARG(cap >= 1 && cap <= (1 << 21), "cap outside 1..2^21");
    SVO_ARG(tab && tab->counts && tab->poses && tab->ids && tab->X && tab->seen && tab->active && tab->obs_left && tab->obs_right, "null table");
    SVO_ARG(P1 && P2 && res, "null P1 / P2 / result");
    SVO_TRY(check_optimiser_params(ctx, rounds, iters, sigma_px));
    SVO_ARG(min_obs >= 1, "min_obs < 1");
    SVO_ARG(mem == SVO_MEM_HOST || mem == SVO_MEM_DEVICE, "mem must be SVO_MEM_HOST or SVO_MEM_DEVICE");
    const bool host = mem == SVO_MEM_HOST;
    size_t hm = 0;
    if (host) {
        SVO_ARG(tab->counts[0] >= 0 && tab->counts[0] <= kWindowMaxFrames, "the table holds more than SVO_WINDOW_MAX_FRAMES frames");
        SVO_ARG(tab->counts[1] >= 0 && tab->counts[1] <= cap, "the table holds more rows than `cap`");
        hm = (size_t)tab->counts[1];
    }
    const size_t nc = (size_t)cap;
    const unsigned read = kTabAll & ~kTabIds;                 // the optimiser does not read the ids
    BlockCut cut;
    const size_t s_xa = cut.add(sizeof(double) * 3 * nc), s_xb = cut.add(sizeof(double) * 3 * nc), s_sys = cut.add(sizeof(double) * kWbaRow * nc),
                 s_act = cut.add(sizeof(uint32_t) * nc), s_res = cut.add(host ? sizeof(svo_window_result) : 0);
    size_t at[8];
    window_table_cut(cut, hm, host ? read : 0u, at);
    SVO_HIP(hipSetDevice(ctx->device));
    if (dev_reserve(ctx, &ctx->win.ba_stage, cut.total()) != SVO_OK) return SVO_ERR_HIP;
    uint8_t *s = ctx->win.ba_stage.base;
    WindowBaArgs a{};
    a.cap = cap;
    a.cam = stereo_cam(P1, P2);
    a.rounds = rounds; a.iters = iters; a.min_obs = min_obs; a.sigma = sigma_px;
    a.Xa = (double *)(s + s_xa); a.Xb = (double *)(s + s_xb); a.sys = (double *)(s + s_sys); a.act = (uint32_t *)(s + s_act);
    a.res = host ? (svo_window_result *)(s + s_res) : res;
    SVO_TRY(window_table_in(ctx, *tab, s, at, hm, read, mem, &a.tab));
    launch_window_ba(a, ctx->stream);
    SVO_HIP(hipGetLastError());
    if (!host) return SVO_OK;
    SVO_TRY(from_device(ctx, res, (const svo_window_result *)a.res, (size_t)1, mem));
    SVO_TRY(window_table_out(ctx, *tab, a.tab, hm, kTabPoses | kTabX | kTabActive, mem));
    return io_done(ctx, mem);
}

}  // namespace svo
