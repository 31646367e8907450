// pose_device.h -- the rigid-pose algebra the pose stage ends in, written ONCE: 4 x 4 poses (row-major doubles), their products
// and inverses, the Euler-angle and translation gates, the cleared step record and the one-wave chain product, named after the
// numpy twin (tests/_pose_ref.py: mul4, inv_t4, inv_rt, euler, gates, chain), which each equals bit for bit.  The library is built with
// -ffp-contract=off: an expression gives the same bits wherever it is inlined AS LONG AS ITS ASSOCIATION ORDER STAYS -- do not re-associate.
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include "../../include/svo_abi.h"

namespace svo {
// a pose that travels BY VALUE in a kernel's argument block: a launch queued behind many others keeps the pose it was given
struct Pose16 { double m[16]; };
__host__ __device__ inline void pose_identity16(double *P) { for (int i = 0; i < 16; i++) P[i] = (i % 5 == 0) ? 1.0 : 0.0; }
__host__ __device__ inline Pose16 pose_from_host(const double *host_or_null)     // the caller's host pose, or the identity
{
    Pose16 p;
    pose_identity16(p.m);
    if (host_or_null) for (int i = 0; i < 16; i++) p.m[i] = host_or_null[i];
    return p;
}
// One element of C = A B: the row (a0 a1 a2 a3) of A times the column b[0], b[4], b[8], b[12] of B, in the CHAIN'S ORDER:
// k ascending, separate multiply and add, from 0.  Every product of poses in the library is made of this line.
__host__ __device__ __forceinline__ double pose_mul4_elem(double a0, double a1, double a2, double a3, const double *b)
{
    double s = 0;
    s += a0 * b[0]; s += a1 * b[4]; s += a2 * b[8]; s += a3 * b[12];
    return s;
}
__host__ __device__ inline void pose_mul4(const double *A, const double *B, double *C)     // mul4; C aliases neither A nor B
{
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) C[i * 4 + j] = pose_mul4_elem(A[i * 4], A[i * 4 + 1], A[i * 4 + 2], A[i * 4 + 3], B + j);
}
// inv([R t; 0 1]) in closed form (inv_rt), a step's T_rel_inv: R^T and -(R^T t), each sum LEFT TO RIGHT, negated last
__host__ __device__ inline void pose_inv_rt(const double *R, const double *t, double *Ti)
{
    Ti[0] = R[0]; Ti[1] = R[3]; Ti[2] = R[6];
    Ti[4] = R[1]; Ti[5] = R[4]; Ti[6] = R[7];
    Ti[8] = R[2]; Ti[9] = R[5]; Ti[10] = R[8];
    Ti[3] = -(R[0] * t[0] + R[3] * t[1] + R[6] * t[2]);
    Ti[7] = -(R[1] * t[0] + R[4] * t[1] + R[7] * t[2]);
    Ti[11] = -(R[2] * t[0] + R[5] * t[1] + R[8] * t[2]);
    Ti[12] = 0; Ti[13] = 0; Ti[14] = 0; Ti[15] = 1;
}
// Rule T4 (inv_t4): camera from world of a world-from-camera 4 x 4 P.  Element e of (R row-major, then t), 12 values:
// R = Rw^T, t_i = -((R_i0 tw_0 + R_i1 tw_1) + R_i2 tw_2) -- the (a + b) + c form, negated last; and the same as a 4 x 4.
__host__ __device__ inline double pose_inv_t4_elem(const double *P, int e)
{
    if (e < 9) return P[(e % 3) * 4 + e / 3];
    const int i = e - 9;
    return -((P[i] * P[3] + P[4 + i] * P[7]) + P[8 + i] * P[11]);
}
__host__ __device__ inline void pose_inv_t4(const double *P, double *out)
{
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) out[i * 4 + j] = pose_inv_t4_elem(P, i * 3 + j);
        out[i * 4 + 3] = pose_inv_t4_elem(P, 9 + i);
    }
    out[12] = 0; out[13] = 0; out[14] = 0; out[15] = 1;
}
// The rotation gate (euler + gates): rotationMatrixToEulerAngles (reference src/tracking.cpp:440-463) on the 3 x 3 rotation
// whose rows are ld doubles apart (3: a rotation matrix, 4: the rotation of a pose), every angle below 0.1 (:308).  The
// angles are FLOATS HOLDING DOUBLE EXPRESSIONS, sy < 1e-6 takes the singular branch, and the test order is ey, ex, ez.
__host__ __device__ inline bool pose_euler_gate(const double *R, int ld)
{
    const float sy = (float)sqrt(R[0] * R[0] + R[ld] * R[ld]);
    const bool singular = (double)sy < 1e-6;
    float ex, ey, ez;
    if (!singular) {
        ex = (float)atan2(R[2 * ld + 1], R[2 * ld + 2]); ey = (float)atan2(-R[2 * ld], (double)sy); ez = (float)atan2(R[ld], R[0]);
    } else {
        ex = (float)atan2(-R[ld + 2], R[ld + 1]); ey = (float)atan2(-R[2 * ld], (double)sy); ez = 0.f;
    }
    return (double)fabsf(ey) < 0.1 && (double)fabsf(ex) < 0.1 && (double)fabsf(ez) < 0.1;
}
// |t|^2, components ld doubles apart (1: a vector, 4: the last column of a pose), summed left to right
__host__ __device__ inline double pose_norm2_t(const double *t, int ld) { return t[0] * t[0] + t[ld] * t[ld] + t[2 * ld] * t[2 * ld]; }

// THE cleared step record: counts 0, no motion (R = I, T_rel_inv = I), pose 0.  A failed pair's record, a stream's first
// frame and the online chain's first frame all start from it and fill in what they know.
__host__ __device__ inline void step_record_clear(svo_step_result &r)
{
    r.ok = 0; r.fail_stage = 0; r.n_prev_kps = 0; r.n_cur_kps = 0; r.n_tracked = 0; r.n_inliers = 0; r.ransac_iters = 0; r.lm_iters = 0;
    for (int i = 0; i < 3; i++) { r.rvec[i] = 0; r.tvec[i] = 0; }
    for (int i = 0; i < 9; i++) r.R[i] = (i % 4 == 0) ? 1.0 : 0.0;
    pose_identity16(r.T_rel_inv);
    for (int i = 0; i < 16; i++) r.pose[i] = 0;
}

template <int K>                                   // lane k of every quad of four lanes reads lane K's double
__device__ __forceinline__ double quad_bcast_f64(double v)
{
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), K * 0x55, 0xF, 0xF, true);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), K * 0x55, 0xF, 0xF, true);
    return __hiloint2double(hi, lo);
}
// The chain (chain): P <- P T_p for p = 0 .. cnt - 1 where ok_p, P written out after every step, by ONE WAVE.  Lane
// (i, j) = ((lane >> 2) & 3, lane & 3) carries P[i][j]; a row's four elements reach its lanes by quad DPP broadcast, and the
// cnt <= 64 pairs (T row-major, ok) wait in LDS -- one dependent global load per pair made the serial product cost a memory
// round trip per step.  pose_mul4_elem keeps the association order of a plain triple loop, so chunked and whole-sequence
// chaining agree bit for bit.  pose_at(p): where the 16 doubles of the pose after pair p go.  Returns the running P.
template <class PoseAt>
__device__ __forceinline__ double chain_wave_step(double P, const double *sT, const int *sOk, int cnt, PoseAt pose_at)
{
    const int lane = threadIdx.x & 63, j = lane & 3;
    for (int p = 0; p < cnt; p++) {
        const double p0 = quad_bcast_f64<0>(P), p1 = quad_bcast_f64<1>(P), p2 = quad_bcast_f64<2>(P), p3 = quad_bcast_f64<3>(P);
        if (sOk[p]) P = pose_mul4_elem(p0, p1, p2, p3, sT + p * 16 + j);
        if (lane < 16) pose_at(p)[lane] = P;
    }
    return P;
}
}  // namespace svo
