// lk_common.h -- everything the two pyramidal-LK kernels share, stated once.  lk.hip (exact integer sums, the canonical
// recipe) and lk_sse2.hip (upstream's x86 float accumulation orders) differ in three things only: the tile geometry (a
// traits type: ExactTile in lk.hip, ChainTile in lk_sse2.hip), the patch packing, and how the five sums A11, A12, A22,
// b1, b2 are formed.  Those stay in the two files, with the level / iteration skeleton of their lk_call4 that orders the
// LDS hand-offs.  Here:
//   * the packed dot-product helpers, cvFloor, the bilinear weights;
//   * tile staging: the lane's staging items, the source loads, the I- and J-tile stores as row-pair column words;
//   * the packed Scharr passes with the zero border of the derivative image, and the bilinear patch samples;
//   * every CONTROL RULE of cv::calcOpticalFlowPyrLK -- window position, weights and status per level, the I-tile
//     requests, the J-tile origin and the re-stage test, the minEig / D degeneracy test, the 2x2 solve with the
//     convergence and oscillation tests, the final-window check -- each with its exactness argument;
//   * the kernel driver: workgroup -> (batch item, wave of the item), the wave's chunks of four points, the chain of
//     ncalls calls, the deleteBadmatchFeatures predicate, the keep byte.
// See lk.hip for the mapping these serve.
#pragma once
#include "svo_device.h"
#include "svo_kernels.h"

namespace svo {

constexpr int kSlots = 4;                                 // points per wave
constexpr int W_BITS = 14;
constexpr float kHalfWin = 10.f;                          // (winSize - 1) * 0.5
constexpr float kFltScale = 1.f / (1 << 20);              // FLT_SCALE of the five sums
constexpr int kNoJTile = -(1 << 20);                      // tx0 of a slot without a staged J tile

// A tile geometry (the template parameter T below) names: kColDw (words per tile column), kCols (columns of a slot
// tile), kTileDw = kCols * kColDw (words per slot tile), kStoreCols (how many of the 28 staged columns a staging pass at
// a level's start stores: kCols, or more where the geometry lets the last source dword spill behind the tile),
// kQPairs / kJPairs (row pairs of the I / J tile), kJMargin (spare J rows, and columns on the left, around the window)
// and kAlignedI (the I tile starts at a 4-byte aligned image column).
constexpr int kStagedCols = 28;                           // 7 source dwords per row pair
// columns a window spans: lane segment 2 reads its eight column words from cx + 14
constexpr int kWindowCols = 2 * 7 + 8;
// largest cx = inx - tx0 at which the window's columns are all inside the tile: the x half of the re-stage test
template <class T> constexpr int j_span_x() { return T::kCols - kWindowCols; }

typedef short s16x2 __attribute__((ext_vector_type(2)));
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32_unaligned __attribute__((aligned(1)));
typedef const uint32_t __attribute__((address_space(3))) lds_cu32;

// cvFloor: one instruction (floor + convert; the compiler's __float2int_rd is v_floor_f32 + v_cvt_i32_f32,
// and on gfx950 conversions issue at half the rate of plain 32-bit adds -- profiles/r02_valu_roof.txt)
__device__ __forceinline__ int cv_floor(float v)
{
    int r;
    asm("v_cvt_flr_i32_f32 %0, %1" : "=v"(r) : "v"(v));
    return r;
}
__device__ __forceinline__ uint32_t perm_b32(uint32_t s0, uint32_t s1, uint32_t sel) { return __builtin_amdgcn_perm(s0, s1, sel); }
__device__ __forceinline__ int dot2(uint32_t a, uint32_t b, int c)
{
    return __builtin_amdgcn_sdot2(__builtin_bit_cast(s16x2, a), __builtin_bit_cast(s16x2, b), c, false);
}
// first link of a dot chain: the rounding constant comes from an SGPR through the VOP3P encoding
// (the VOP2 v_dot2c form accumulates in place and would need a v_mov of the constant every time)
__device__ __forceinline__ int dot2_k(uint32_t a, uint32_t b, int k)
{
    int r;
    asm("v_dot2_i32_i16 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "s"(k));
    return r;
}
// first link of a chain that starts from 0: the inline constant instead of a zeroed accumulator (v_mov + v_dot2c)
__device__ __forceinline__ int dot2_0(uint32_t a, uint32_t b)
{
    int r;
    asm("v_dot2_i32_i16 %0, %1, %2, 0" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ uint32_t as_u32(u16x2 v) { return __builtin_bit_cast(uint32_t, v); }
__device__ __forceinline__ u16x2 as_u16x2(uint32_t v) { return __builtin_bit_cast(u16x2, v); }

// exact (float)(hi * 65536 + lo) with round-to-nearest-even: |hi|, |lo| < 2^24 convert exactly
// and one fused multiply-add rounds the exact sum once (f64 conversions issue at a fraction of
// the f32 rate, and this runs every iteration)
__device__ __forceinline__ float wide_to_f32(int hi, int lo)
{
    return __builtin_fmaf((float)hi, 65536.f, (float)lo);
}
// The four bilinear weights as the two packed operands of the column-word dot products:
//   Wa = iw00 | iw10 << 16   (column tap k: window rows A | B),   Wb = iw01 | iw11 << 16   (tap k + 1)
// iw00 = cvRound((1-a)(1-b) 2^14) ...: the 2^14 scale is folded into the b factors first (scaling by a
// power of two is exact, so every product rounds exactly as upstream's expression does).  cvRound of
// 0 <= x <= 2^14 is taken with the 1.5 * 2^23 trick: x + 12582912.f rounds x to the nearest-even
// integer and leaves it in the low mantissa bits (two full-rate adds instead of v_rndne + v_cvt);
// the low 16 bits of the sum's bit pattern ARE the weight, so the packing is one v_perm.
struct PackedWeights { uint32_t Wa, Wb; };
__device__ __forceinline__ PackedWeights bilinear_weights(float a, float b)
{
    const float magic = 12582912.f;                            // 0x4B400000
    const float a1 = 1.f - a, b1 = (1.f - b) * (float)(1 << W_BITS), b0 = b * (float)(1 << W_BITS);
    const uint32_t u00 = __float_as_uint(a1 * b1 + magic), u01 = __float_as_uint(a * b1 + magic),
                   u10 = __float_as_uint(a1 * b0 + magic);     // 0x4B400000 + iw
    const uint32_t w11 = (uint32_t)(1 << W_BITS) + 3u * 0x4B400000u - u00 - u01 - u10;
    PackedWeights w;
    w.Wa = perm_b32(u10, u00, 0x05040100u);
    w.Wb = perm_b32(w11, u01, 0x05040100u);
    return w;
}

// ---- flags as lane masks ------------------------------------------------------------------------------------------
// Every per-slot flag of the control path (live, the level / iteration flags, re-stage, converged, status) is a
// wave-uniform 64-bit LANE MASK in an SGPR pair: bit l = the flag of lane l, i.e. of slot l >> 4.  A mask comes straight
// out of a vector compare (the builtins below write the compare's SGPR-pair result; no lane is ever masked off in the
// callers, so a bit is the predicate of its lane and ~m is its negation), masks combine on the scalar unit (&, |, &~), a
// ballot is the mask itself, an any-test is m != 0, and a mask is applied with ONE v_cndmask_b32 whose condition operand is
// the SGPR pair.  A flag kept as a bool is a divergent i1: every ballot of it came out as v_cndmask_b32 v, 0, 1, s[..] +
// v_cmp_ne_u32 (the compiler re-masks it with exec), and every "if (flag)" as an s_and_saveexec diamond.
// The predicates are the ones of the bool form: "a < b" on floats is the ORDERED compare (false for a NaN), and a
// negated flag is the mask's complement, which is true for a NaN exactly where "!(a < b)" is.
typedef unsigned long long lanemask;
enum { kIcmpUgt = 34, kIcmpUge = 35 };                                // llvm::CmpInst predicates of the compare builtins
enum { kFcmpOgt = 2, kFcmpOlt = 4, kFcmpOle = 5 };
__device__ __forceinline__ lanemask mask_ugt(unsigned a, unsigned b) { return __builtin_amdgcn_uicmp(a, b, kIcmpUgt); }
__device__ __forceinline__ lanemask mask_uge(unsigned a, unsigned b) { return __builtin_amdgcn_uicmp(a, b, kIcmpUge); }
// float compares: __builtin_amdgcn_fcmpf (the builtin without the f is the DOUBLE compare and converts its operands)
__device__ __forceinline__ lanemask mask_lt(float a, float b) { return __builtin_amdgcn_fcmpf(a, b, kFcmpOlt); }
__device__ __forceinline__ lanemask mask_le(float a, float b) { return __builtin_amdgcn_fcmpf(a, b, kFcmpOle); }
__device__ __forceinline__ lanemask mask_le(double a, double b) { return __builtin_amdgcn_fcmp(a, b, kFcmpOle); }
__device__ __forceinline__ lanemask mask_gt(double a, double b) { return __builtin_amdgcn_fcmp(a, b, kFcmpOgt); }
// m ? a : b per lane: v_cndmask_b32 d, b, a, s[m]
__device__ __forceinline__ bool lane_of(lanemask m) { return __builtin_amdgcn_inverse_ballot_w64(m); }
__device__ __forceinline__ int select(int a, int b, lanemask m) { return lane_of(m) ? a : b; }
__device__ __forceinline__ float select(float a, float b, lanemask m) { return lane_of(m) ? a : b; }
// slot s's bit of a mask (its control lanes all carry the same flag)
__device__ __forceinline__ bool slot_bit(lanemask m, int s) { return (m >> (16 * s)) & 1ull; }

// 1 / (1 << level) of a pyramid level (wave-uniform): 2^-level is a normal float, so its bit pattern is the biased exponent
// 127 - level alone -- one scalar shift for the IEEE division sequence (convert, two v_div_scale, v_rcp, five fma / mul,
// v_div_fmas, v_div_fixup) that the quotient costs.  The value is the quotient's, exactly: every product with it rounds as before.
__device__ __forceinline__ float level_scale(int level) { return __uint_as_float((uint32_t)(127 - level) << 23); }

// "ix < -win || ix >= w || iy < -win || iy >= h" with two unsigned compares
__device__ __forceinline__ lanemask window_oob(int ix, int iy, int w, int h)
{
    return mask_uge((unsigned)(ix + kWin), (unsigned)(w + kWin)) | mask_uge((unsigned)(iy + kWin), (unsigned)(h + kWin));
}

// ---- one iteration's pixel work for one slot --------------------------------------------------
// Column words C_j = (J[r0][j] | J[r1][j] << 16) pair the two window rows, so a bilinear sample is
//   val_k = dot2(C_k, (w00 | w10 << 16)) + dot2(C_k+1, (w01 | w11 << 16)) + 2^8
// (signed 16-bit weights: w11 == -1 needs no special case).
__device__ __forceinline__ int dot2_v(uint32_t a, uint32_t b, int c)      // a . b + c, c in a VGPR that stays live
{
    int r;
    asm("v_dot2_i32_i16 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
__device__ __forceinline__ int dot2_sv(uint32_t a, uint32_t b_uniform, int c)   // b wave-uniform (SGPR), c in a VGPR
{
    int r;
    asm("v_dot2_i32_i16 %0, %1, %2, %3" : "=v"(r) : "v"(a), "s"(b_uniform), "v"(c));
    return r;
}
// the rounding of the J samples, 2^8 scaled like the column words (pixel << 7), held in a VGPR: a VOP3P instruction can
// read ONE scalar operand, and that one is the slot's weight (an SGPR from v_readlane); a scalar rounding constant cost
// a v_mov per slot and iteration
__device__ __forceinline__ int j_sample_rounding()
{
    int vround = 1 << (W_BITS - 5 - 1 + 7);
    asm volatile("" : "+v"(vround));
    return vround;
}

// ---- tile staging -------------------------------------------------------------------------------
// A tile is staged from 7 source dwords (28 columns) per row pair: staging item lane + 64 t = row pair * 7 + dword
// column.  dst: the item's first column word in a column-major tile with CS words per column.
struct StageLane { int pr[3], dc4[3], dst[3]; };
template <int CS>
__device__ __forceinline__ StageLane stage_lane(int lane)
{
    StageLane q;
#pragma unroll
    for (int t = 0; t < 3; t++) {
        const int i = lane + 64 * t;
        q.pr[t] = i / 7; q.dc4[t] = 4 * (i - q.pr[t] * 7); q.dst[t] = q.dc4[t] * CS + q.pr[t];
    }
    return q;
}
// lane part of the items' source offsets at a level: one 24-bit multiply-add each (the 32-bit product came out as
// v_mad_u64_u32).  Exact: pr <= 27 (26 among the items in use) and the pitch of every accepted frame size is far below 2^24 (svo_create refuses
// widths above 16384; kMaxLkPitch in svo_device.h, asserted where the geometry is built), so neither operand loses a bit.
__device__ __forceinline__ void stage_src(uint32_t (&src)[3], const StageLane &q, int pitch)
{
#pragma unroll
    for (int t = 0; t < 3; t++) src[t] = __umul24((unsigned)q.pr[t], (unsigned)pitch) + (uint32_t)q.dc4[t];
}
// A tile's source dwords for this lane: rows `rowA` (upper) and `rowB` = rowA + pitch of every item, at 32-bit
// offsets from the slot's wave-uniform base (global_load with an SGPR base: scalar part per slot, lane part per level)
__device__ __forceinline__ void tile_loads(uint32_t (&r)[3][2], const uint8_t *rowA, const uint8_t *rowB, uint32_t s_off,
                                           const uint32_t (&q_src)[3], int lane, int n_items)
{
#pragma unroll
    for (int t = 0; t < 3; t++) {
        if (lane + 64 * t < n_items) {
            const uint32_t o = s_off + q_src[t];
            r[t][0] = *(const u32_unaligned *)(rowA + o); r[t][1] = *(const u32_unaligned *)(rowB + o);
        }
    }
}
// the tile of PAIRS row pairs whose first pixel is (x, y) of the level; x, y from slot s's control lane
template <int PAIRS>
__device__ __forceinline__ void tile_request(uint32_t (&r)[3][2], const PyrGeom &g, int level, int pitch, const uint8_t *slot,
                                             int x, int y, int s, const uint32_t (&q_src)[3], int lane)
{
    const int xs = __builtin_amdgcn_readlane(x, 16 * s), ys = __builtin_amdgcn_readlane(y, 16 * s);
    tile_loads(r, slot, slot + pitch, (uint32_t)(g.origin[level] + ys * pitch + xs), q_src, lane, PAIRS * 7);
}
// ... and their four column words each (pixel[r][c] | pixel[r + 1][c] << 16) into a column-major I tile
template <class T>
__device__ __forceinline__ void tile_store_i(uint32_t *tile, const uint32_t (&r)[3][2], const StageLane &q, int lane)
{
#pragma unroll
    for (int t = 0; t < 3; t++) {
        if (lane + 64 * t < T::kQPairs * 7) {
            const uint32_t top = r[t][0], bot = r[t][1];
            uint32_t *d = tile + q.dst[t];
#pragma unroll
            for (int c = 0; c < 4; c++) {
                // a column past the tile would land in the next slot's first column, or behind the wave's LDS region
                if (24 + c >= T::kStoreCols && q.dc4[t] == 24) continue;
                d[c * T::kColDw] = perm_b32(bot, top, 0x0c040c00u + 0x00010001u * c);
            }
        }
    }
}
// ... into a J tile.  The columns from kStoreCols on are left out; MASKED (a re-stage of one slot beside live
// neighbours): the columns from kCols on.
template <class T, bool MASKED>
__device__ __forceinline__ void tile_store_j(uint32_t *tile, const uint32_t (&r)[3][2], const StageLane &q, int lane)
{
#pragma unroll
    for (int t = 0; t < 3; t++) {
        if (lane + 64 * t < T::kJPairs * 7) {
            const uint32_t top = r[t][0], bot = r[t][1];
            uint32_t *d = tile + q.dst[t];
            // samples are stored as pixel << 7 (byte into the high byte of its half, one packed shift): the
            // bilinear sums then come out scaled by 2^7 and "sum >> 9" is simply their high half
            const u16x2 one = {1, 1};
#pragma unroll
            for (int c = 0; c < 4; c++) {
                if (24 + c >= (MASKED ? T::kCols : T::kStoreCols) && q.dc4[t] == 24) continue;
                d[c * T::kColDw] = as_u32(as_u16x2(perm_b32(bot, top, 0x040c000cu + 0x01000100u * c)) >> one);
            }
        }
    }
}

// ---- the patch: packed Scharr derivatives and bilinear samples -----------------------------------------------------
// A lane's NC tile columns from `q0` (its first column, row pair `row`) as COLUMN WORDS pairing two vertically adjacent
// rows (low half = upper row): Q01/Q12/Q23[j] = tile rows (row, row+1)/(row+1, row+2)/(row+2, row+3) of column j.  The
// packed Scharr passes produce the derivative rows A (image row gyA) and B (gyA + 1) side by side in one register per
// column, which is exactly the operand the bilinear v_dot2 wants:
//   val_k = dot2(D[k], (w00 | w10 << 16)) + dot2(D[k+1], (w01 | w11 << 16)) + rounding
// so no lane ever realigns a pixel pair.  Derivative column c = 0..NC-3 (image column gx0 + c) comes from tile columns
// c..c+2; Q12[c + 1] is the pixel pair under it.
template <int NC, int CS, bool EDGE>
__device__ __forceinline__ void scharr_columns(lds_cu32 *q0, int gx0, int gyA, int w, int h, uint32_t (&Q12)[NC],
                                               uint32_t (&DX)[NC - 2], uint32_t (&DY)[NC - 2])
{
    uint32_t Q01[NC], Q23[NC];
    // ONE address per slot: everything else is an immediate offset of the reads
#pragma unroll
    for (int j = 0; j < NC; j++) { Q01[j] = q0[j * CS]; Q12[j] = q0[j * CS + 1]; Q23[j] = q0[j * CS + 2]; }
    // vertical Scharr passes, rows A | B packed.  Both passes carry a factor 4 (coefficients 12 / 40
    // instead of 3 / 10; |4 d| <= 16320 still fits 16 bits): the interpolated derivative
    // (sum + 2^13) >> 14 then equals (4 sum + 2^15) >> 16, i.e. the HIGH half of the accumulator, and
    // the patch packing picks bytes 2-3 directly instead of shifting every value first.
    uint32_t T0[NC], T1[NC];
    const u16x2 k12 = {12, 12}, k40 = {40, 40};
#pragma unroll
    for (int j = 0; j < NC; j++) {
        T0[j] = as_u32((as_u16x2(Q01[j]) + as_u16x2(Q23[j])) * k12 + as_u16x2(Q12[j]) * k40);       // 4 t0
        T1[j] = as_u32(as_u16x2(Q23[j]) - as_u16x2(Q01[j]));                                          // t1
    }
    // horizontal passes
#pragma unroll
    for (int c = 0; c < NC - 2; c++) {
        DX[c] = as_u32(as_u16x2(T0[c + 2]) - as_u16x2(T0[c]));                                        // 4 dx
        DY[c] = as_u32((as_u16x2(T1[c]) + as_u16x2(T1[c + 2])) * k12 + as_u16x2(T1[c + 1]) * k40);    // 4 dy
    }
    // the derivative image's border is BORDER_CONSTANT 0: mask positions outside the image
    // (only possible when the window hangs over the edge: the EDGE instantiation)
    if (EDGE) {
        const int gyB = gyA + 1;
        const uint32_t rows = ((gyA >= 0 && gyA < h) ? 0x0000FFFFu : 0u) | ((gyB >= 0 && gyB < h) ? 0xFFFF0000u : 0u);
#pragma unroll
        for (int c = 0; c < NC - 2; c++) {
            const int gx = gx0 + c;
            const uint32_t mk = (gx >= 0 && gx < w) ? rows : 0u;
            DX[c] &= mk; DY[c] &= mk;
        }
    }
}
// the lane's NP = NC - 3 patch pixels: I with 5 fractional bits; Ix, Iy as value << 16 | rounding residue
template <int NC>
__device__ __forceinline__ void patch_samples(const uint32_t (&Q12)[NC], const uint32_t (&DX)[NC - 2], const uint32_t (&DY)[NC - 2],
                                              uint32_t Wa, uint32_t Wb, int (&iv)[8], int (&ix)[8], int (&iy)[8])
{
#pragma unroll
    for (int k = 0; k < NC - 3; k++) {
        iv[k] = dot2(Q12[k + 2], Wb, dot2_k(Q12[k + 1], Wa, 1 << (W_BITS - 5 - 1))) >> (W_BITS - 5);
        ix[k] = dot2(DX[k + 1], Wb, dot2_k(DX[k], Wa, 1 << (W_BITS + 1)));
        iy[k] = dot2(DY[k + 1], Wb, dot2_k(DY[k], Wa, 1 << (W_BITS + 1)));
    }
}

// ---- the control rules of one cv::calcOpticalFlowPyrLK call ---------------------------------------------------------
// Control values are per lane = per slot lane >> 4: one vector instruction advances all four points.

// first image column of the I tile: the patch needs the columns from ipx - 1
template <class T> __device__ __forceinline__ int i_tile_x0(int ipx) { return T::kAlignedI ? (ipx - 1) & ~3 : ipx - 1; }

// The I tiles of a level depend on prevPt only: they are requested one level ahead (the top level's before the level
// loop), so their latency is covered by the previous level's iterations.  `src`: the lane part of the level's tile source
// offsets (stage_src), which the pass over that level uses again for its J tiles instead of forming it a second time.
template <class T>
__device__ __forceinline__ void request_I(uint32_t (&rI)[kSlots][3][2], uint32_t (&src)[3], const PyrGeom &g, int level,
                                          const uint8_t *slotI, float2 prevPt, lanemask live, const StageLane &q, int lane)
{
    const float lscale = level_scale(level);
    const int ipx = cv_floor(prevPt.x * lscale - kHalfWin), ipy = cv_floor(prevPt.y * lscale - kHalfWin);
    const int pitch = g.pitch[level];
    const lanemask m = live & ~window_oob(ipx, ipy, g.w[level], g.h[level]);
    const int x0 = i_tile_x0<T>(ipx), y0 = ipy - 1;
    stage_src(src, q, pitch);
#pragma unroll
    for (int s = 0; s < kSlots; s++) {
        if (!slot_bit(m, s)) continue;
        tile_request<T::kQPairs>(rI[s], g, level, pitch, slotI, x0, y0, s, src, lane);
    }
}

// A level's start: nextPt scaled up, the I window position and weights, the status rule for a window outside the
// level, and the J window of the first iteration (nextPt is known, so its tile is requested together with the I tiles
// and the patch arithmetic covers the latency of both).
struct LkLevel {
    int w, h;
    int ipx, ipy;               // I window corner
    uint32_t WIa, WIb;          // I weights
    lanemask on;                // the slot iterates at this level
    float qx, qy;               // nextPt - halfWin
    int tx0, ty0;               // J tile origin; tx0 == kNoJTile: none staged
    lanemask j_staged;          // the slot has a J tile at the level's start (tx0 != kNoJTile)
};
// (status: the mask of the slots whose status byte is still 1)
template <class T>
__device__ __forceinline__ LkLevel level_begin(const PyrGeom &g, int level, float2 prevPt, lanemask live, float &nx, float &ny,
                                               lanemask &status)
{
    LkLevel v;
    v.w = g.w[level]; v.h = g.h[level];
    const float lscale = level_scale(level);
    float px = prevPt.x * lscale, py = prevPt.y * lscale;
    if (level == g.nlevels - 1) { nx = px; ny = py; }
    else { nx = nx * 2.f; ny = ny * 2.f; }
    px -= kHalfWin; py -= kHalfWin;
    v.ipx = cv_floor(px); v.ipy = cv_floor(py);
    const lanemask oob = window_oob(v.ipx, v.ipy, v.w, v.h);
    if (level == 0) status &= ~(live & oob);
    v.on = live & ~oob;
    const PackedWeights wt = bilinear_weights(px - (float)v.ipx, py - (float)v.ipy);
    v.WIa = wt.Wa; v.WIb = wt.Wb;
    v.qx = nx - kHalfWin; v.qy = ny - kHalfWin;
    const int inx = cv_floor(v.qx), iny = cv_floor(v.qy);
    v.j_staged = v.on & ~window_oob(inx, iny, v.w, v.h);
    v.tx0 = select(inx - T::kJMargin, kNoJTile, v.j_staged); v.ty0 = select(iny - T::kJMargin, 0, v.j_staged);
    return v;
}

// The minEig test without its division.  Upstream tests minEig = num / (2 * win * win) < 0.001f with num = A22 + A11 - sqrt(..); the
// kernel returns no err, so the quotient is used in that comparison alone.  Correctly rounded division by the positive constant
// 882.f is monotone (non-decreasing) in num, so the floats whose quotient lies below 0.001f are exactly those below one float T:
//   fl(num / 882.f) < 0.001f  <=>  num < kMinEigNumBelow,
// with both sides false for a NaN and for +inf and true for every negative num.  T is the smallest float whose rounded quotient
// reaches 0.001f = 0x3A83126F: 0x3F61CAC1 = 0x1.c39582p-1 (its predecessor's quotient rounds to 0x3A83126E), found by bisection over
// the float32 bit patterns and checked around T and over random floats by tests/test_host_lk_mineig_threshold.py.
constexpr float kMinEigNumBelow = 0x1.c39582p-1f;

// The 2x2 system of a level: a slot whose minimum eigenvalue or determinant is too small stops here (status 0 at
// level 0).  Dinv = 1 / D; returns the slots that go on.  The sums of a slot that is not lvl_on are whatever its row
// of the reduction held (lk.hip, "dead slots"): its D, minEig and Dinv are computed and never used -- `degenerate` acts
// on status and on the returned mask only through "lvl_on &".
__device__ __forceinline__ lanemask level_solve_setup(float A11, float A12, float A22, int level, lanemask lvl_on, lanemask &status,
                                                      float &Dinv)
{
    const float D = A11 * A22 - A12 * A12;
    const float minEigNum = A22 + A11 - sqrtf((A11 - A22) * (A11 - A22) + 4.f * A12 * A12);      // minEig * (2 * kWin * kWin)
    static_assert(2 * kWin * kWin == 882, "kMinEigNumBelow is derived for the divisor 882");
    const lanemask degenerate = mask_lt(minEigNum, kMinEigNumBelow) | mask_lt(D, 1.1920929e-07f);
    if (level == 0) status &= ~(lvl_on & degenerate);
    Dinv = 1.f / D;
    return lvl_on & ~degenerate;
}

// An iteration's start: the J window position and weights, the status rule for a window that left the level, and the
// re-stage test: the tile holds kJMargin spare rows above and below and kJMargin spare columns left of the window it
// was staged for, and j_span_x - kJMargin columns right of it (one fewer than on the left in a 27-column tile); a
// window that drifted further gets a new tile around itself.
// A slot that does not iterate computes all of this from a stale window position (iter_update); nothing of it is used:
// status and restage carry "it_on &", the tile origin moves under restage only, and the weights and joff of a slot are
// read by the pixel work of that slot alone, which runs under the slot's bit of `on`.
struct LkIter {
    lanemask on;                // the slot still iterates
    uint32_t Wa, Wb;            // J weights
    int joff;                   // slot part of the J sample offset (bytes), tile position of the slot included
    lanemask restage;
};
template <class T>
__device__ __forceinline__ LkIter iter_begin(float qx, float qy, int w, int h, int level, int lane, lanemask it_on, lanemask &status,
                                             int &tx0, int &ty0)
{
    LkIter it;
    const int inx = cv_floor(qx), iny = cv_floor(qy);
    const lanemask oob = window_oob(inx, iny, w, h);
    if (level == 0) status &= ~(it_on & oob);
    it_on &= ~oob;
    const PackedWeights wj = bilinear_weights(qx - (float)inx, qy - (float)iny);
    it.Wa = wj.Wa; it.Wb = wj.Wb;
    it.restage = it_on & (mask_ugt((unsigned)(inx - tx0), (unsigned)j_span_x<T>()) |
                          mask_ugt((unsigned)(iny - ty0), (unsigned)(2 * T::kJMargin)));
    // a re-staged tile starts kJMargin before the window: cx = cy = kJMargin then fall out of the new origin
    tx0 = select(inx - T::kJMargin, tx0, it.restage); ty0 = select(iny - T::kJMargin, ty0, it.restage);
    const int cx = inx - tx0, cy = iny - ty0;
    it.joff = ((int)__umul24((unsigned)cx, T::kColDw) + cy + (lane >> 4) * T::kTileDw) * 4;
    it.on = it_on;
    return it;
}

// An iteration's end: the 2x2 solve, the step, the convergence and oscillation tests (a slot drops out when it
// converges or oscillates); returns the slots that go on.
// nextPt (nx, ny) moves under the slot's flag.  The window position qx, qy and prevDelta are working values of the
// iterations: they take the step in every lane, and a slot that has stopped (or whose b sums are what a dead row of the
// reduction held, lk.hip "dead slots") only ever feeds them to iter_begin and to the tests below, where every use
// carries "it_on &"; the next level recomputes qx, qy from nextPt and resets prevDelta.
__device__ __forceinline__ lanemask iter_update(float A11, float A12, float A22, float Dinv, float b1f, float b2f, int j, lanemask it_on,
                                                float &qx, float &qy, float &nx, float &ny, float &pdx, float &pdy)
{
    const float dlx = (A12 * b2f - A22 * b1f) * Dinv;
    const float dly = (A12 * b1f - A11 * b2f) * Dinv;
    // "delta.ddot(delta) <= epsilon" is a double comparison upstream; float decides it unless
    // the sum lands within 1e-4 relative of epsilon (float error here < 2e-7 relative)
    const float dd = dlx * dlx + dly * dly;
    lanemask conv = mask_le(dd, 0.9999e-4f);
    if (__builtin_expect((it_on & ~conv & mask_lt(dd, 1.0001e-4f)) != 0, 0)) {
        asm volatile("" ::: "memory");               // a real branch: if-converted, the f64 path ran every iteration
        conv = mask_le((double)dlx * (double)dlx + (double)dly * (double)dly, 0.01 * 0.01);
    }
    qx += dlx; qy += dly;
    // "std::abs(delta.x + prevDelta.x) < 0.01" compares a float with the double 0.01; the
    // largest float below 0.01 is 0.01f itself, so "<= 0.01f" in float is the same predicate
    const lanemask osc = j > 0 ? it_on & ~conv & mask_le(fabsf(dlx + pdx), 0.01f) & mask_le(fabsf(dly + pdy), 0.01f) : 0ull;
    const float sx = qx + kHalfWin, sy = qy + kHalfWin;
    nx = select(select(sx - dlx * 0.5f, sx, osc), nx, it_on);
    ny = select(select(sy - dly * 0.5f, sy, osc), ny, it_on);
    pdx = dlx; pdy = dly;
    return it_on & ~conv & ~osc;
}

// err is requested by the reference: the final window must still be inside (A.4 step 7)
// (a slot that is not live, or whose status is 0 already, is not changed by clearing its bit again)
__device__ __forceinline__ void final_window_check(float nx, float ny, int w, int h, int level, lanemask live, lanemask &status)
{
    if (level == 0) {
        const int fx = cv_floor(nx - kHalfWin), fy = cv_floor(ny - kHalfWin);
        status &= ~(live & window_oob(fx, fy, w, h));
    }
}

// ---- the kernel driver ---------------------------------------------------------------------------------------------
// Grid: ONE dimension, a.gx workgroups of W waves per batch item.  XCD-aware mapping: consecutive workgroup ids go
// round-robin to the 8 XCDs, each with its own 4 MB L2, so item = (id / 8 / gx) * 8 + id % 8 keeps
// every XCD on its own items -- an XCD then has about one item's four pyramids (3.3 MB) in flight
// instead of slices of all items that are in flight anywhere on the chip (L2 hit rate 63 % -> see
// DESIGN.md).  Items in whole groups of 8 are dealt one per XCD; the last (batch % 8) items -- the single pair of
// the online path among them -- are spread over all XCDs in the plain order.
struct LkItem { int b, bx; };                           // batch item, workgroup of the item
__device__ __forceinline__ LkItem lk_item_of_workgroup(const LkArgs &a)
{
    const int n_aware = (a.batch & ~7) * a.gx;
    LkItem it;
    if ((int)blockIdx.x < n_aware) {
        const int xcd = blockIdx.x & 7, slot_id = blockIdx.x >> 3;
        it.b = (slot_id / a.gx) * 8 + xcd; it.bx = slot_id % a.gx;
    } else {
        const int r = blockIdx.x - n_aware;
        it.b = (a.batch & ~7) + r / a.gx; it.bx = r % a.gx;
    }
    return it;
}

// The waves of an item walk its points in strides of a.gx * W * 4 (waves x four slots), so the launch is sized from
// the batch, not from the keypoint CAPACITY (cv::FAST is uncapped and the capacity is generous: a grid of capacity / 16
// workgroups of four per item was mostly empty waves).  No workgroup barrier anywhere: each wave loops on its own.
// With ncalls == 4 the wave walks the whole circular chain L1 -> R1 -> R2 -> L2 -> L1' for its four points and stops
// early once all of them are rejected.
// lk_call(slotI, slotJ, prevPt, outPt, status, live): one cv::calcOpticalFlowPyrLK call for the wave's four points.
template <int W, class Call>
__device__ __forceinline__ void lk_track_item(const LkArgs &a, int wave, int lane, Call &&lk_call)
{
    const LkItem item = lk_item_of_workgroup(a);
    const int b = item.b, slot = lane >> 4;
    int n = a.n_pts ? a.n_pts[b] : a.n_fixed;
    n = min(n, a.cap);
    // slots per wave: four when the launch fills the chip (the control work of an iteration is shared by
    // four points); a launch of a few items only (the online path: one pair) is latency-bound -- there the
    // points are spread over as many waves as the grid has, down to one point per wave
    int spw = kSlots;
    if (a.spread) spw = min(kSlots, max(1, (n + a.gx * W - 1) / (a.gx * W)));
    for (int first = (item.bx * W + wave) * spw; first < n; first += a.gx * W * spw) {
        const int idx = first + slot;
        const bool valid = slot < spw && idx < n;
        const bool writer = valid && lane == 16 * slot;         // one lane per slot stores results
        const int64_t po = (int64_t)b * a.pts_stride + (valid ? idx : first);
        const float2 p0 = a.pts_in[po];
        float2 cur = p0, nxt;
        // the flags of the chain as lane masks (see "flags as lane masks" above)
        lanemask outside = mask_lt(p0.x, 0.f) | mask_lt(p0.y, 0.f), bad = 0, noepi = 0;
        lanemask live = __ballot(valid);
        float prev_y = p0.y;
#pragma nounroll
        for (int c = 0; c < a.ncalls; c++) {
            const uint8_t *sI = a.prev[c] + (int64_t)b * a.slot_stride;
            const uint8_t *sJ = a.next[c] + (int64_t)b * a.slot_stride;
            lanemask st;                                        // the slots with status 1
            lk_call(sI, sJ, cur, nxt, st, live);
            if (writer && lane_of(live)) {
                a.pts_out[c][po] = nxt;
                a.status[c][po] = (uint8_t)select(1, 0, st);
            }
            // Tracking::deleteBadmatchFeatures terms (p0 = t1_left, p1 = t1_right, p2 = t2_right,
            // p3 = t2_left, p0_return = LK#4 output; call-site mapping src/tracking.cpp:619-620,
            // predicate :623-660)
            outside |= live & (mask_lt(nxt.x, 0.f) | mask_lt(nxt.y, 0.f));
            bad |= live & ~st;
            if (c == 0 || c == 2) noepi |= live & mask_gt((double)fabsf(prev_y - nxt.y), a.match_err);   // |y0-y1|, |y2-y3|
            prev_y = select(nxt.y, prev_y, live);
            cur.x = select(nxt.x, cur.x, live); cur.y = select(nxt.y, cur.y, live);
            // a rejected point can never be kept: the remaining calls of the circular chain only feed
            // the keep predicate (their pts_out/status entries are scratch in the fused mode)
            if (a.ncalls == 4) live &= ~(outside | bad | noepi);
            if (!live) break;
        }
        if (a.ncalls == 4 && writer) a.keep[po] = !lane_of(outside | bad | noepi);
        wave_lds_fence();                                      // the next chunk restages this wave's tiles
    }
}

}  // namespace svo
