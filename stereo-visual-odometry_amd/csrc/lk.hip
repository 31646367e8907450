// lk.hip -- pyramidal iterative Lucas-Kanade tracking for gfx950: the body of
// cv::calcOpticalFlowPyrLK(prev, next, pts, out, status, err, Size(21,21), 3,
//                          TermCriteria(COUNT+EPS, 30, 0.01), 0, 0.001)
// as called four times per frame by Tracking::LK_Robust_Find_MuliImage_MatchedFeatures
// (reference src/tracking.cpp:583-622), plus the deleteBadmatchFeatures predicate (:623-660).
//
// Mapping: ONE WAVEFRONT TRACKS FOUR POINTS ("slots"), ONE WAVE PER WORKGROUP (kLkWavesPerWg; four in
// the latency shape), no barrier.  The kernel is VALU-issue bound (tiles come from L2), and more than half of a
// one-point-per-wave iteration is per-point SCALAR work (window position, bilinear weights, 2x2
// solve, convergence tests) that a wave executes as full vector instructions.  Here that scalar work
// is done once for four points: lane l carries the control state of slot l >> 4 (its row of 16
// lanes), so one vector instruction advances all four points, while the pixel work is done slot
// after slot by all 63 pixel lanes:
//   * lane l owns window row l/3, columns (l%3)*7..+6 of EVERY slot (63 lanes x 7 px = 441 px);
//   * tiles live in LDS as ROW-PAIR COLUMN WORDS (pixel[r][c] | pixel[r+1][c] << 16), formed once while
//     staging (4 v_perm per source dword pair): exactly the operand of the bilinear v_dot2_i32_i16, so
//     neither the patch build nor an iteration spends an instruction on byte alignment or unpacking;
//   * per level, per slot: the 24x27 I tile (requested one level ahead); the lane reads its 3 row pairs x
//     10 columns, forms the Scharr derivatives of the 2x8 positions it interpolates from ON THE FLY with
//     packed 16-bit math (the reference path materialises a full int16x2 derivative image per level
//     per call), interpolates I, Ix, Iy with v_dot2_i32_i16 and keeps the patch as 12 packed VGPRs;
//   * per iteration, per active slot: eight conflict-free dword reads from a column-major 27x27 J tile
//     (re-staged only when the window drifts out of it; requested beside the patch arithmetic), a
//     four-tap bilinear sample is two v_dot2_i32_i16 (signed 16-bit weight pairs; the words hold
//     pixel << 7, so the sample is the high half of its sum), then v_dot2 mismatch sums;
//   * the 16 partial sums of an iteration (4 slots x {b1,b2} x {low,high half}) are reduced with ONE
//     reduce-scatter over the rows (v_permlane32/16_swap + add, then DPP inside the row) that leaves
//     slot s's four sums in every quad of row s, exactly where that slot's control lanes need them;
//     the twelve A sums of a level (4 slots x {A11, A12, A22}) go the same way in one twelve-value reduce-scatter
//     (reduce_scatter12_rows, svo_device.h);
//   * the flags of the control path (live, iterating at the level / in the loop, re-stage, converged, status) are
//     wave-uniform LANE MASKS in SGPR pairs (lk_common.h): vector compares write them, the scalar unit combines them,
//     a ballot is the mask itself and one v_cndmask_b32 applies it; a slot that sits an iteration out leaves its
//     partial sums undefined instead of zero-filling them ("dead slots" below).  A wave-iteration with all four
//     slots at work is 207 vector instructions: 87 of control, reduction and solve + 30 per slot (3 v_readlane, 1 address
//     add, 14 + 8 v_dot2, 3 v_perm, 1 shift) -- 221 = 101 + 4 x 30 with bool flags and zero fills; the loop body has
//     no branch besides the per-slot skips, the re-stage test and the near-epsilon f64 test.
// The column-word J tiles cost 4x the LDS of byte tiles: 12 528 B per wave, ten of the 1280-byte granules LDS is handed
// out in, so twelve waves fit into a CU's 160 KB: three waves per SIMD, 168 VGPRs.
// A wave's life varies 2x with the iteration counts of its points, so a throughput launch's workgroup is
// ONE wave: it gives its LDS back the moment it ends and the dispatcher starts the next one (four-wave
// workgroups hold 50 KB until their slowest wave has ended).
//
// Exactness: all pixel arithmetic is upstream's fixed point (14-bit weights, 5 fractional bits);
// the five sums A11,A12,A22,b1,b2 are accumulated as exact integers (per-lane int32 partials,
// 16-bit halves reduced separately, recombined with one fused multiply-add) and converted to float
// once -- the canonical recipe of oracle/lk.c, so status bytes and point coordinates are
// bit-identical to the oracle.  FP contraction is off.
//
// Algorithmic HBM bytes (SURVEY.md 8d gather convention): per point per call
//   sum over 4 levels (24*24 + 22*22) + 8 in + 8 out + 1 status = 4257 B.
//
// What lives where: this file holds the tile geometry (ExactTile), the 7-pixel patch packing with the exact A partial
// sums (patch_slot), the mismatch sums (mismatch_slot), the level / iteration skeleton of lk_call4 with its LDS
// hand-offs and stamp points, lk_kernel's LDS declaration and the launchers.  The control rules of the algorithm, the
// tile staging, the Scharr passes and the kernel driver (item mapping, chunk loop, chain of calls, keep predicate) are
// lk_common.h's, shared with lk_sse2.hip.
#include <cstring>
#include "lk_common.h"

namespace svo {

// I tile: 24 rows x 27 bytes of the level, staged as ROW-PAIR COLUMN WORDS: Q[p][c] = byte c of tile
// row p | byte c of row p + 1 << 16 (23 pairs x 27 columns, one dword each).  The patch build wants
// exactly these words for the row pairs (r, r+1), (r+1, r+2), (r+2, r+3) of every lane's 10 columns;
// formed while staging (4 v_perm per staged dword pair, 12 per lane) they replace the 30 v_perm +
// 12 v_alignbyte every lane spent on its own copy, and the lane's reads become plain dword reads.
// The tile starts at the 4-byte aligned column at or left of ipx - 1 (offI <= 3 columns of slack): the last column a
// lane reads is 3 + 7 * 2 + 9 = 26.  The seven source dwords of a row pair carry 28 columns; the last one is not stored
// (in a 27-column tile it would be the next slot's column 0 and, behind slot 3, the word after the wave's LDS region).
// J tile: the same row-pair column words, 27 pairs x 27 columns around the window: 3 spare rows above and below, 3 spare
// columns on the left and 2 on the right (a window drifts that far at one level only rarely, and then the tile is
// staged again around it; a re-stage changes no result).  The 28th column would make a wave's tiles 12 992 B, eleven
// granules: eleven waves per CU instead of twelve.
// Both are stored COLUMN-MAJOR with 29 words per column: lane (row, seg) reads column cx + 7 seg + k, pair cy + row
// (I: its row pairs row, row+1, row+2 of column offI + 7 seg + j), so the banks of a 32-lane half are
// 7 * 29 * seg + row = 11 seg + row (mod 32) -- conflict-free; the row-major order is 2-way conflicted for every
// stride below 53 (half of all LDS-array cycles of the patch build; SQ_LDS_BANK_CONFLICT was 30 % of
// SQ_LDS_IDX_ACTIVE).  Slot s's J tile takes over slot s's I tile.
struct ExactTile {
    static constexpr int kColDw = 29, kCols = 27, kTileDw = kCols * kColDw;      // 783 dwords per slot
    static constexpr int kStoreCols = kCols;                       // nothing spills: slot 3's tile ends the wave's region
    static constexpr int kQPairs = 23, kJPairs = 27, kJMargin = 3;
    static constexpr bool kAlignedI = true;
};
constexpr int kLdsDwPerWave = kSlots * ExactTile::kTileDw;         // 3132 dwords
// the I tile's last column read: offI <= 3, + 7 * 2 (segment) + 9; the J tile's: j_span_x + kWindowCols - 1
static_assert(3 + 14 + 9 < ExactTile::kCols && j_span_x<ExactTile>() == 5 && ExactTile::kJMargin <= j_span_x<ExactTile>(), "tile columns");
static_assert(kLdsDwPerWave * 4 <= 10 * 1280, "ten LDS granules per wave: twelve single-wave workgroups per CU");

// Diagnostic build (-DSVO_LK_STAMP=k, tools/gpu/lk_stamps.sh): every wave adds the s_memtime cycles it spends in
// section k of lk_call4 (between stamp points k and k + 1; k = 8: the whole call) to a counter read back with
// svo_debug_lk_stamps.  ONE section per build: a stamp drains the LDS queue and waits for the scalar memory
// unit, and stamping every section at once tripled the kernel's time and measured mostly the stamps.
#ifdef SVO_LK_STAMP
__device__ unsigned long long g_lk_stamp[2 * 1024];      // 1024 slots (by workgroup) against atomic contention; summed on read-back
__device__ __forceinline__ uint32_t lk_now() { return (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)__builtin_amdgcn_s_memtime()); }
#define LK_STAMP_DECL uint32_t lk_t_ = 0, lk_acc_ = 0, lk_n_ = 0
#define LK_AT(i) do { if ((i) == SVO_LK_STAMP) lk_t_ = lk_now(); else if ((i) == SVO_LK_STAMP + 1) { lk_acc_ += lk_now() - lk_t_; lk_n_++; } } while (0)
#define LK_CALL_BEGIN do { if (SVO_LK_STAMP == 8) lk_t_ = lk_now(); } while (0)
#define LK_CALL_END(lane) do { if (SVO_LK_STAMP == 8) { lk_acc_ += lk_now() - lk_t_; lk_n_++; } \
    if ((lane) == 0) { atomicAdd(&g_lk_stamp[2 * (blockIdx.x & 1023)], (unsigned long long)lk_acc_); atomicAdd(&g_lk_stamp[2 * (blockIdx.x & 1023) + 1], (unsigned long long)lk_n_); } } while (0)
#else
#define LK_STAMP_DECL
#define LK_AT(i)
#define LK_CALL_BEGIN
#define LK_CALL_END(lane)
#endif


// per-lane constants of the pixel role
struct PixLane { int row, seg; uint32_t onmask, qoff; };   // qoff: byte offset of the lane's first I-tile word inside a slot tile

// ---- phase A for one slot: this lane's 7 patch pixels from the staged I tile -------------------
// Tile rows row..row+3 = image rows ipy+row-1..ipy+row+2, columns j = 0..9 = image columns
// ipx-1+seg*7+j (scharr_columns, lk_common.h).
// Outputs: packed patch derivatives (Ix, Iy as 4 pairs each; pair 3 has a zero high half), the
// lane's NEGATED constants -sum(I*Ix), -sum(I*Iy) over its 7 pixels, and the three partial sums of
// Ix^2, Ix*Iy, Iy^2.  The iterations need I only inside sum((J - I) * Ix) = sum(J*Ix) - sum(I*Ix):
// the second term does not change, so the per-iteration mismatch chain starts from the negated
// constant instead of subtracting I from every J sample (exact: integers, |partial| < 2^29).
template <bool EDGE>
__device__ __forceinline__ void patch_slot(uint32_t tile_addr, const PixLane &pl, uint32_t Wau,
                                           uint32_t Wbu, int ipx, int ipy, int w, int h,
                                           uint32_t (&IxP)[4], uint32_t (&IyP)[4], int &nIIx, int &nIIy,
                                           int &pA11, int &pA12, int &pA22)
{
    uint32_t IvP[4];
    // (lane 63 carries no window pixel: zero weights make its I, Ix, Iy and sums vanish; `onmask` is
    //  all ones in the pixel lanes, zero in lane 63 -- one v_and per weight word)
    const uint32_t Wa = Wau & pl.onmask, Wb = Wbu & pl.onmask;
    // (tile_addr: the slot's tile + offI columns, wave-uniform; qoff: the lane's column / row-pair offset)
    uint32_t Q12[10], DX[8], DY[8];
    scharr_columns<10, ExactTile::kColDw, EDGE>((lds_cu32 *)(size_t)(tile_addr + pl.qoff), ipx + pl.seg * 7, ipy + pl.row, w, h, Q12, DX, DY);
    int iv[8], ix[8], iy[8];
    iv[7] = ix[7] = iy[7] = 0;
    patch_samples<10>(Q12, DX, DY, Wa, Wb, iv, ix, iy);
    pA11 = 0; pA12 = 0; pA22 = 0;
    int sIIx = 0, sIIy = 0;
#pragma unroll
    for (int m = 0; m < 4; m++) {
        IvP[m] = perm_b32((uint32_t)iv[2 * m + 1], (uint32_t)iv[2 * m], 0x05040100u);
        IxP[m] = perm_b32((uint32_t)ix[2 * m + 1], (uint32_t)ix[2 * m], 0x07060302u);      // the two high halves
        IyP[m] = perm_b32((uint32_t)iy[2 * m + 1], (uint32_t)iy[2 * m], 0x07060302u);
        pA11 = m == 0 ? dot2_0(IxP[m], IxP[m]) : dot2(IxP[m], IxP[m], pA11);
        pA12 = m == 0 ? dot2_0(IxP[m], IyP[m]) : dot2(IxP[m], IyP[m], pA12);
        pA22 = m == 0 ? dot2_0(IyP[m], IyP[m]) : dot2(IyP[m], IyP[m], pA22);
        sIIx = m == 0 ? dot2_0(IvP[m], IxP[m]) : dot2(IvP[m], IxP[m], sIIx);
        sIIy = m == 0 ? dot2_0(IvP[m], IyP[m]) : dot2(IvP[m], IyP[m], sIIy);
    }
    nIIx = -sIIx; nIIy = -sIIy;
}

// One iteration's mismatch sums of one slot from the lane's eight J column words (`vround`: j_sample_rounding)
__device__ __forceinline__ void mismatch_slot(const uint32_t (&C)[8], uint32_t Wa, uint32_t Wb,
                                              const uint32_t (&IxP)[4], const uint32_t (&IyP)[4], int nIIx, int nIIy,
                                              int vround, int &pb1, int &pb2)
{
    int d[7];
#pragma unroll
    for (int k = 0; k < 7; k++) d[k] = dot2(C[k + 1], Wb, dot2_sv(C[k], Wa, vround));
    // J samples = high halves of the sums (column words hold pixel << 7, vround = 2^15: (sum * 2^7) >> 16
    // = sum >> 9, 0 <= sum < 2^22): two of them side by side with one v_perm
#pragma unroll
    for (int m = 0; m < 4; m++) {
        const uint32_t vp = m < 3 ? perm_b32((uint32_t)d[2 * m + 1], (uint32_t)d[2 * m], 0x07060302u)
                                  : (uint32_t)d[6] >> 16;
        // the chains start from - sum(I * Ix), - sum(I * Iy) (see patch_slot); three-operand form for the
        // first link so that the constant is not copied into the accumulator first
        pb1 = m == 0 ? dot2_v(vp, IxP[m], nIIx) : dot2(vp, IxP[m], pb1);
        pb2 = m == 0 ? dot2_v(vp, IyP[m], nIIy) : dot2(vp, IyP[m], pb2);
    }
}


// Partial sums that are defined without an instruction.  DEAD SLOTS: a slot that does no pixel work in a pass (its bit
// of m_on / it_on is clear) hands the reduce-scatter (reduce_scatter8_rows for b, reduce_scatter12_rows for A) whatever
// these registers hold instead of zeros (zero-filling cost 8 v_mov per wave-iteration and 12 per level).  That garbage
// reaches neither a live slot nor a stored byte:
//   * neither reduce-scatter mixes slots: the two swap steps hand the values of slot s to row s of the wave and
//     every later step adds lanes of one row, so rows of live slots sum live values only (integer adds: no traps);
//   * row s's results are read by slot s's control lanes alone, and every use of what they become is guarded by that
//     slot's flag: A11, A12, A22, D, minEig, Dinv by "lvl_on &" in level_solve_setup and by it_on (a subset of lvl_on)
//     in the iterations; b1, b2 and the step by "it_on &" in iter_update's near-epsilon test, nextPt selects and
//     returned mask (lk_common.h spells the guards out next to each rule).
// (one statement for all sums of a slot: identical single definitions are merged into one register and copied apart)
__device__ __forceinline__ void undefined_sums(int &x, int &y) { asm("" : "=v"(x), "=v"(y)); }
__device__ __forceinline__ void undefined_sums(int &x, int &y, int &z) { asm("" : "=v"(x), "=v"(y), "=v"(z)); }

// One cv::calcOpticalFlowPyrLK call for the wave's four points.  Control values (prevPt, outPt) are per lane = per
// slot lane >> 4, flags (status, live) lane masks; the rules they follow are lk_common.h's.
__device__ __forceinline__ void lk_call4(const PyrGeom &g, const uint8_t *slotI, const uint8_t *slotJ, float2 prevPt,
                                         float2 &outPt, lanemask &status, lanemask live, uint32_t *lds, const uint32_t *lds_wg,
                                         int wave_off, int lane)
{
    typedef ExactTile T;
    LK_STAMP_DECL;
    LK_CALL_BEGIN;
    PixLane pl;
    pl.row = min(lane / 3, kWin - 1); pl.seg = lane - (lane / 3) * 3; pl.onmask = lane < 63 ? ~0u : 0u;
    pl.qoff = (uint32_t)((pl.seg * 7 * T::kColDw + pl.row) * 4);
    asm volatile("" : "+v"(pl.onmask));                       // keep it a mask (one v_and per weight word), not a select

    uint32_t IxP[kSlots][4], IyP[kSlots][4];
    int nIIx[kSlots], nIIy[kSlots];
    // lane part of the J sample offset, the wave's LDS region included (bytes from the workgroup array)
    const int lane_off = (pl.seg * 7 * T::kColDw + pl.row) * 4 + wave_off;
    const StageLane q = stage_lane<T::kColDw>(lane);
    const uint32_t lds_base = (uint32_t)(size_t)(lds_cu32 *)lds;   // byte address of the wave's LDS region
    const int vround = j_sample_rounding();
    status = ~0ull;
    float nx = 0.f, ny = 0.f;                    // nextPts[i]
    uint32_t rI[kSlots][3][2];
    uint32_t q_src[3], q_next[3];                // lane part of the tile source offsets at the level / at the next one
    request_I<T>(rI, q_src, g, g.nlevels - 1, slotI, prevPt, live, q, lane);
    for (int level = g.nlevels - 1; level >= 0; --level) {
        LK_AT(0);
        // ---- control: window position and weights of every slot, the J window of the first iteration
        LkLevel lv = level_begin<T>(g, level, prevPt, live, nx, ny, status);
        lanemask lvl_on = lv.on;
        const int w = lv.w, h = lv.h, pitch = g.pitch[level];
        const int offI = (lv.ipx - 1) - i_tile_x0<T>(lv.ipx);
        const lanemask m_on = lvl_on, m_j = lv.j_staged;
        uint32_t rJ[kSlots][3][2];
        // ---- I tiles (as row-pair column words; all four fit the wave's LDS region, which the J tiles
        //      take over afterwards), patches + A sums
        int pA[kSlots][3];
#pragma unroll
        for (int s = 0; s < kSlots; s++) {
            if (!slot_bit(m_on, s)) continue;
            tile_store_i<T>(lds + s * T::kTileDw, rI[s], q, lane);
        }
        // the J tiles are requested now (vmcnt counts in order: the waits above were for the I tiles only)
#pragma unroll
        for (int s = 0; s < kSlots; s++) {
            if (!slot_bit(m_j, s)) continue;
            tile_request<T::kJPairs>(rJ[s], g, level, pitch, slotJ, lv.tx0, lv.ty0, s, q_src, lane);
        }
        wave_lds_fence();
        LK_AT(1);                                // 0 -> 1: level control, I staging, J requests
#pragma unroll
        for (int s = 0; s < kSlots; s++) {
            undefined_sums(pA[s][0], pA[s][1], pA[s][2]);      // dead slots: above
            if (!slot_bit(m_on, s)) continue;
            const uint32_t qaddr = lds_base + (uint32_t)((s * T::kTileDw + __builtin_amdgcn_readlane(offI, 16 * s) * T::kColDw) * 4);
            const uint32_t W01s = __builtin_amdgcn_readlane(lv.WIa, 16 * s), W23s = __builtin_amdgcn_readlane(lv.WIb, 16 * s);
            const int ipxs = __builtin_amdgcn_readlane(lv.ipx, 16 * s), ipys = __builtin_amdgcn_readlane(lv.ipy, 16 * s);
            if (__builtin_expect(ipxs < 0 || ipxs + kWin >= w || ipys < 0 || ipys + kWin >= h, 0))     // the window hangs over the edge
                patch_slot<true>(qaddr, pl, W01s, W23s, ipxs, ipys, w, h, IxP[s], IyP[s], nIIx[s], nIIy[s],
                                 pA[s][0], pA[s][1], pA[s][2]);
            else
                patch_slot<false>(qaddr, pl, W01s, W23s, ipxs, ipys, w, h, IxP[s], IyP[s], nIIx[s], nIIy[s],
                                  pA[s][0], pA[s][1], pA[s][2]);
        }
        LK_AT(2);                                // 1 -> 2: patch_slot x 4
        wave_lds_fence();                        // the J tiles reuse the I tiles' LDS
#pragma unroll
        for (int s = 0; s < kSlots; s++) {
            if (!slot_bit(m_j, s)) continue;
            tile_store_j<T, false>(lds + s * T::kTileDw, rJ[s], q, lane);
        }
        wave_lds_fence();
        float A11, A12, A22;
        {
            int r1, r2;                          // row s: {A11.lo, A12.lo, A11.hi, A12.hi}, {A22.lo, A22.lo, A22.hi, A22.hi} of slot s
            reduce_scatter12_rows(pA, lane, r1, r2);
            A11 = wide_to_f32(quad_bcast<2>(r1), quad_bcast<0>(r1)) * kFltScale;
            A12 = wide_to_f32(quad_bcast<3>(r1), quad_bcast<1>(r1)) * kFltScale;
            A22 = wide_to_f32(quad_bcast<2>(r2), quad_bcast<0>(r2)) * kFltScale;
        }
        float Dinv;
        lvl_on = level_solve_setup(A11, A12, A22, level, lvl_on, status, Dinv);

        // ---- iterations (all slots in lockstep; a slot drops out when it converges or leaves)
        if (level > 0) request_I<T>(rI, q_next, g, level - 1, slotI, prevPt, live, q, lane);
        LK_AT(3);                                // 2 -> 3: J stores, A reduction, 2x2 set-up, next level's I requests
        float pdx = 0.f, pdy = 0.f;
        lanemask it_on = lvl_on;
        for (int j = 0; j < kLkMaxIter; j++) {
            if (!it_on) break;
            LK_AT(4);
            const LkIter it = iter_begin<T>(lv.qx, lv.qy, w, h, level, lane, it_on, status, lv.tx0, lv.ty0);
            it_on = it.on;
            const lanemask m_it = it_on, m_rs = it.restage;
            if (__builtin_expect(m_rs != 0, 0)) {     // a window drifted out of its tile
#pragma unroll
                for (int s = 0; s < kSlots; s++) {
                    if (!slot_bit(m_rs, s)) continue;
                    uint32_t r[3][2];
                    tile_request<T::kJPairs>(r, g, level, pitch, slotJ, lv.tx0, lv.ty0, s, q_src, lane);
                    tile_store_j<T, false>(lds + s * T::kTileDw, r, q, lane);
                }
                wave_lds_fence();
            }
            LK_AT(5);                            // 4 -> 5: iteration control: floor, weights, restage test
            int pb[kSlots][2];
#pragma unroll
            for (int s = 0; s < kSlots; s++) {
                undefined_sums(pb[s][0], pb[s][1]);                // dead slots: above
                if (!slot_bit(m_it, s)) continue;
                const int joffs = __builtin_amdgcn_readlane(it.joff, 16 * s);
                const uint32_t Was = __builtin_amdgcn_readlane(it.Wa, 16 * s), Wbs = __builtin_amdgcn_readlane(it.Wb, 16 * s);
                // byte address = workgroup array + slot part (SGPR) + lane part: one add, no re-alignment of an index
                lds_cu32 *pj = (lds_cu32 *)(size_t)((uint32_t)(size_t)(lds_cu32 *)lds_wg + (uint32_t)(joffs + lane_off));
                uint32_t C[8];
#pragma unroll
                for (int k = 0; k < 8; k++) C[k] = pj[k * T::kColDw];
                mismatch_slot(C, Was, Wbs, IxP[s], IyP[s], nIIx[s], nIIy[s], vround, pb[s][0], pb[s][1]);
            }
            LK_AT(6);                            // 5 -> 6: slot pixel work: J reads, bilinear + mismatch dot products
            float b1f, b2f;
            {
                int v[8];
#pragma unroll
                for (int s = 0; s < kSlots; s++) { v[2 * s] = pb[s][0]; v[2 * s + 1] = pb[s][1]; }
                const int r = reduce_scatter8_rows(v, lane);       // row s: {b1.lo, b2.lo, b1.hi, b2.hi} of slot s in every quad
                b1f = wide_to_f32(quad_bcast<2>(r), quad_bcast<0>(r)) * kFltScale;
                b2f = wide_to_f32(quad_bcast<3>(r), quad_bcast<1>(r)) * kFltScale;
            }
            it_on = iter_update(A11, A12, A22, Dinv, b1f, b2f, j, it_on, lv.qx, lv.qy, nx, ny, pdx, pdy);
            LK_AT(7);                            // 6 -> 7: reduce-scatter, solve, convergence tests
        }
        final_window_check(nx, ny, w, h, level, live, status);
        if (level > 0) {
#pragma unroll
            for (int t = 0; t < 3; t++) q_src[t] = q_next[t];
        }
    }
    outPt = make_float2(nx, ny);
    LK_CALL_END(lane);
}

// Waves per workgroup (4, 2 or 1; -DSVO_LK_WAVES_PER_WG=k for A/B builds).  The waves of a workgroup share
// nothing but the LDS allocation, and a workgroup gives its LDS back only when its SLOWEST wave has ended:
// with four waves the slots of the finished ones stay empty until then, because no other workgroup fits
// beside 3 x 50 KB.  With single-wave workgroups the hardware dispatcher is the
// work queue: a wave that ends frees its LDS at once and the next one starts.
#ifndef SVO_LK_WAVES_PER_WG
#define SVO_LK_WAVES_PER_WG 1
#endif
constexpr int kLkWavesPerWg = SVO_LK_WAVES_PER_WG;
static_assert(kLkWavesPerWg == 4 || kLkWavesPerWg == 2 || kLkWavesPerWg == 1, "lk_kernel: 4, 2 or 1 waves per workgroup");
// The latency shape (launches of fewer than 4 items) stays at four: measured when a lone wave's tiles took eleven LDS
// granules (28-column tiles: eleven waves per CU where three four-wave workgroups held twelve; stream k = 2: -3 % as
// single waves).  Its waves all start at once, so it has nothing to gain from the early hand-back.
constexpr int kLkSpreadWavesPerWg = 4;

// Grid and item mapping: lk_track_item (lk_common.h); a wave's LDS region is its four slot tiles.
template <int W>
__global__ __launch_bounds__(64 * W) __attribute__((amdgpu_waves_per_eu(3, 3))) void lk_kernel(LkArgs a)
{
    __shared__ uint32_t lds[W * kLdsDwPerWave];
    const int wave = W == 1 ? 0 : (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
    uint32_t *my = lds + wave * kLdsDwPerWave;
    lk_track_item<W>(a, wave, lane, [&](const uint8_t *sI, const uint8_t *sJ, float2 cur, float2 &nxt, lanemask &st, lanemask live) {
        lk_call4(a.g, sI, sJ, cur, nxt, st, live, my, lds, wave * (kLdsDwPerWave * 4), lane);
    });
}

// Stable compaction (deleteBadmatchFeatures erases in place, preserving order): one workgroup of
// 1024 threads per batch item, ballot/popcount ranks inside waves, LDS scan across waves.
__global__ __launch_bounds__(1024) void compact_kernel(CompactArgs a)
{
    __shared__ int wave_tot[16];
    __shared__ int base_s;
    const int b = blockIdx.x;
    int n = a.n_pts ? a.n_pts[b] : a.n_fixed;
    n = min(n, a.cap);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t o = (int64_t)b * a.pts_stride;
    if (threadIdx.x == 0) base_s = 0;
    __syncthreads();
    for (int start = 0; start < n; start += 1024) {
        int i = start + threadIdx.x;
        bool k = i < n && a.keep[o + i] != 0;
        unsigned long long m = __ballot(k);
        int rank = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) wave_tot[wv] = __popcll(m);
        __syncthreads();
        int pre = 0, tot = 0;
        for (int q = 0; q < 16; q++) { int t = wave_tot[q]; if (q < wv) pre += t; tot += t; }
        int dst = base_s + pre + rank;
        if (k) {
#pragma unroll
            for (int c = 0; c < 4; c++) a.out[c][o + dst] = a.in[c][o + i];
        }
        __syncthreads();
        if (threadIdx.x == 0) base_s += tot;
        __syncthreads();
    }
    if (threadIdx.x == 0) a.m_out[b] = base_s;
}

#ifdef SVO_LK_STAMP
extern "C" int svo_debug_lk_stamps(unsigned long long out[2], int reset)
{
    static unsigned long long h[2 * 1024];
    if (hipMemcpyFromSymbol(h, HIP_SYMBOL(g_lk_stamp), sizeof(h)) != hipSuccess) return -1;
    out[0] = out[1] = 0;
    for (int i = 0; i < 1024; i++) { out[0] += h[2 * i]; out[1] += h[2 * i + 1]; }
    if (reset) { memset(h, 0, sizeof(h)); if (hipMemcpyToSymbol(HIP_SYMBOL(g_lk_stamp), h, sizeof(h)) != hipSuccess) return -1; }
    return 0;
}
#endif

void launch_lk(const LkArgs &a0, int batch, int max_pts, hipStream_t st)
{
    if (max_pts <= 0 || batch <= 0) return;
    if (a0.accum != 0) { launch_lk_sse2(a0, batch, max_pts, st); return; }      // SVO_LK_ACCUM_SSE2 / _SIMD128: the float-order kernel
    // up to 768 waves per item (3072 points per pass: a KITTI frame's ~2.5 k corners in one pass, a few
    // waves leave at once; denser frames loop), never more than capacity / 4
    constexpr int W = kLkWavesPerWg;
    const int chunks = (max_pts + W * kSlots - 1) / (W * kSlots);
    LkArgs a = a0;
    a.gx = chunks < 768 / W ? chunks : 768 / W;
    a.spread = 0;
    a.batch = batch;
    if (batch < 4) {                             // fewer than 768 workgroups of four: 3 per CU are resident at once
        static const int room_all = getenv("SVO_LK_SPREAD_ROOM") ? atoi(getenv("SVO_LK_SPREAD_ROOM")) : 768;     // test hook (A/B runs)
        const int wide = (max_pts + 3) / 4, room = room_all / batch;
        a.gx = wide < room ? wide : room;
        a.spread = 1;
        hipLaunchKernelGGL(lk_kernel<kLkSpreadWavesPerWg>, dim3(batch * a.gx), dim3(64 * kLkSpreadWavesPerWg), 0, st, a);
        return;
    }
    hipLaunchKernelGGL(lk_kernel<W>, dim3(batch * a.gx), dim3(64 * W), 0, st, a);
}

void launch_compact(const CompactArgs &a, int batch, hipStream_t st)
{
    if (batch <= 0) return;
    hipLaunchKernelGGL(compact_kernel, dim3(batch), dim3(1024), 0, st, a);
}

}  // namespace svo
