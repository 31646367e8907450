// fast_scratch.h -- tile shape of fast.hip's score kernel and the layout of the scratch through which it hands its corners
// to the emit kernel (internal; svo_create sizes the two buffers of FastArgs with these).
//
// FastArgs.score : the RECORDS.  Tile column tx owns the kFastTileW bytes at  y * spitch + tx * kFastTileW  of image row y,
//     spitch = fast_record_pitch(w).  They hold the row's corners inside the tile, left to right:
//       nms     : 2 bytes per corner, x - tx * kFastTileW in the low byte and the score in the high byte.  With strict 3x3
//                 NMS no two survivors are neighbours, so a row of tw <= kFastTileW pixels holds at most ceil(tw / 2) <=
//                 kFastTileW / 2 of them: 2 * kFastTileW / 2 bytes, the region exactly;
//       no nms  : 1 byte per corner (x - tx * kFastTileW; the response is 0), at most tw <= kFastTileW corners.
//     Both bounds hold for any image content and for partial tiles (the pitch covers whole tiles), so nothing is ever cut.
//     tests/test_gpu_fast_bounds.py::test_saturated_records pins both: tile rows of 32 survivors and of 64 corners, the last
//     record at rank 31 / 63, beside live records of the next tile column (inputs: tests/_fast_cases.py staircase_rows).
// FastArgs.rowcount : the COUNTS, one byte per (image row, tile column) in raster order -- byte y * tile_cols + tx, at most
//     kFastTileW <= 255 -- rounded up to whole 16-byte groups per image, fast_count_words(w, h) ints.
// Every byte the emit kernel reads is written by the tile that owns it in the same launch: nothing is zeroed beforehand.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace svo {

// 64 x 32: against 64 x 16 the halo rows and the barriers are shared by twice the pixels and the quick test fills its trips
// (18 x 34 dwords over 256 threads) -- fast_score_kernel 384 -> 299 us on 257 images of 1241 x 376; 64 x 48 gave 306 us
// (profiles/fast_sparse_ab.json).  The scratch layout does not depend on the height.
constexpr int kFastTileW = 64, kFastTileH = 32;
static_assert(kFastTileW <= 64, "one 64-bit occupancy word per tile row; a corner's x inside the tile and a row's count fit a byte");

__host__ __device__ inline int fast_tile_cols(int w) { return (w + kFastTileW - 1) / kFastTileW; }
inline int fast_record_pitch(int w) { return fast_tile_cols(w) * kFastTileW; }                 // bytes per image row of FastArgs.score
inline int64_t fast_count_words(int w, int h) { return (((int64_t)fast_tile_cols(w) * h + 15) / 16) * 4; }   // ints per image of FastArgs.rowcount

}  // namespace svo
