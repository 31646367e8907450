// pinned_layout.h -- how the context's page-locked host scratch (svo_ctx::h_pinned) is cut up (host only: no HIP include).
#pragma once
#include "block_cut.h"

namespace svo {
constexpr size_t kPinnedInts = 64;         // device counts read back: a call names the positions it uses

// Three disjoint ranges, in this order, each aligned as BlockCut aligns; svo_create allocates `total` bytes.
//   ints    : kPinnedInts ints;
//   block   : the largest list any call reads back THROUGH pinned memory -- svo_orb_extract's max_keypoints records + 32-byte
//             descriptors, svo_fast_detect's xy + response lists (12 bytes per corner), or one fixed record (`fixed_bytes`: the
//             largest of them);
//   records : max_batch step records (deliver_records).
struct PinnedLayout {
    size_t ints = 0, ints_bytes = 0, block = 0, block_bytes = 0, records = 0, records_bytes = 0, total = 0;
};

inline PinnedLayout pinned_layout(size_t max_keypoints, size_t max_batch, size_t keypoint_bytes, size_t step_bytes, size_t fixed_bytes)
{
    PinnedLayout l;
    l.ints_bytes = sizeof(int) * kPinnedInts;
    l.block_bytes = max_keypoints * (keypoint_bytes + 32);
    if (l.block_bytes < max_keypoints * 12) l.block_bytes = max_keypoints * 12;
    if (l.block_bytes < fixed_bytes) l.block_bytes = fixed_bytes;
    l.records_bytes = max_batch * step_bytes;
    BlockCut cut;
    l.ints = cut.add(l.ints_bytes);
    l.block = cut.add(l.block_bytes);
    l.records = cut.add(l.records_bytes);
    l.total = cut.total();
    return l;
}
}  // namespace svo
