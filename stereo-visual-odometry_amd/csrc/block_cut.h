// block_cut.h -- rounding up, and cutting ONE block of device memory into aligned sub-ranges (host only: no HIP include).
#pragma once
#include <cstddef>

namespace svo {
constexpr size_t kDevAlign = 256;          // every sub-range of a device block starts on a multiple of this

constexpr size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// Offsets of consecutive sub-ranges, in the order they are asked for.  add(bytes) returns where the range starts and moves
// the end up to the next multiple of kDevAlign behind it; a zero-byte range starts where the next one will and consumes
// nothing.  total() is the size of the block that holds them all.
struct BlockCut {
    size_t end = 0;
    size_t add(size_t bytes) { const size_t at = end; end += align_up(bytes, kDevAlign); return at; }
    size_t total() const { return end; }
};
}  // namespace svo
