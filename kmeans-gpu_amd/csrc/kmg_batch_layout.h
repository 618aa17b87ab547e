// kmg_batch_layout.h -- where the images of a sub-batch lie in one device block and in the grid of a batched launch (kmg_batch.hip,
// kmg_batch_apply.hip).  Host only, no device, no processor: plain C++ that a host test can include
// (tests/native/check_batch_layout.cpp).
#pragma once

#include <stdint.h>

#include <vector>

namespace kmg {

// workgroups of one batched launch at most; a larger batch runs as several pieces, one after the other
constexpr uint64_t kBatchMaxGrid = 1ull << 20;
// every image of a packed block starts at a multiple of this: the 16-byte loads of load4 and the vector stores of store4 /
// store4_index (4, 8 or 16 bytes) then are aligned for every format, and no vector access of one image reaches a neighbour's bytes
// (the vector paths are taken for four pixels in range only)
constexpr uint64_t kBatchAlign = 16;

constexpr uint64_t kBatchDefaultResident = 1ull << 30;   // what max_resident_bytes = 0 stands for (include/kmeans_hip.h)

// The sub-batches of n >= 1 images that keep bytes[i] on the device each: consecutive images [c[s], c[s + 1]), 0 = c[0] < ... < c[m] = n,
// filled greedily -- image i opens a new one when it is not the first of its own and the bytes held plus its own exceed the bound
// (0 = kBatchDefaultResident); an image larger than the bound is alone.  No sum wraps: a sub-batch that has an image grows within the bound.
inline std::vector<uint32_t> batch_cuts(const uint64_t *bytes, uint32_t n, uint64_t bound)
{
    if (!bound) bound = kBatchDefaultResident;
    std::vector<uint32_t> cuts(1, 0u);
    uint64_t held = 0;
    for (uint32_t i = 0; i < n; ++i) {
        if (i > cuts.back() && (held > bound || bytes[i] > bound - held)) { cuts.push_back(i); held = 0; }
        held += bytes[i];
    }
    cuts.push_back(n);
    return cuts;
}

// Packed block: offset[i] = the byte offset of image i (pixels[i] pixels of bytes_per_pixel bytes), *total = the bytes of the block.
// false: a size does not fit 64 bits or the block would exceed `limit` bytes; nothing is to be allocated then.
inline bool batch_offsets(const uint64_t *pixels, uint32_t m, uint32_t bytes_per_pixel, std::vector<uint64_t> &offset, uint64_t *total,
                          uint64_t limit = UINT64_MAX - kBatchAlign)
{
    offset.assign(m, 0);
    uint64_t at = 0;
    for (uint32_t i = 0; i < m; ++i) {
        if (bytes_per_pixel && pixels[i] > (UINT64_MAX - kBatchAlign) / bytes_per_pixel) return false;
        const uint64_t bytes = (pixels[i] * bytes_per_pixel + (kBatchAlign - 1)) & ~(kBatchAlign - 1);
        offset[i] = at;
        if (bytes > limit || at > limit - bytes) return false;
        at += bytes;
    }
    *total = at;
    return true;
}

// The grid of a batched pass with `tile` pixels per workgroup: first_wg[i] = the index of image i's first workgroup, *grid = the
// sum of the images' tiles (an image of p pixels has ceil(p / tile) of them).  false: the grid does not fit the 32 bits of a
// record's first-workgroup column.
inline bool batch_grid(const uint64_t *pixels, uint32_t m, uint64_t tile, std::vector<uint32_t> &first_wg, uint64_t *grid)
{
    first_wg.assign(m, 0);
    uint64_t at = 0;
    for (uint32_t i = 0; i < m; ++i) {
        const uint64_t tiles = pixels[i] / tile + (pixels[i] % tile ? 1u : 0u);
        first_wg[i] = (uint32_t)at;
        if (tiles > 0xFFFFFFFFull || at + tiles > 0xFFFFFFFFull) return false;
        at += tiles;
    }
    *grid = at;
    return true;
}

// The launches of a grid: workgroups [first, first + count) each, count <= bound, in order, covering [0, grid) once.
struct BatchLaunch { uint32_t first, count; };

inline std::vector<BatchLaunch> batch_launches(uint64_t grid, uint64_t bound = kBatchMaxGrid)
{
    std::vector<BatchLaunch> cuts;
    for (uint64_t at = 0; at < grid; at += bound) cuts.push_back({(uint32_t)at, (uint32_t)(grid - at < bound ? grid - at : bound)});
    return cuts;
}

}  // namespace kmg
