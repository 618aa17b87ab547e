// kmg_index_plan.h -- the rule of kmg_index_plan (include/kmeans_hip.h): which palette entries an index map
// keeps, in which order, where the transparent slot goes and how many bits an index needs.  Host only, all integers, no device:
// plain C++ that a host test can include.
#pragma once

#include <stdint.h>

#include <algorithm>
#include <vector>

namespace kmg {

// the flag word (KMG_INDEX_* of include/kmeans_hip.h): the low two bits are the order
constexpr uint32_t kIndexOrderMask = 3u, kIndexOrderKeep = 0u, kIndexOrderUsage = 1u, kIndexOrderLuma = 2u;
constexpr uint32_t kIndexKeepUnused = 4u, kIndexKeepTransparent = 8u, kIndexTransparentFirst = 16u;
constexpr uint32_t kIndexFlagsAll = kIndexOrderMask | kIndexKeepUnused | kIndexKeepTransparent | kIndexTransparentFirst;
constexpr uint16_t kIndexDropped = 0xFFFFu;
constexpr uint32_t kIndexPlanMaxK = 3072u;                                  // KMG_MAX_K

struct IndexPlanInfo { uint32_t n_colors, n_slots; int32_t transparent; uint32_t bits; };

// the smallest of 1, 2, 4, 8, 16 with 2^bits >= n_slots (n_slots <= KMG_MAX_K + 1)
inline uint32_t index_bits(uint32_t n_slots) { return n_slots <= 2u ? 1u : n_slots <= 4u ? 2u : n_slots <= 16u ? 4u : n_slots <= 256u ? 8u : 16u; }

// 10000 x the Rec. 709 luma of a palette entry's bytes
inline uint32_t index_luma(const uint8_t *rgba) { return 2126u * rgba[0] + 7152u * rgba[1] + 722u * rgba[2]; }

// NULL when the plan was written, else why not (nothing written then).  usage: k + 2, palette: k x 4, remap: k + 1,
// out_palette: (k + 1) x 4 bytes, of which n_slots x 4 are written.
inline const char *index_plan(const uint64_t *usage, const uint8_t *palette, uint32_t k, uint32_t flags, uint16_t *remap,
                              uint8_t *out_palette, IndexPlanInfo *info)
{
    if (!usage || !palette || !remap || !out_palette || !info) return "a pointer is NULL";
    if (k == 0 || k > kIndexPlanMaxK) return "k is outside 1 .. KMG_MAX_K";
    const uint32_t order = flags & kIndexOrderMask;
    if ((flags & ~kIndexFlagsAll) || order == 3u) return "unknown flag bits or order";
    if (usage[k + 1] != 0) return "the map holds indices above k";

    std::vector<uint32_t> kept;
    kept.reserve(k);
    for (uint32_t i = 0; i < k; ++i)
        if (usage[i] > 0 || (flags & kIndexKeepUnused)) kept.push_back(i);
    const bool present = usage[k] > 0 || (flags & kIndexKeepTransparent);
    const uint32_t n_colors = (uint32_t)kept.size(), n_slots = n_colors + (present ? 1u : 0u);
    if (n_slots == 0) return "the record is all zero and no keep flag is set: nothing to index";

    // (kept is in ascending old index: a stable sort leaves ties there)
    if (order == kIndexOrderUsage)
        std::stable_sort(kept.begin(), kept.end(), [&](uint32_t a, uint32_t b) { return usage[a] > usage[b]; });
    else if (order == kIndexOrderLuma)
        std::stable_sort(kept.begin(), kept.end(), [&](uint32_t a, uint32_t b) { return index_luma(palette + 4u * a) < index_luma(palette + 4u * b); });

    const bool first = present && (flags & kIndexTransparentFirst);
    const uint32_t base = first ? 1u : 0u, slot = first ? 0u : n_colors;
    // out_palette may be the caller's `palette`: the kept colours are read before anything is written
    std::vector<uint8_t> pal((size_t)n_slots * 4u, 0u);
    for (uint32_t j = 0; j < n_colors; ++j)
        for (uint32_t c = 0; c < 4u; ++c) pal[(size_t)(base + j) * 4u + c] = palette[(size_t)kept[j] * 4u + c];
    for (uint32_t i = 0; i <= k; ++i) remap[i] = kIndexDropped;
    for (uint32_t j = 0; j < n_colors; ++j) remap[kept[j]] = (uint16_t)(base + j);
    if (present) remap[k] = (uint16_t)slot;
    std::copy(pal.begin(), pal.end(), out_palette);
    info->n_colors = n_colors;
    info->n_slots = n_slots;
    info->transparent = present ? (int32_t)slot : -1;
    info->bits = index_bits(n_slots);
    return nullptr;
}

}  // namespace kmg
