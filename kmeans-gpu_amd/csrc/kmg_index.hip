// kmg_index.hip -- index output (kmg_output_format INDEX8 / INDEX16) of the two routes whose RGBA8 kernels live
// in kmg_table.hip (pinned to the counter profiles, tests/test_profiles_fresh.py):
//   k_labels_index -- the replace pass through the colour cube's label tables: the lookups of k_labels_pairs (k <= 256) and
//                     k_labels (k > 256) on the same tables, writing the label instead of pal[label];
//   k_narrow_index -- the mask-word dither route: its kernels run unchanged with an identity palette into u32 scratch, and this
//                     pass narrows those labels to u8 / u16 (extra traffic: 4 B written + 4 B read per pixel).
// Alpha mode: a pixel whose alpha byte is below the cutoff is written as k, the transparent slot.

#include "kmg_internal.h"
#include "kmg_table_dev.h"

namespace kmg {

namespace {

constexpr int kIndexBlock = 1024;

// PAIRS (k <= 256): k_labels_pairs without hot cells -- the cell's pair entry in LDS decides a pixel unless the plane puts it in
// the slab, where the u8 per-colour label does.  !PAIRS (k > 256): k_labels -- the 8x8x8 summary in LDS, the 4x4x4 summary, the
// u16 per-colour label.
template <typename OutT, bool ALPHA, bool PAIRS>
__global__ __launch_bounds__(kIndexBlock) void k_labels_index(const uint32_t *__restrict__ rgba, uint64_t n,
                                                              const void *__restrict__ colour_labels,
                                                              const uint16_t *__restrict__ sub_table, uint32_t k,
                                                              OutT *__restrict__ out, int aligned, uint32_t cutoff)
{
    __shared__ uint32_t s_lds[PAIRS ? kCells + 128 : kCells / 2];
    if (PAIRS) {
        const uint4 *src = reinterpret_cast<const uint4 *>(sub_table + kSubCells + kCells);
        uint4 *dst = reinterpret_cast<uint4 *>(s_lds);
        for (uint32_t i = threadIdx.x; i < kCells / 4; i += kIndexBlock) dst[i] = src[i];
        if (threadIdx.x < 128) s_lds[kCells + threadIdx.x] = threadIdx.x < kPairDirs ? pair_dir_word(threadIdx.x) : 0u;
    } else {
        const uint4 *src = reinterpret_cast<const uint4 *>(sub_table + kSubCells);
        uint4 *dst = reinterpret_cast<uint4 *>(s_lds);
        for (uint32_t i = threadIdx.x; i < kCells / 8; i += kIndexBlock) dst[i] = src[i];
    }
    __syncthreads();
    const uint32_t *s_pair = s_lds, *s_dir = s_lds + kCells;
    const uint16_t *s_cell = reinterpret_cast<const uint16_t *>(s_lds);
    constexpr uint64_t TILE = (uint64_t)kIndexBlock * 8;
    const uint64_t tiles = (n + TILE - 1) / TILE;
    for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        uint32_t px[8], ci[8];
        uint64_t i0[2];
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            i0[g] = tile * TILE + (uint64_t)g * (kIndexBlock * 4) + (uint64_t)threadIdx.x * 4;
            load4_stream(rgba, i0[g], n, aligned != 0, px + g * 4);
#pragma unroll
            for (int q = 0; q < 4; ++q) ci[g * 4 + q] = colour_index(px[g * 4 + q]);
        }
        uint32_t lab[8];
        if (PAIRS) {
            bool fine[8];
#pragma unroll
            for (int p = 0; p < 8; ++p) {
                const uint32_t e = s_pair[ci[p] >> 9];
                const uint32_t dirw = s_dir[(e >> 16) & 127u];
                const uint32_t xyz = (px[p] & 0x00070707u) | 0x01000000u;   // (r & 7, g & 7, b & 7, 1)
                const int proj = __builtin_amdgcn_sdot4((int)xyz, (int)dirw, 0, false);
                const int tlo = (int)((e >> 23) & 63u), w = (int)(e >> 29);
                const bool inA = proj < tlo, inB = proj >= tlo + w + (w == 7 ? 64 : 0);
                lab[p] = inA ? (e & 0xFFu) : ((e >> 8) & 0xFFu);
                fine[p] = !(inA || inB);
            }
#pragma unroll
            for (int p = 0; p < 8; ++p)
                if (fine[p]) lab[p] = (uint32_t)static_cast<const uint8_t *>(colour_labels)[ci[p]];
        } else {
#pragma unroll
            for (int p = 0; p < 8; ++p) lab[p] = (uint32_t)s_cell[ci[p] >> 9];
#pragma unroll
            for (int p = 0; p < 8; ++p)
                if (lab[p] == kSubMixed) lab[p] = (uint32_t)sub_table[ci[p] >> 6];
#pragma unroll
            for (int p = 0; p < 8; ++p)
                if (lab[p] == kSubMixed) lab[p] = (uint32_t)static_cast<const uint16_t *>(colour_labels)[ci[p]];
        }
#pragma unroll
        for (int p = 0; p < 8; ++p) lab[p] = index_of<ALPHA>(lab[p], px[p], cutoff, k);
#pragma unroll
        for (int g = 0; g < 2; ++g) store4_index<OutT, true>(out, i0[g], n, aligned != 0, lab + g * 4);
    }
}

template <typename OutT, bool ALPHA>
__global__ __launch_bounds__(kBlock) void k_narrow_index(const uint32_t *__restrict__ rgba, const uint32_t *__restrict__ labels,
                                                         uint64_t n, uint32_t k, OutT *__restrict__ out, int aligned, uint32_t cutoff)
{
    const uint64_t groups = (n + 3) / 4;
    for (uint64_t g = (uint64_t)blockIdx.x * kBlock + threadIdx.x; g < groups; g += (uint64_t)gridDim.x * kBlock) {
        const uint64_t i0 = g * 4;
        uint32_t lab[4], px[4] = {0u, 0u, 0u, 0u};
        load4_stream(labels, i0, n, aligned != 0, lab);
        if (ALPHA) load4_stream(rgba, i0, n, aligned != 0, px);
#pragma unroll
        for (int q = 0; q < 4; ++q) lab[q] = index_of<ALPHA>(lab[q], px[q], cutoff, k);
        store4_index<OutT, true>(out, i0, n, aligned != 0, lab);
    }
}

}  // namespace

hipError_t launch_labels_index(const uint32_t *rgba, uint64_t n, const void *colour_labels, const uint16_t *sub_table, uint32_t k,
                               void *out, int format, hipStream_t st, uint32_t alpha_cutoff)
{
    const uint64_t tiles = (n + kIndexBlock * 8 - 1) / (kIndexBlock * 8);
    // as launch_labels: one workgroup per CU with the 128 KiB pair table, two with the 64 KiB summaries
    const uint32_t cap = k <= 256 ? device_info().cus : 2u * device_info().cus;
    const uint32_t grid = (uint32_t)(tiles < cap ? (tiles ? tiles : 1) : cap);
    const bool known = with_index_type(format, [&](auto t) { with_bool(alpha_cutoff != 0, [&](auto A) { with_bool(k <= 256, [&](auto P) {
        using OutT = typename decltype(t)::type;
        hipLaunchKernelGGL((k_labels_index<OutT, A(), P()>), dim3(grid), dim3(kIndexBlock), 0, st, rgba, n, colour_labels, sub_table, k,
                           static_cast<OutT *>(out), output_aligned<OutT>(rgba, out), alpha_cutoff);
    }); }); });
    return known ? hipGetLastError() : hipErrorInvalidValue;
}

hipError_t launch_narrow_index(const uint32_t *rgba, const uint32_t *labels, uint64_t n, uint32_t k, void *out, int format, hipStream_t st,
                               uint32_t alpha_cutoff)
{
    const uint64_t blocks = ((n + 3) / 4 + kBlock - 1) / kBlock;
    const uint32_t grid = (uint32_t)(blocks < 4096 ? (blocks ? blocks : 1) : 4096);
    const bool known = with_index_type(format, [&](auto t) { with_bool(alpha_cutoff != 0, [&](auto A) {
        using OutT = typename decltype(t)::type;
        // (labels: the plan's own scratch, 256-byte aligned; the source's alignment decides for both loads)
        const int aligned = output_aligned<OutT>(rgba, out) & output_aligned<uint32_t>(labels, labels);
        hipLaunchKernelGGL((k_narrow_index<OutT, A()>), dim3(grid), dim3(kBlock), 0, st, rgba, labels, n, k, static_cast<OutT *>(out), aligned,
                           alpha_cutoff);
    }); });
    return known ? hipGetLastError() : hipErrorInvalidValue;
}

}  // namespace kmg
