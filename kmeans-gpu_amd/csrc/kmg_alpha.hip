// kmg_alpha.hip -- alpha mode (kmg_options.alpha_cutoff, include/kmeans_hip.h): the ordered stream compaction that hands the kept
// pixels of an image to the unchanged Lloyd path (kmg_dev_alpha_compact).
//
// Two launches over the same partition of the image into the workgroups' runs of tiles (kmg_pass.h):
//   k_alpha_count    kept pixels of each run -> counts[g]
//   k_alpha_scatter  run g's first output index = counts[0] + ... + counts[g - 1] (every workgroup sums them itself: at most
//                    kPassMaxGrid words, from L2), then its tiles in order.  A lane holds four consecutive pixels; their kept
//                    count c (0..4) is split into its three bits, and one 64-bit ballot + mbcnt per bit gives the lane's offset
//                    inside its wave (sum of 2^b x mbcnt); the wave totals go through LDS for the wave's offset inside the tile;
//                    a running offset carries the run from tile to tile.  The last workgroup writes n_kept.
// Every store is a vector store; there are no atomics and no waits between workgroups.
// k_alpha_merge: the alpha pass-through of the two output routes whose kernels live in kmg_table.hip.

#include "kmg_pass.h"

namespace kmg {

namespace {

// bit q = pixel i0 + q exists and its alpha byte reaches the cutoff
__device__ __forceinline__ uint32_t kept_bits(const uint32_t px[4], uint64_t i0, uint64_t n, uint32_t cutoff)
{
    uint32_t m = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) m |= (i0 + (uint64_t)q < n && (px[q] >> 24) >= cutoff) ? 1u << q : 0u;
    return m;
}

__global__ __launch_bounds__(kPassBlock) void k_alpha_count(const uint32_t *__restrict__ rgba, uint64_t n, uint32_t cutoff,
                                                              unsigned long long *__restrict__ counts, int aligned)
{
    __shared__ unsigned long long s_part[kPassWaves];
    uint64_t t0, t1;
    tile_run((n + kPassTile - 1) / kPassTile, t0, t1);
    uint32_t mine = 0;
#pragma unroll 4
    for (uint64_t t = t0; t < t1; ++t) {
        const uint64_t i0 = t * kPassTile + (uint64_t)threadIdx.x * 4u;
        uint32_t px[4];
        load4_stream(rgba, i0, n, aligned != 0, px);
        mine += (uint32_t)__builtin_popcount(kept_bits(px, i0, n, cutoff));
    }
    const unsigned long long total = block_sum(mine, s_part);
    if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

__global__ __launch_bounds__(kPassBlock) void k_alpha_scatter(const uint32_t *__restrict__ rgba, uint64_t n, uint32_t cutoff,
                                                                const unsigned long long *__restrict__ counts, uint32_t *__restrict__ out,
                                                                unsigned long long *__restrict__ n_kept, int aligned)
{
    __shared__ unsigned long long s_part[kPassWaves];
    __shared__ uint32_t s_wave[2][kPassWaves];               // wave totals, double-buffered: one barrier per tile
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    unsigned long long before = 0;
    for (uint32_t g = threadIdx.x; g < blockIdx.x; g += kPassBlock) before += counts[g];
    uint64_t base = block_sum(before, s_part);                  // this run's first output index
    if (blockIdx.x == gridDim.x - 1u && threadIdx.x == 0) *n_kept = base + counts[blockIdx.x];
    uint64_t t0, t1;
    tile_run((n + kPassTile - 1) / kPassTile, t0, t1);
    uint32_t nx[4] = {0u, 0u, 0u, 0u};
    if (t0 < t1) load4_stream(rgba, t0 * kPassTile + (uint64_t)threadIdx.x * 4u, n, aligned != 0, nx);
    uint32_t parity = 0;
    for (uint64_t t = t0; t < t1; ++t, parity ^= 1u) {
        const uint64_t i0 = t * kPassTile + (uint64_t)threadIdx.x * 4u;
        const uint32_t px[4] = {nx[0], nx[1], nx[2], nx[3]};
        if (t + 1 < t1) load4_stream(rgba, i0 + kPassTile, n, aligned != 0, nx);       // the next tile, in flight meanwhile
        const uint32_t m = kept_bits(px, i0, n, cutoff);
        const uint32_t c = (uint32_t)__builtin_popcount(m);
        uint32_t off = 0, tot = 0;
#pragma unroll
        for (uint32_t b = 0; b < 3; ++b) {
            const unsigned long long bal = __ballot((c >> b) & 1u);
            off += __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u)) << b;
            tot += (uint32_t)__builtin_popcountll(bal) << b;
        }
        if (lane == 0) s_wave[parity][wave] = tot;
        __syncthreads();
        uint32_t wbase = 0, ttot = 0;
#pragma unroll
        for (uint32_t w = 0; w < kPassWaves; ++w) {
            const uint32_t v = s_wave[parity][w];
            wbase += w < wave ? v : 0u;
            ttot += v;
        }
        uint64_t dst = base + wbase + off;
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if ((m >> q) & 1u) out[dst++] = px[q];
        base += ttot;
    }
}

// out[i] keeps its RGB and takes the alpha byte of rgba[i] (the routes of kmg_table.hip, whose kernels have no ALPHA switch)
__global__ __launch_bounds__(kPassBlock) void k_alpha_merge(const uint32_t *__restrict__ rgba, uint32_t *__restrict__ out, uint64_t n,
                                                              int aligned)
{
    const uint64_t stride = (uint64_t)gridDim.x * kPassTile;
    for (uint64_t i0 = (uint64_t)blockIdx.x * kPassTile + (uint64_t)threadIdx.x * 4u; i0 < n; i0 += stride) {
        uint32_t px[4], o[4];
        load4_stream(rgba, i0, n, aligned != 0, px);
        load4_stream(out, i0, n, aligned != 0, o);
#pragma unroll
        for (int q = 0; q < 4; ++q) o[q] = with_alpha<true>(o[q], px[q]);
        store4_stream(out, i0, n, aligned != 0, o);
    }
}

}  // namespace

hipError_t launch_alpha_merge(const uint32_t *rgba, uint32_t *out, uint64_t n, hipStream_t st)
{
    const int aligned = ((reinterpret_cast<uintptr_t>(rgba) & 15u) == 0 && (reinterpret_cast<uintptr_t>(out) & 15u) == 0) ? 1 : 0;
    hipLaunchKernelGGL(k_alpha_merge, dim3(alpha_compact_grid(n)), dim3(kPassBlock), 0, st, rgba, out, n, aligned);
    return hipGetLastError();
}

uint32_t alpha_compact_grid(uint64_t n) { return pass_grid((n + kPassTile - 1) / kPassTile); }

hipError_t launch_alpha_compact(const uint32_t *rgba, uint64_t n, uint32_t cutoff, uint32_t *out, unsigned long long *n_kept,
                                unsigned long long *counts, hipStream_t st)
{
    const uint32_t grid = alpha_compact_grid(n);
    const int aligned = ((reinterpret_cast<uintptr_t>(rgba) & 15u) == 0) ? 1 : 0;
    hipLaunchKernelGGL(k_alpha_count, dim3(grid), dim3(kPassBlock), 0, st, rgba, n, cutoff, counts, aligned);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_alpha_scatter, dim3(grid), dim3(kPassBlock), 0, st, rgba, n, cutoff, counts, out, n_kept, aligned);
    return hipGetLastError();
}

}  // namespace kmg
