// kmg_dither_map.hip -- KMG_MODE_DITHER with a threshold map on the scan route (include/kmeans_hip.h at kmg_dither_map; DESIGN.md
// 4.20): k_apply_map, the dither body of k_apply (kmg_kernels.hip) with the 16 offsets of the reference's matrix replaced by a
// table of mw x mh offsets t * v.  k_apply keeps its own text and its instantiations their code; the default choice never comes here.
//
// Compile with -ffp-contract=off: arithmetic must match kmg_math.h operation for operation.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kmg_internal.h"
#include "kmg_kernels.h"
#include "kmg_device.h"
#include "kmg_lloyd_dev.h"       // argmin_scan

namespace kmg {

namespace {

constexpr int kMapPPT = 8;       // pixels per thread: k_apply's on large images (kAssignPPT)

// OutT (kmg_device.h): uint32_t writes pal[label] (RGBA8), uint8_t / uint16_t the index (the alpha cutoff in bits 8..15 of
// `aligned`)
// LDS (dynamic): [centroids kpad x 16 B][sRGB table 1 KiB][mw x mh offsets]
// The offsets lie row-major, so the four pixels of a lane read consecutive dwords and the lanes of a wave read at stride four:
// four lanes per bank on a map 32 or 64 wide (MI355X: 32 banks per group of 32 lanes for a dword read), 8 LDS cycles instead of 2
// for each of the 4 reads of a group of pixels -- against k x 4 centroid reads of the scan behind it.
template <int PPT, bool CHUNKED, bool ALPHA, typename OutT>
__global__ __launch_bounds__(kBlock) void k_apply_map(const uint32_t *__restrict__ rgba, uint32_t w, uint64_t n, uint32_t row0,
                                                      const Centroid *__restrict__ cent, uint32_t k, const float *__restrict__ lut,
                                                      const uint32_t *__restrict__ pal, float t, DitherMapDev map,
                                                      OutT *__restrict__ out, int aligned)
{
    extern __shared__ float4 smem4[];
    const uint32_t kpad = (k + 3u) & ~3u;
    float4 *s_cent = smem4;
    float *s_lut = reinterpret_cast<float *>(smem4 + kpad);
    float *s_off = s_lut + 256;

    s_lut[threadIdx.x] = lut[threadIdx.x];
    stage_centroids(s_cent, cent, k, kpad);
    const uint32_t entries = (map.xmask + 1u) * (map.ymask + 1u);
    for (uint32_t i = threadIdx.x; i < entries; i += kBlock) s_off[i] = t * map.v[i];    // off = t * v, one rounding
    __syncthreads();

    constexpr int GROUPS = PPT / 4;
    constexpr uint64_t TILE = (uint64_t)kBlock * PPT;
    const uint64_t tiles = (n + TILE - 1) / TILE;
    for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        uint64_t i0[GROUPS];
        PixelTerms pt[PPT];
        float best[PPT];
        uint32_t idx[PPT];
        uint32_t src_a[ALPHA ? PPT : 1];                             // alpha mode: the source words' alpha bytes
#pragma unroll
        for (int g = 0; g < GROUPS; ++g) {
            i0[g] = tile * TILE + (uint64_t)g * (kBlock * 4) + (uint64_t)threadIdx.x * 4;
            uint32_t px[4];
            load4(rgba, i0[g], n, kIndexOut<OutT> ? (aligned & 1) != 0 : aligned != 0, px);
            if (ALPHA) {
#pragma unroll
                for (int q = 0; q < 4; ++q) src_a[g * 4 + q] = px[q];
            }
            // image coordinates of the group's first pixel (n < 2^32): one 32-bit divide per 4 pixels
            const uint32_t i32 = (uint32_t)i0[g];
            uint32_t gy = i32 / w;
            uint32_t gx = i32 - gy * w;
            gy += row0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int p = g * 4 + q;
                float L, a, b;
                px_to_lab(s_lut, px[q], L, a, b);
                const float off = s_off[(gx & map.xmask) + ((gy & map.ymask) << map.xshift)];
                L = L + off; a = a + off; b = b + off;             // mix_colors.wgsl:72
                gx += 1;
                if (gx == w) { gx = 0; gy += 1; }
                pt[p] = pixel_terms(L, a, b);
                // :73 closest = vec3(10000.0): the running minimum starts at the sentinel's distance; index k selects the
                // converted sentinel in pal[]
                best[p] = cie94_key(pt[p], 10000.0f, 10000.0f, 10000.0f, chroma(10000.0f, 10000.0f));
                idx[p] = k;
            }
        }
        argmin_scan<PPT, CHUNKED, true>(pt, best, idx, s_cent, k, kpad);
#pragma unroll
        for (int g = 0; g < GROUPS; ++g) {
            uint32_t o[4];
            if constexpr (kIndexOut<OutT>) {
#pragma unroll
                for (int q = 0; q < 4; ++q) o[q] = index_of<ALPHA>(idx[g * 4 + q], src_a[ALPHA ? g * 4 + q : 0], ((uint32_t)aligned >> 8) & 255u, k);
                store4_index<OutT, false>(out, i0[g], n, (aligned & 1) != 0, o);
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q) o[q] = with_alpha<ALPHA>(pal[idx[g * 4 + q]], src_a[ALPHA ? g * 4 + q : 0]);
                store4(out, i0[g], n, aligned != 0, o);
            }
        }
    }
}

}  // namespace

size_t apply_map_lds_bytes(uint32_t k, uint32_t map_entries)
{
    return sizeof(float4) * ((k + 3u) & ~3u) + (256 + (size_t)map_entries) * sizeof(float);
}

// the grid is capped at kApplyMapGridCap workgroups of kBlock * kMapPPT pixels: from kApplyMapGridCap * 2048 + 1 pixels on a
// workgroup walks a second tile
constexpr uint32_t kApplyMapGridCap = 2048;

hipError_t launch_apply_map(const uint32_t *rgba, uint32_t w, uint32_t rows, uint32_t row0, const Centroid *cent, uint32_t k, const float *lut,
                            const uint32_t *pal, float t, DitherMapDev map, void *out, int format, hipStream_t st, uint32_t alpha_cutoff)
{
    const uint64_t n = (uint64_t)w * rows;
    const uint64_t tiles = (n + (uint64_t)kBlock * kMapPPT - 1) / ((uint64_t)kBlock * kMapPPT);
    const uint32_t grid = (uint32_t)(tiles < kApplyMapGridCap ? (tiles ? tiles : 1) : kApplyMapGridCap);
    const bool chunked = k >= 32;
    // 48 KiB of centroids at KMG_MAX_K and 16 KiB of a 64 x 64 map are above the 64 KiB every device has: gfx950 gives a
    // workgroup up to 160 KiB
    const size_t lds = apply_map_lds_bytes(k, dither_map_entries(map));
    if (lds > device_info().lds_max) return hipErrorInvalidValue;
    const bool known = with_out_type(format, [&](auto ot) {
        using OutT = typename decltype(ot)::type;
        const int flags = output_flags<OutT>(rgba, out, alpha_cutoff);
        with_bool(chunked, [&](auto C) { with_bool(alpha_cutoff != 0, [&](auto A) {
            hipLaunchKernelGGL((k_apply_map<kMapPPT, C(), A(), OutT>), dim3(grid), dim3(kBlock), lds, st, rgba, w, n, row0, cent, k, lut,
                               kIndexOut<OutT> ? nullptr : pal, t, map, static_cast<OutT *>(out), flags);
        }); });
    });
    return known ? hipGetLastError() : hipErrorInvalidValue;
}

}  // namespace kmg
