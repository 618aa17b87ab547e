// kmg_apply_dev.h -- the per-pixel output pass at full resolution as one __device__ function: find_centroid + swap + lab_to_rgb
// (replace), or mix_colors.wgsl main_dither + lab_to_rgb (dither): the body of k_apply (kmg_kernels.hip), statement for statement,
// with the tiles a workgroup takes as arguments -- a grid stride over the tiles of ONE image there, one tile of the image the
// workgroup belongs to in k_batch_apply (kmg_batch_apply.hip).  No threshold map here: a batch gives images with
// a map their own per-image pass.  k_apply itself keeps its own text.  Calling this function from it (with the offsets type of
// kmg_kernels.h as a last template parameter) was built and timed against the parent build (DESIGN.md 4.20,
// profiles/r15_output_bodies_time.txt): all 36 instantiations came out 14 - 87 instructions shorter with 0 - 34 fewer VGPRs, the
// 8192^2 passes 0 - 4 % faster, bytes identical -- and one of 17 rows, a 256 x 256 image at k = 256 with the blue-noise map,
// 0.6 us (0.9 %) slower where the parent's own two turns differed by 0.1 us, which the acceptance rule set beforehand does not
// allow.  Only k (+1 sentinel) distinct output colours exist, so the Lab->sRGB8 conversion is done once per centroid on the host
// (pal[]).  c_bayer below is the one definition of the reference's matrix for the scan (k_apply reads it too).
//
// Compile with -ffp-contract=off: arithmetic must match kmg_math.h operation for operation.
#pragma once

#include "kmg_device.h"
#include "kmg_lloyd_dev.h"       // argmin_scan

namespace kmg {

__constant__ const float c_bayer[16] = {0, 8, 2, 10, 12, 4, 14, 6, 3, 11, 1, 9, 15, 7, 13, 5};

// Tiles first_tile, first_tile + tile_stride, ... of the image (rgba, w, n) by the calling workgroup; a tile is kBlock * PPT
// pixels.  row0: the image row of pixel 0 (the Bayer index).
// OutT (kmg_device.h): uint32_t writes pal[label] (RGBA8), uint8_t / uint16_t the index (the alpha cutoff in bits 8..15 of
// `aligned`)
// LDS (dynamic): [centroids kpad x 16 B][sRGB table 1 KiB][16 offsets]
template <int PPT, bool DITHER, bool CHUNKED, bool ALPHA, typename OutT>
__device__ __forceinline__ void apply_tiles(const uint32_t *__restrict__ rgba, uint32_t w, uint64_t n, uint32_t row0,
                                            const Centroid *__restrict__ cent, uint32_t k, const float *__restrict__ lut,
                                            const uint32_t *__restrict__ pal, float threshold, OutT *__restrict__ out, int aligned,
                                            uint64_t first_tile, uint64_t tile_stride)
{
    extern __shared__ float4 smem4[];
    const uint32_t kpad = (k + 3u) & ~3u;
    float4 *s_cent = smem4;
    float *s_lut = reinterpret_cast<float *>(smem4 + kpad);
    float *s_off = s_lut + 256;

    s_lut[threadIdx.x] = lut[threadIdx.x];
    stage_centroids(s_cent, cent, k, kpad);
    if (DITHER && threadIdx.x < 16) {
        // mix_colors.wgsl:21-27,70,72: threshold * (M[x%4 + 4*(y%4)] / 16 - 0.5)
        float iv = c_bayer[threadIdx.x] / 16.0f - 0.5f;
        s_off[threadIdx.x] = threshold * iv;
    }
    __syncthreads();

    constexpr int GROUPS = PPT / 4;
    constexpr uint64_t TILE = (uint64_t)kBlock * PPT;
    const uint64_t tiles = (n + TILE - 1) / TILE;
    for (uint64_t tile = first_tile; tile < tiles; tile += tile_stride) {
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
            uint32_t gx = 0, gy = 0;
            if (DITHER) {
                const uint32_t i32 = (uint32_t)i0[g];
                gy = i32 / w;
                gx = i32 - gy * w;
                gy += row0;
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int p = g * 4 + q;
                float L, a, b;
                px_to_lab(s_lut, px[q], L, a, b);
                if (DITHER) {
                    const float off = s_off[(gx & 3u) + ((gy & 3u) << 2)];
                    L = L + off; a = a + off; b = b + off;         // :72
                    gx += 1;
                    if (gx == w) { gx = 0; gy += 1; }
                }
                pt[p] = pixel_terms(L, a, b);
                if (DITHER) {
                    // :73 closest = vec3(10000.0): the running minimum starts at the sentinel's
                    // distance; index k selects the converted sentinel in pal[]
                    best[p] = cie94_key(pt[p], 10000.0f, 10000.0f, 10000.0f, chroma(10000.0f, 10000.0f));
                    idx[p] = k;
                } else {
                    best[p] = 1.0e10f;                             // find_centroid.wgsl:29-30
                    idx[p] = 0u;
                }
            }
        }
        argmin_scan<PPT, CHUNKED, DITHER>(pt, best, idx, s_cent, k, kpad);
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

}  // namespace kmg
