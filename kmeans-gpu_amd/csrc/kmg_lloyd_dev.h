// kmg_lloyd_dev.h -- device helpers that the kernels of kmg_kernels.hip share with their batched versions in kmg_batch.hip: the
// arg-min scan over a centroid table in LDS (assign and output kernels) and the key helpers of the single-pick initialisation.
// Device code only; compile with -ffp-contract=off (kmg_math.h).
#pragma once

#include "kmg_device.h"
#include "kmg_table_dev.h"       // lane_value, wave_min, wave_max_u32_dpp

namespace kmg {

// ------------------------------------------------------------------------------------------
// Arg-min scan shared by the assign and the output kernels.
//
// The centroid table lives in LDS as (L, a, b, C) float4 entries and is read with ONE
// ds_read_b128 per centroid per wave (all lanes read the same address -> broadcast), so the
// centroid operands arrive in VGPRs.  (Scalar loads would be free, but on gfx950 a VALU
// instruction with an SGPR source issues at half rate -- tools/valu_rate.hip.)
//
// CHUNKED: centroids are visited four at a time; only the chunk minimum is compared against the
// running best (v_min3 + v_min + v_cmp + 2 v_cndmask per 4 pairs instead of 3 per pair) and the
// winning index inside the chunk is recovered afterwards by re-evaluating that one chunk.
// Strict '<' between chunk minima keeps the earliest chunk, the recovery takes the first entry
// that attains the minimum: exactly find_centroid.wgsl's "first minimum wins".
// The table is padded to a multiple of 4 with entries no pixel can be closest to.
// ------------------------------------------------------------------------------------------
constexpr uint32_t kNoChunk = 0xFFFFFFFFu;

// Near-tie repair (kmg_math.h): the scan orders by the key and remembers the second smallest key; a pixel whose
// second smallest key is within the tie threshold of the smallest is decided again by the LITERAL distance among
// the centroids inside the threshold, first minimum winning -- find_centroid.wgsl:32-41 / mix_colors.wgsl:73-80
// exactly.  SENTINEL (dither): the running minimum starts at the distance to vec3(10000.0), index k.
template <int PPT, bool CHUNKED, bool SENTINEL>
__device__ __forceinline__ void argmin_scan(const PixelTerms (&pt)[PPT], float (&best)[PPT],
                                            uint32_t (&idx)[PPT], const float4 *s_cent, uint32_t k,
                                            uint32_t kpad)
{
    float second[PPT];                                   // best <= second: the two smallest keys met so far
#pragma unroll
    for (int p = 0; p < PPT; ++p) second[p] = 3.0e38f;
    if (!CHUNKED) {
#pragma unroll 2
        for (uint32_t j = 0; j < k; ++j) {
            const float4 c = s_cent[j];
#pragma unroll
            for (int p = 0; p < PPT; ++p) {
                float d = cie94_key(pt[p], c.x, c.y, c.z, c.w);
                bool lt = d < best[p];
                if (kLiteralArgmin) second[p] = __builtin_amdgcn_fmed3f(d, best[p], second[p]);
                best[p] = lt ? d : best[p];
                idx[p] = lt ? j : idx[p];
            }
        }
    } else {
        uint32_t chunk[PPT];
#pragma unroll
        for (int p = 0; p < PPT; ++p) chunk[p] = kNoChunk;
        for (uint32_t j = 0; j < kpad; j += 4) {
            const float4 c0 = s_cent[j], c1 = s_cent[j + 1], c2 = s_cent[j + 2], c3 = s_cent[j + 3];
#pragma unroll
            for (int p = 0; p < PPT; ++p) {
                float d0 = cie94_key(pt[p], c0.x, c0.y, c0.z, c0.w);
                float d1 = cie94_key(pt[p], c1.x, c1.y, c1.z, c1.w);
                float d2 = cie94_key(pt[p], c2.x, c2.y, c2.z, c2.w);
                float d3 = cie94_key(pt[p], c3.x, c3.y, c3.z, c3.w);
                float m = fminf(fminf(fminf(d0, d1), d2), d3);
                bool lt = m < best[p];
                // second smallest chunk minimum; the other keys of the winning chunk are looked at below
                if (kLiteralArgmin) second[p] = __builtin_amdgcn_fmed3f(m, best[p], second[p]);
                best[p] = lt ? m : best[p];
                chunk[p] = lt ? j : chunk[p];
            }
        }
#pragma unroll
        for (int p = 0; p < PPT; ++p) {
            if (chunk[p] != kNoChunk) {
                uint32_t found = chunk[p] + 3;
                float d4[4];
#pragma unroll
                for (int q = 3; q >= 0; --q) {
                    const float4 c = s_cent[chunk[p] + q];
                    d4[q] = cie94_key(pt[p], c.x, c.y, c.z, c.w);
                    if (q < 3) found = (d4[q] <= best[p]) ? chunk[p] + q : found;
                }
                idx[p] = found;
                if (kLiteralArgmin) {
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        second[p] = fminf(second[p], chunk[p] + q == found ? 3.0e38f : d4[q]);
                }
            }
        }
    }
    if (kLiteralArgmin) {
        float thr[PPT];
        bool near_any = false;
#pragma unroll
        for (int p = 0; p < PPT; ++p) {
            thr[p] = tie_threshold(best[p]);
            near_any = near_any || second[p] <= thr[p];
        }
        if (__ballot(near_any)) {
            // One near-tie pixel at a time, the WAVE working on it: the pixel's terms go to every lane, lane l takes the
            // centroids l, l + 64, ... -- the literal distance where the key is inside the threshold, smallest index first --
            // and the wave reduces to (smallest distance, lowest index among equals) = what the reference's ordered scan with
            // strict `<` returns.  The cost follows the number of such pixels (a few per thousand): the loop this replaces
            // walked the whole table with all lanes for every wave that held one -- 40 % of the vector work of the kernel at
            // 4096^2, k = 16 (512 pixels per wave: nearly every wave), and on a small image the launch's duration (46 us at
            // k = 256 for the wave that met one; profiles/NOTES.md, round 4).
            const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
            for (int p = 0; p < PPT; ++p) {
                unsigned long long todo = __ballot(second[p] <= thr[p]);
                while (todo) {
                    const uint32_t src = (uint32_t)__builtin_ctzll(todo);
                    todo &= todo - 1ull;
                    PixelTerms q;
                    q.L = lane_value(pt[p].L, src); q.a = lane_value(pt[p].a, src); q.b = lane_value(pt[p].b, src);
                    q.C = lane_value(pt[p].C, src); q.wC = lane_value(pt[p].wC, src); q.wH = lane_value(pt[p].wH, src);
                    const float t = lane_value(thr[p], src);
                    float my_d = 3.0e38f;
                    uint32_t my_j = 0xFFFFFFFFu;
                    for (uint32_t j = lane; j < k; j += 64u) {
                        const float4 c = s_cent[j];
                        if (cie94_key(q, c.x, c.y, c.z, c.w) <= t) {
                            const float d = cie94_c(q.L, q.a, q.b, q.C, c.x, c.y, c.z, c.w);
                            if (d < my_d) { my_d = d; my_j = j; }
                        }
                    }
                    const float wd = wave_min(my_d);
                    const uint32_t wj = ~wave_max_u32_dpp(~(my_d == wd ? my_j : 0xFFFFFFFFu));
                    // (find_centroid.wgsl:29-30 / mix_colors.wgsl:73-75: what the scan starts from)
                    const float start = SENTINEL ? cie94_c(q.L, q.a, q.b, q.C, 10000.0f, 10000.0f, 10000.0f, chroma(10000.0f, 10000.0f)) : 100000.0f;
                    const uint32_t res = wd < start ? wj : (SENTINEL ? k : 0u);
                    if (lane == src) idx[p] = res;
                }
            }
        }
    }
}

// ---- farthest-point initialisation, single pick (k_init_pass<PICK> of kmg_kernels.hip, where the key is described) ----
__device__ __forceinline__ uint32_t init_key_index(unsigned long long kk)
{
    uint32_t index = 0;                                       // Candidate(0, 0.0) when every distance is 0
    if ((kk >> 32) != 0ull) {
        const uint32_t low = (uint32_t)kk;
        index = (low & ~15u) | (15u - (low & 15u));
    }
    return index;
}

// largest of n_slots keys, in thread 0 (s_key: kBlock / 64 words of LDS; ends with a barrier)
__device__ __forceinline__ unsigned long long init_max_slot(const unsigned long long *__restrict__ slots, uint32_t n_slots,
                                                            unsigned long long *s_key)
{
    unsigned long long m = 0ull;
    for (uint32_t q = threadIdx.x; q < n_slots; q += kBlock) { const unsigned long long v = slots[q]; m = v > m ? v : m; }
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_down(m, off, 64);
        m = o > m ? o : m;
    }
    if ((threadIdx.x & 63) == 0) s_key[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < kBlock / 64; ++w) m = s_key[w] > m ? s_key[w] : m;
    return m;
}

}  // namespace kmg
