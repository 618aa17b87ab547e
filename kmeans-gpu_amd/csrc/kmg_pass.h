// kmg_pass.h -- what the bounded-grid streaming passes share: k_alpha_count / _scatter / _merge (kmg_alpha.hip),
// k_error_stats (kmg_error.hip), k_frame_delta (kmg_sequence.hip), k_frame_hold (kmg_hold.hip).
//
// Such a pass walks an image once and leaves a few exact integers in a device record:
//   grid       at most kPassMaxGrid workgroups of kPassBlock threads (pass_grid), each over one contiguous run of tiles (tile_run);
//              a tile is one 16-byte or four-pixel group per lane (kPassTile pixels where a lane takes four)
//   loads      vector loads where the pointers allow, per element with bounds otherwise; the kernel has the next tile's loads in
//              flight during the current tile's arithmetic
//   reduction  accumulators stay in registers, are reduced per wave with cross-lane operations, across the waves through LDS, and
//              leave the workgroup as one integer atomic per field that has something to say: no float atomics, no waits between
//              workgroups.  Each kernel spells its own out: a shared form of it, and of the row cursor and box of the two delta
//              passes, was measured 1 to 3 % slower in three of them (profiles/NOTES.md) and is not here.
// Everything here is inlined.
#pragma once

#include "kmg_device.h"

namespace kmg {

constexpr uint32_t kPassBlock = 256;                    // 4 waves
constexpr uint32_t kPassWaves = kPassBlock / 64;
constexpr uint32_t kPassTile = kPassBlock * 4;          // 4 consecutive pixels per lane
constexpr uint32_t kPassMaxGrid = 2048;                 // cdna_hip_programming.md Guideline 11: grid-stride beyond ~2048
constexpr uint32_t kFresh = 0xFFFFFFFFu;                // a minimum nothing has moved yet

inline uint32_t pass_grid(uint64_t tiles) { return (uint32_t)(tiles < kPassMaxGrid ? (tiles ? tiles : 1) : kPassMaxGrid); }

// tiles [t0, t1) of this workgroup's contiguous run (empty for the last workgroups where the tiles do not go round)
__device__ __forceinline__ void tile_run(uint64_t tiles, uint64_t &t0, uint64_t &t1)
{
    const uint64_t per = (tiles + gridDim.x - 1) / gridDim.x;
    t0 = min((uint64_t)blockIdx.x * per, tiles);
    t1 = min(t0 + per, tiles);
}

// the sum of v over the workgroup, in every lane (s_part: kPassWaves words of LDS)
__device__ __forceinline__ unsigned long long block_sum(unsigned long long v, unsigned long long *s_part)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & 63u) == 0) s_part[threadIdx.x >> 6] = v;
    __syncthreads();
    unsigned long long s = 0;
#pragma unroll
    for (uint32_t w = 0; w < kPassWaves; ++w) s += s_part[w];
    return s;
}

// q of an sRGB8 colour: the fixed-point grid of the Lab terms, (rint(64 L), rint(64 a), rint(64 b)) of the device's own rgb_to_lab
__device__ __forceinline__ void px_to_q(const float *s_lut, uint32_t px, int32_t q[3])
{
    float L, a, b;
    px_to_lab(s_lut, px, L, a, b);
    q[0] = (int32_t)rintf(L * 64.0f);
    q[1] = (int32_t)rintf(a * 64.0f);
    q[2] = (int32_t)rintf(b * 64.0f);
}

// four consecutive indices as words: one 4-byte (u8) or 8-byte (u16) load, or one load per index in range
template <typename T, bool NT>
__device__ __forceinline__ void load4_index(const T *p, uint64_t i0, uint64_t n, bool aligned, uint32_t v[4])
{
    if (aligned && i0 + 4 <= n) {
        if (sizeof(T) == 1) {
            const uint32_t *q = reinterpret_cast<const uint32_t *>(p + i0);
            const uint32_t w = NT ? __builtin_nontemporal_load(q) : *q;
            v[0] = w & 255u; v[1] = (w >> 8) & 255u; v[2] = (w >> 16) & 255u; v[3] = w >> 24;
        } else {
            const u32x2 *q = reinterpret_cast<const u32x2 *>(p + i0);
            const u32x2 w = NT ? __builtin_nontemporal_load(q) : *q;
            v[0] = w.x & 0xFFFFu; v[1] = w.x >> 16; v[2] = w.y & 0xFFFFu; v[3] = w.y >> 16;
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = (i0 + j < n) ? (uint32_t)p[i0 + j] : 0u;
    }
}

}  // namespace kmg
