// kmg_diffuse_wide.hip -- KMG_MODE_DIFFUSE for the filters other than Floyd-Steinberg (kmg_diffusion in include/kmeans_hip.h:
// Sierra Lite, Atkinson, Burkes, Sierra-2, Sierra-3, Jarvis, Stucki).  The contract is Floyd-Steinberg's with
// S = sum W[dy][dx] e(x - dx, y - dy) over two columns to either side and two rows up, and floor((S + D/2) / D) for a divisor
// that need not be a power of two.  All of it is int32, so any schedule that respects the dependences gives the serial loop's bytes.
//
// Schedule.  As in kmg_diffuse.hip: one lane per row, a wave owns a chunk of 64 rows, chunks are drawn from a ticket counter and
// chunk t waits on chunk t - 1 only.  What differs:
//   SKEW    lane i works on column s - SKEW i at step s.  A filter that takes e(x + 2, y - 1) needs SKEW = 3 (critical path
//           W + 3 (H - 1) steps); one that reaches e(x + 1, y - 1) at the most runs at Floyd-Steinberg's 2.  R = SKEW - 1 is the
//           column offset at which the row above becomes available: lane i - 1 finished column x + R one step earlier.
//   rows    u1[j] / u2[j] hold e(x + R - 4 + j, y - 1) / (.., y - 2), j = 0 .. 4, unpacked.  Both shift by one per step.  The new
//           u1[4] is lane i - 1's last error, one __shfl_up as before.  The new u2[4] is e(x + R, y - 2): lane i - 1 is at column
//           x + R, and that row is ITS row above, so the value is the entry of its own window at its own column.  It keeps the
//           packed words of that window's newest R + 1 entries (pk[0] = its own column), and pk[0] rides on the same
//           distance-1 shuffle.  No shuffle by 2, no LDS round trip.
//   zeros   a lane outside its row (x < 0, x >= w, lane >= rows of the chunk) hands on 0, and the global rows are read as 0 past
//           the width, so every neighbour outside the image contributes 0 without a test in the sum.
//   weights the twelve weights, the rounding bias and the reciprocal of the divisor are wave-uniform kernel arguments.  With
//           u = S + D/2 + 4096 D (0 <= u < 2^19) floor((S + D/2) / D) = umulhi(u, ceil(2^32 / D)) - 4096 exactly: the reciprocal's
//           excess e = ceil(2^32 / D) D - 2^32 < D <= 48 and u e < 2^32.  No float anywhere.
//   hand-off erow holds two ring slots of TWO rows each (4 x w packed words): slot (parity + t) & 1 is what chunk t reads, row 0 =
//           the error of the row above the chunk, row 1 = of the row above that.  Lane 0 reads both from there (lane 1 gets its
//           row y - 2 from lane 0's window like every other lane).  A chunk writes its last row and the one before it; a chunk of
//           ONE row (the last of an image, or a band of one row) forwards the last row it was handed as the row before.  Both
//           stores precede the release; the progress word counts columns of the LAST row (the row before is SKEW columns ahead,
//           the forwarded row R + kBody).  The reader of body s0 needs s0 + kBody + R columns.
// Watchdog, tickets, heartbeats, the control block and the abandoned chunk are those of kmg_diffuse.hip (kmg_diffuse_dev.h).

#include "kmg_diffuse_dev.h"
#include "kmg_diffusion.h"

namespace kmg {

namespace {

__device__ __forceinline__ void unpack_err(uint2 v, int e[3])
{
    e[0] = (int)(int16_t)(v.x & 0xFFFFu); e[1] = (int)v.x >> 16; e[2] = (int)v.y;
}

template <int ROUTE, bool ALPHA, typename OutT, int SKEW>
__global__ __launch_bounds__(64) void k_diffuse_wide(const uint32_t *__restrict__ rgba, uint32_t w, uint32_t rows,
                                                     OutT *__restrict__ out, uint2 *__restrict__ erow, uint32_t parity,
                                                     DiffCtl *__restrict__ ctl, uint32_t *__restrict__ sticky, const Centroid *__restrict__ cent, uint32_t k,
                                                     const float *__restrict__ lut, const uint32_t *__restrict__ pal,
                                                     const void *__restrict__ colour_labels, const uint16_t *__restrict__ sub_table,
                                                     uint32_t cutoff, const DiffuseFilter f)
{
    constexpr int R = SKEW - 1;
    constexpr uint32_t kLdsWords = ROUTE == kDiffusePairs ? kPairsLds : ROUTE == kDiffuseCells ? kCellsLds : 4u * 3072u + 256u + 3072u;
    __shared__ __attribute__((aligned(16))) uint32_t s_lds[kLdsWords];
    const uint32_t lane = threadIdx.x;
    float4 *s_cent = nullptr;
    float *s_lut = nullptr;
    uint32_t *s_pal;
    if (ROUTE == kDiffusePairs) {
        const uint4 *src = reinterpret_cast<const uint4 *>(sub_table + kSubCells + kCells);
        uint4 *dst = reinterpret_cast<uint4 *>(s_lds);
        for (uint32_t i = lane; i < kCells / 4; i += 64) dst[i] = src[i];
        for (uint32_t i = lane; i < 128; i += 64) s_lds[kCells + i] = i < kPairDirs ? pair_dir_word(i) : 0u;
        s_pal = s_lds + kCells + 128;
    } else if (ROUTE == kDiffuseCells) {
        const uint4 *src = reinterpret_cast<const uint4 *>(sub_table + kSubCells);
        uint4 *dst = reinterpret_cast<uint4 *>(s_lds);
        for (uint32_t i = lane; i < kCells / 8; i += 64) dst[i] = src[i];
        s_pal = s_lds + kCells / 2;
    } else {
        s_cent = reinterpret_cast<float4 *>(s_lds);
        for (uint32_t i = lane; i < k; i += 64) { const Centroid c = cent[i]; s_cent[i] = make_float4(c.L, c.a, c.b, c.C); }
        s_lut = reinterpret_cast<float *>(s_lds + 4u * 3072u);
        for (uint32_t i = lane; i < 256; i += 64) s_lut[i] = lut[i];
        s_pal = s_lds + 4u * 3072u + 256u;
    }
    for (uint32_t i = lane; i < k; i += 64) s_pal[i] = pal[i] | 0xFF000000u;
    __syncthreads();

    const uint32_t n_chunks = (rows + 63u) / 64u;
    for (;;) {
        uint32_t t = 0;
        if (lane == 0) t = __hip_atomic_fetch_add(&ctl->ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        t = __builtin_amdgcn_readfirstlane(__shfl(t, 0));
        if (t >= n_chunks || timed_out(ctl)) return;
        const uint32_t y0 = t * 64u, nr = min(64u, rows - y0);
        const bool row_ok = lane < nr;
        const uint64_t row_base = (uint64_t)(y0 + (row_ok ? lane : 0u)) * w;
        const uint2 *e_in1 = erow + (size_t)((parity + t) & 1u) * 2u * w, *e_in2 = e_in1 + w;
        uint2 *e_out1 = erow + (size_t)((parity + t + 1u) & 1u) * 2u * w, *e_out2 = e_out1 + w;
        uint32_t known = t == 0 ? w : 0u;                            // chunk 0 reads the pending rows: complete
        uint32_t published = 0;
        int eL1[3] = {0, 0, 0}, eL2[3] = {0, 0, 0};                  // e(x - 1, y), e(x - 2, y)
        int u1[5][3], u2[5][3];
        uint2 pk[R + 1];
#pragma unroll
        for (int i = 0; i < 5; ++i)
#pragma unroll
            for (int c = 0; c < 3; ++c) u1[i][c] = u2[i][c] = 0;
#pragma unroll
        for (int q = 0; q <= R; ++q) pk[q] = make_uint2(0u, 0u);
        uint2 eo = make_uint2(0u, 0u);
        const int steps = (int)w + SKEW * ((int)nr - 1);
        bool abandoned = false;
        uint32_t beats = 0;
        heartbeat(ctl, t, beats);                                    // (the chunk has started)
        for (int s0 = 0; s0 < steps; s0 += kBody) {
            const uint32_t need = (uint32_t)min((long long)s0 + kBody + R, (long long)w);
            if (known < need && !wait_progress(ctl, sticky, t, need, known, beats)) { abandoned = true; break; }
            heartbeat(ctl, t, beats);
            // rows above for lane 0: columns s0 + R .. s0 + R + kBody - 1, one per lane of the first kBody lanes
            uint2 blk1 = make_uint2(0u, 0u), blk2 = make_uint2(0u, 0u);
            const bool blk_ok = lane < (uint32_t)kBody && s0 + R + (int)lane < (int)w;
            if (blk_ok) { blk1 = e_in1[s0 + R + lane]; blk2 = e_in2[s0 + R + lane]; }
            if (nr == 1u && blk_ok) e_out2[s0 + R + lane] = blk1;   // one row: the row it was handed is the next chunk's row before
            if (s0 == 0) {
                // columns 0 .. R - 1: the other lanes receive them before their column 0, lane 0 has no such steps
                uint2 p1 = make_uint2(0u, 0u), p2 = make_uint2(0u, 0u);
                if (lane < (uint32_t)R && lane < w) { p1 = e_in1[lane]; p2 = e_in2[lane]; }
                if (nr == 1u && lane < (uint32_t)R && lane < w) e_out2[lane] = p1;
#pragma unroll
                for (int m = 0; m < R; ++m) {
                    const uint2 a = make_uint2(__builtin_amdgcn_readlane(p1.x, m), __builtin_amdgcn_readlane(p1.y, m));
                    const uint2 b = make_uint2(__builtin_amdgcn_readlane(p2.x, m), __builtin_amdgcn_readlane(p2.y, m));
                    if (lane == 0) { unpack_err(a, u1[5 - R + m]); unpack_err(b, u2[5 - R + m]); pk[m + 1] = a; }
                }
            }
            const int xb = s0 - SKEW * (int)lane;                    // this lane's column at the body's first step
            uint32_t px[kBody];
#pragma unroll
            for (int j = 0; j < kBody; ++j) {
                const int x = xb + j;
                px[j] = (row_ok && x >= 0 && x < (int)w) ? rgba[row_base + (uint32_t)x] : 0u;
            }
            uint32_t ob[kBody];
            uint2 eb[kBody];
#pragma unroll
            for (int j = 0; j < kBody; ++j) {
                const int x = xb + j;
                uint2 up1, up2;
                up1.x = (uint32_t)__shfl_up((int)eo.x, 1);
                up1.y = (uint32_t)__shfl_up((int)eo.y, 1);
                up2.x = (uint32_t)__shfl_up((int)pk[0].x, 1);
                up2.y = (uint32_t)__shfl_up((int)pk[0].y, 1);
                const uint32_t b1x = __builtin_amdgcn_readlane(blk1.x, j), b1y = __builtin_amdgcn_readlane(blk1.y, j);
                const uint32_t b2x = __builtin_amdgcn_readlane(blk2.x, j), b2y = __builtin_amdgcn_readlane(blk2.y, j);
                if (lane == 0) { up1.x = b1x; up1.y = b1y; up2.x = b2x; up2.y = b2y; }
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int c = 0; c < 3; ++c) { u1[i][c] = u1[i + 1][c]; u2[i][c] = u2[i + 1][c]; }
                unpack_err(up1, u1[4]);
                unpack_err(up2, u2[4]);
#pragma unroll
                for (int q = 0; q < R; ++q) pk[q] = pk[q + 1];
                pk[R] = up1;
                if (x == 0) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) eL1[c] = eL2[c] = 0;
                }
                const bool act = row_ok && x >= 0 && x < (int)w;
                const uint32_t src = px[j];
                const bool keep = !ALPHA || (src >> 24) >= cutoff;
                int tq[3];
                uint32_t cpx = 0xFF000000u;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    // e(x - dx, y - dy) is u[4 - R - dx]; dx = -2 lies outside the window at SKEW 2, where its weights are 0
                    int S = __mul24(f.w[0], eL1[c]) + __mul24(f.w[1], eL2[c]);
#pragma unroll
                    for (int dx = -2; dx <= 2; ++dx) {
                        if (4 - R - dx > 4) continue;
                        S += __mul24(f.w[4 + dx], u1[4 - R - dx][c]) + __mul24(f.w[9 + dx], u2[4 - R - dx][c]);
                    }
                    const uint32_t u = (uint32_t)((keep ? S : 0) + (int)f.bias);
                    const int v = 16 * (int)((src >> (8 * c)) & 255u) + (int)__umulhi(u, f.magic) - 4096;
                    tq[c] = min(max(v, 0), 4080);
                    cpx |= (uint32_t)((tq[c] + 8) >> 4) << (8 * c);
                }
                const uint32_t lbl = diffuse_label<ROUTE>(cpx, s_lds, s_cent, s_lut, k, colour_labels, sub_table, act);
                const uint32_t o = s_pal[act && lbl < k ? lbl : 0u];
                int e[3];
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    e[c] = keep ? tq[c] - 16 * (int)((o >> (8 * c)) & 255u) : 0;
                    eL2[c] = eL1[c];
                    eL1[c] = e[c];
                }
                eo = act ? pack_err(e[0], e[1], e[2]) : make_uint2(0u, 0u);
                if constexpr (kIndexOut<OutT>) ob[j] = index_of<ALPHA>(act && lbl < k ? lbl : 0u, src, cutoff, k);
                else ob[j] = with_alpha<ALPHA>(o, src);
                eb[j] = eo;
            }
#pragma unroll
            for (int j = 0; j < kBody; ++j) {
                const int x = xb + j;
                if (row_ok && x >= 0 && x < (int)w) {
                    out[row_base + (uint32_t)x] = (OutT)ob[j];
                    if (lane == nr - 1u) e_out1[x] = eb[j];
                    if (lane + 2u == nr) e_out2[x] = eb[j];
                }
            }
            // publish the columns of the last row done so far (hand-off recipe: stores, drain, agent release, drain, relaxed store)
            const int done = min(max(s0 + kBody - SKEW * ((int)nr - 1), 0), (int)w);
            if ((uint32_t)done > published) {
                published = (uint32_t)done;
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                if (lane == 0)
                    __hip_atomic_store(&ctl->prog[t % kDiffuseRing], ((unsigned long long)(t + 1u) << 32) | published,
                                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        if (abandoned) {
            // the pass failed (the host reports it): no row of this chunk keeps a half-diffused value
            for (uint32_t r = 0; r < nr; ++r)
                for (uint32_t x = lane; x < w; x += 64) out[(uint64_t)(y0 + r) * w + x] = (OutT)0u;
            return;
        }
    }
}

// the kernel's arguments from kmg_diffusion.h's table
DiffuseFilter diffuse_filter(int filter)
{
    DiffuseFilter f{};
    const int32_t d = diffusion_table(filter, f.w);
    f.bias = (uint32_t)(d / 2 + 4096 * d);
    f.magic = (uint32_t)(((1ull << 32) + (uint64_t)d - 1u) / (uint64_t)d);
    f.skew = (f.w[2] || f.w[7]) ? 3 : 2;                              // a weight on e(x + 2, y - 1) or e(x + 2, y - 2)
    return f;
}

}  // namespace

hipError_t launch_diffuse_wide(int route, int filter, const uint32_t *rgba, uint32_t w, uint32_t rows, void *out, int format, void *erow,
                               uint32_t parity, void *ctl, uint32_t *sticky, const Centroid *cent, uint32_t k, const float *lut,
                               const uint32_t *pal, const void *colour_labels, const uint16_t *sub_table, hipStream_t st, uint32_t alpha_cutoff)
{
    const DiffuseFilter f = diffuse_filter(filter);
    const uint32_t grid = diffuse_grid(route, rows);
    bool launched = false;                                            // (stays false for a route or format that does not exist)
    with_value<kDiffuseScan, kDiffusePairs, kDiffuseCells>(route, [&](auto R) { with_bool(alpha_cutoff != 0, [&](auto A) {
        with_out_type(format, [&](auto t) { with_value<2, 3>(f.skew, [&](auto S) {
            using OutT = typename decltype(t)::type;
            hipLaunchKernelGGL((k_diffuse_wide<R(), A(), OutT, S()>), dim3(grid), dim3(64), 0, st, rgba, w, rows, static_cast<OutT *>(out),
                               (uint2 *)erow, parity, (DiffCtl *)ctl, sticky, cent, k, lut, pal, colour_labels, sub_table, alpha_cutoff, f);
            launched = true;
        }); });
    }); });
    return launched ? hipGetLastError() : hipErrorInvalidValue;
}

}  // namespace kmg
