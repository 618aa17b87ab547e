// kmg_diffuse.hip -- KMG_MODE_DIFFUSE: Floyd-Steinberg error diffusion onto the palette (the contract is in
// include/kmeans_hip.h at kmg_reduce_mode).  All arithmetic of the diffusion is int32, the nearest colour is the
// replace pass's label of the quantised colour, so any schedule that respects the dependences gives the bytes of a serial loop.
//
// Schedule.  One lane per image row: a wave owns a CHUNK of 64 consecutive rows and at step s lane i works on column s - 2 i.
// Pixel (x, y) needs e(x - 1, y) (the lane's own previous step) and e(x - 1 .. x + 1, y - 1): lane i - 1 finished column x + 1 one
// step earlier, so the row above arrives by one __shfl_up per step and two older values stay in registers.  Lane 0 reads the last
// row of the chunk above from an error row in global memory, written by the wave that owns that chunk and published in batches of
// kBody columns.  A workgroup is one wave; it draws chunks from a ticket counter, and chunk t waits on chunk t - 1 only, which went
// to a workgroup that was already running: progress never depends on how many workgroups are resident or in which order they
// were dispatched.  The critical path of a W x H image is W + 2 (H - 1) steps plus one hand-off per chunk boundary.
//
// Safety on a shared device: every wait is bounded by s_memrealtime -- kSpinTicks without progress OF THE PASS.  A chunk's
// predecessor may itself be waiting (while the pipeline fills, chunk t waits for the t chunks before it), so every chunk keeps a
// heartbeat word that it bumps once per body while it computes and whenever it sees its own predecessor's heartbeat or progress
// change while it waits: a beat travels down the chain of waiting chunks, and a waiter's clock restarts on any beat.  Only a pass in
// which no chunk has moved for kSpinTicks gives up: the wave sets the timeout word (and the caller's sticky word), writes zeros over
// its rows and leaves, and every other wave leaves at its next poll.  Ticket, progress, heartbeat and timeout words live in the
// caller's per-call control block (diffuse_ctl_bytes()), zeroed before every launch.  No grid barrier, no wait on a later ticket.

#include "kmg_diffuse_dev.h"      // DiffCtl, heartbeat, wait_progress, timed_out, diffuse_label, pack_err

namespace kmg {

namespace {

// ALPHA (alpha mode, kmg_options.alpha_cutoff = cutoff): a pixel whose alpha byte is below the cutoff takes no part -- S = 0 (its
// own colour unmodified), e = 0 -- and every output word keeps its pixel's alpha byte.
// OutT (kmg_device.h): uint32_t writes the RGBA8 word, uint8_t / uint16_t the label (k for a pixel alpha mode drops)
template <int ROUTE, bool ALPHA, typename OutT>
__global__ __launch_bounds__(64) void k_diffuse(const uint32_t *__restrict__ rgba, uint32_t w, uint32_t rows,
                                                OutT *__restrict__ out, uint2 *__restrict__ erow, uint32_t parity,
                                                DiffCtl *__restrict__ ctl, uint32_t *__restrict__ sticky, const Centroid *__restrict__ cent, uint32_t k,
                                                const float *__restrict__ lut, const uint32_t *__restrict__ pal,
                                                const void *__restrict__ colour_labels, const uint16_t *__restrict__ sub_table,
                                                uint32_t cutoff)
{
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
        const uint2 *e_in = erow + (size_t)((parity + t) & 1u) * w;
        uint2 *e_out = erow + (size_t)((parity + t + 1u) & 1u) * w;
        uint32_t known = t == 0 ? w : 0u;                            // chunk 0 reads the pending row: complete
        uint32_t published = 0;
        int eL[3] = {0, 0, 0}, am1[3] = {0, 0, 0}, a0[3] = {0, 0, 0}, ap1[3] = {0, 0, 0};
        uint2 eo = make_uint2(0u, 0u);
        const int steps = (int)w + 2 * ((int)nr - 1);
        bool abandoned = false;
        uint32_t beats = 0;
        heartbeat(ctl, t, beats);                                    // (the chunk has started)
        for (int s0 = 0; s0 < steps; s0 += kBody) {
            const uint32_t need = (uint32_t)min((long long)s0 + kBody + 1, (long long)w);
            if (known < need && !wait_progress(ctl, sticky, t, need, known, beats)) { abandoned = true; break; }
            heartbeat(ctl, t, beats);
            // row above for lane 0: columns s0 + 1 .. s0 + kBody, one per lane of the first kBody lanes
            uint2 blk = make_uint2(0u, 0u);
            if (lane < (uint32_t)kBody && s0 + 1 + (int)lane < (int)w) blk = e_in[s0 + 1 + lane];
            if (s0 == 0 && lane == 0) {
                // e(0, y - 1): the other lanes receive it one step before their column 0, lane 0 has no such step
                const uint2 z = e_in[0];
                ap1[0] = (int)(int16_t)(z.x & 0xFFFFu); ap1[1] = (int)z.x >> 16; ap1[2] = (int)z.y;
            }
            const int xb = s0 - 2 * (int)lane;                       // this lane's column at the body's first step
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
                uint2 up;
                up.x = (uint32_t)__shfl_up((int)eo.x, 1);
                up.y = (uint32_t)__shfl_up((int)eo.y, 1);
                const uint32_t bx = __builtin_amdgcn_readlane(blk.x, j), by = __builtin_amdgcn_readlane(blk.y, j);
                if (lane == 0) { up.x = bx; up.y = by; }
                const bool in_w = x + 1 < (int)w;
                const int upv[3] = {(int)(int16_t)(up.x & 0xFFFFu), (int)up.x >> 16, (int)up.y};
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    am1[c] = x == 0 ? 0 : a0[c];
                    a0[c] = ap1[c];
                    ap1[c] = in_w ? upv[c] : 0;
                    if (x == 0) eL[c] = 0;
                }
                const bool act = row_ok && x >= 0 && x < (int)w;
                const uint32_t src = px[j];
                const bool keep = !ALPHA || (src >> 24) >= cutoff;
                int tq[3];
                uint32_t cpx = 0xFF000000u;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const int S = keep ? 7 * eL[c] + 3 * ap1[c] + 5 * a0[c] + am1[c] : 0;
                    const int v = 16 * (int)((src >> (8 * c)) & 255u) + ((S + 8) >> 4);
                    tq[c] = min(max(v, 0), 4080);
                    cpx |= (uint32_t)((tq[c] + 8) >> 4) << (8 * c);
                }
                const uint32_t lbl = diffuse_label<ROUTE>(cpx, s_lds, s_cent, s_lut, k, colour_labels, sub_table, act);
                const uint32_t o = s_pal[act && lbl < k ? lbl : 0u];
                int e[3];
#pragma unroll
                for (int c = 0; c < 3; ++c) { e[c] = keep ? tq[c] - 16 * (int)((o >> (8 * c)) & 255u) : 0; eL[c] = e[c]; }
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
                    if (lane == nr - 1u) e_out[x] = eb[j];
                }
            }
            // publish the columns of the last row done so far (hand-off recipe: stores, drain, agent release, drain, relaxed store)
            const int done = min(max(s0 + kBody - 2 * ((int)nr - 1), 0), (int)w);
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

}  // namespace

size_t diffuse_ctl_bytes() { return sizeof(DiffCtl); }

uint32_t diffuse_grid(int route, uint32_t rows)
{
    // workgroups per CU the static LDS admits (pair table 130 KiB: one; summaries 76 KiB: two; scan <= 61 KiB: two)
    const uint32_t per_cu = route == kDiffusePairs ? 1u : 2u;
    const uint32_t cap = device_info().cus * per_cu;
    const uint32_t chunks = (rows + 63u) / 64u;
    uint32_t g = chunks < cap ? chunks : cap;
    if (g > kDiffuseRing - 1u) g = kDiffuseRing - 1u;         // a progress slot is reused only after its reader has finished
    return g ? g : 1u;
}

// The error rows in `erow`: two ring slots, each the rows a chunk hands to the next -- one row of w packed words (8 bytes a
// column) for Floyd-Steinberg, two for the other filters (kmg_diffuse_wide.hip).  The buffer is sized for the larger.
size_t diffuse_erow_bytes(uint32_t w) { return 2 * 16 * (size_t)w; }

size_t diffuse_slot_bytes(int filter, uint32_t w) { return (filter == KMG_DIFFUSION_FLOYD_STEINBERG ? 8u : 16u) * (size_t)w; }

hipError_t launch_diffuse(int route, int filter, const uint32_t *rgba, uint32_t w, uint32_t rows, void *out, int format, void *erow,
                          uint32_t parity, void *ctl, uint32_t *sticky, const Centroid *cent, uint32_t k, const float *lut,
                          const uint32_t *pal, const void *colour_labels, const uint16_t *sub_table, hipStream_t st, uint32_t alpha_cutoff)
{
    if (filter != KMG_DIFFUSION_FLOYD_STEINBERG)
        return launch_diffuse_wide(route, filter, rgba, w, rows, out, format, erow, parity, ctl, sticky, cent, k, lut, pal, colour_labels,
                                   sub_table, st, alpha_cutoff);
    const uint32_t grid = diffuse_grid(route, rows);
    bool launched = false;                                            // (stays false for a route or format that does not exist)
    with_value<kDiffuseScan, kDiffusePairs, kDiffuseCells>(route, [&](auto R) { with_bool(alpha_cutoff != 0, [&](auto A) {
        with_out_type(format, [&](auto t) {
            using OutT = typename decltype(t)::type;
            hipLaunchKernelGGL((k_diffuse<R(), A(), OutT>), dim3(grid), dim3(64), 0, st, rgba, w, rows, static_cast<OutT *>(out), (uint2 *)erow,
                               parity, (DiffCtl *)ctl, sticky, cent, k, lut, pal, colour_labels, sub_table, alpha_cutoff);
            launched = true;
        });
    }); });
    return launched ? hipGetLastError() : hipErrorInvalidValue;
}

}  // namespace kmg
