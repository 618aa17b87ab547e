// kmg_local.hip -- colour-keyed delta frames (kmg_dev_frame_delta_colour / _colour_lossy, include/kmeans_hip.h): the
// delta passes of kmg_sequence.hip and kmg_hold.hip for frames that each have a palette of their own.  The canvas holds what is SHOWN,
// an RGBA8 word (0: nothing), and the comparison goes through the frame's palette.
//
//   k_frame_local    one template over the index type (u8 / u16) and the rule (exact / lossy), on the skeleton of kmg_pass.h, with
//                    k_frame_hold as its model.  The palette is staged once per workgroup in LDS as k + 1 words, entry k = 0; an
//                    index is clamped to k before the lookup, so none reads outside it.  A lane takes four consecutive pixels per
//                    tile: one 4- / 8-byte non-temporal load of the frame's indices, one 16-byte load of the shown words and --
//                    lossy -- one 16-byte non-temporal load of the source and one 16-byte load of the held source.  The delta map
//                    is stored for every group of four, the shown words and the held source only where a pixel of the group
//                    changes them.  Coordinates, box and reduction: as k_frame_hold.
// An element outside the band takes no part: the loads give it 0 everywhere, and P[0] is a colour, so it is masked by its position.

#include "kmg_pass.h"
#include "kmg_state.h"

namespace kmg {

namespace {

enum { lChanged = 0, lCleared = 1, lX0 = 2, lY0 = 3, lX1 = 4, lY1 = 5, lHeld = 6, lFields = 7 };

// one lane's four pixels of a tile: frame index, shown word, and -- lossy -- source and held source
struct LocalGroup { uint32_t c[4], v[4], s[4], h[4]; };

template <typename T, bool LOSSY>
__device__ __forceinline__ void local_load(const uint32_t *src, const uint32_t *held, const T *index, const uint32_t *shown, uint64_t i0,
                                           uint64_t n, bool aligned, LocalGroup &g)
{
    load4_index<T, true>(index, i0, n, aligned, g.c);
    load4(shown, i0, n, aligned, g.v);                                 // (read again by the next frame: not streamed)
    if (LOSSY) {
        load4_stream(src, i0, n, aligned, g.s);
        load4(held, i0, n, aligned, g.h);
    }
}

template <typename T, bool LOSSY>
__global__ __launch_bounds__(kPassBlock) void k_frame_local(const uint32_t *src, const T *index, const uint32_t *__restrict__ palette,
                                                            uint32_t *shown, uint32_t *held, T *__restrict__ delta, uint64_t n,
                                                            uint32_t width, uint32_t row0, uint32_t k, uint32_t tolerance,
                                                            const float *__restrict__ lut, int aligned, uint32_t step_x, uint32_t step_y,
                                                            unsigned long long *__restrict__ info)
{
    constexpr uint32_t kPal = sizeof(T) == 1 ? 256u : KMG_MAX_K + 1u;  // k + 1 words: INDEX8 has k <= 255
    constexpr int F = LOSSY ? lFields : lHeld;
    __shared__ uint32_t s_pal[kPal];
    __shared__ float s_lut[LOSSY ? 256 : 1];
    __shared__ uint32_t s_part[kPassWaves][lFields];
    __shared__ unsigned long long s_sse[kPassWaves];
    for (uint32_t i = threadIdx.x; i <= k; i += kPassBlock) s_pal[i] = i < k ? palette[i] : 0u;
    if (LOSSY) s_lut[threadIdx.x] = lut[threadIdx.x];
    __syncthreads();

    uint64_t t0, t1;
    tile_run((n + kPassTile - 1) / kPassTile, t0, t1);

    uint32_t changed = 0, cleared = 0, n_held = 0;
    uint32_t bx0 = kFresh, by0 = kFresh, bx1 = 0, by1 = 0;
    unsigned long long held_sse = 0;
    if (t0 < t1) {
        uint64_t i0 = t0 * kPassTile + (uint64_t)threadIdx.x * 4u;
        // (x, y) of pixel i0: the one division of this lane
        uint32_t y = (uint32_t)(i0 / width), x = (uint32_t)(i0 - (uint64_t)y * width);
        LocalGroup nx;
        local_load<T, LOSSY>(src, held, index, shown, i0, n, aligned != 0, nx);
        for (uint64_t t = t0; t < t1; ++t) {
            const LocalGroup g = nx;
            if (t + 1 < t1) local_load<T, LOSSY>(src, held, index, shown, i0 + kPassTile, n, aligned != 0, nx);   // the next tile, in flight meanwhile
            uint32_t out_d[4], out_v[4], out_h[4], ch_mask = 0;
            bool put_shown = false, put_held = false;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool inside = i0 + (uint32_t)j < n;
                const uint32_t c = min(g.c[j], k), v = g.v[j];
                const uint32_t p = s_pal[c];                           // (c <= k: inside the staged table)
                const bool differs = p != v;
                bool hold = false;
                if (LOSSY) {
                    const uint32_t s = g.s[j], h = g.h[j];
                    const bool holdable = v != 0u && p != 0u;
                    uint32_t D = 0;
                    if (holdable && ((s ^ h) & 0x00FFFFFFu) != 0u) {   // equal bytes have equal q: D = 0 without a conversion
                        int32_t qs[3], qh[3];
                        px_to_q(s_lut, s, qs);
                        px_to_q(s_lut, h, qh);
                        const int32_t dL = qs[0] - qh[0], da = qs[1] - qh[1], db = qs[2] - qh[2];
                        D = (uint32_t)(dL * dL) + (uint32_t)(da * da) + (uint32_t)(db * db);               // < 2^29
                    }
                    hold = holdable && D <= tolerance;
                    const bool counted = inside && hold && differs;
                    n_held += counted ? 1u : 0u;
                    held_sse += counted ? D : 0u;
                    out_h[j] = hold ? h : s;
                    put_held |= inside && !hold && s != h;
                }
                const bool ch = inside && !hold && differs;
                cleared += (ch && p == 0u) ? 1u : 0u;
                ch_mask |= ch ? 1u << j : 0u;
                out_d[j] = ch ? c : k;
                out_v[j] = hold ? v : p;
                put_shown |= ch;
            }
            store4_index<T, true>(delta, i0, n, aligned != 0, out_d);
            if (put_shown) store4(shown, i0, n, aligned != 0, out_v);
            if (LOSSY && put_held) store4(held, i0, n, aligned != 0, out_h);
            if (ch_mask) {
                changed += (uint32_t)__builtin_popcount(ch_mask);
                uint32_t xe = x, ye = y;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if ((ch_mask >> j) & 1u) {
                        const uint32_t yy = row0 + ye;
                        bx0 = min(bx0, xe); bx1 = max(bx1, xe + 1u);
                        by0 = min(by0, yy); by1 = max(by1, yy + 1u);
                    }
                    if (++xe == width) { xe = 0; ++ye; }
                }
            }
            // the same lane's pixels of the next tile
            i0 += kPassTile;
            const uint64_t xs = (uint64_t)x + step_x;
            y += step_y;
            if (xs >= width) { x = (uint32_t)(xs - width); ++y; } else x = (uint32_t)xs;
        }
    }

    const uint32_t v[lFields] = {changed, cleared, bx0, by0, bx1, by1, n_held};
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
    for (int f = 0; f < F; ++f) {
        uint32_t a = v[f];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const uint32_t b = __shfl_xor(a, o);
            a = (f == lX0 || f == lY0) ? min(a, b) : ((f == lX1 || f == lY1) ? max(a, b) : a + b);
        }
        if (lane == 0) s_part[wave][f] = a;
    }
    if (LOSSY) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) held_sse += __shfl_xor(held_sse, o);
        if (lane == 0) s_sse[wave] = held_sse;
    }
    __syncthreads();
    // kmg_frame_delta / kmg_frame_hold: changed, cleared (u64 sums), x0, y0 (minima), x1, y1 (maxima) as u32, then -- lossy -- held,
    // held_sse (u64 sums); a field this workgroup cannot move is left alone
    if (threadIdx.x < (uint32_t)F) {
        const uint32_t f = threadIdx.x;
        const bool is_min = f == lX0 || f == lY0, is_max = f == lX1 || f == lY1;
        uint32_t a = s_part[0][f];
#pragma unroll
        for (uint32_t w = 1; w < kPassWaves; ++w) a = is_min ? min(a, s_part[w][f]) : (is_max ? max(a, s_part[w][f]) : a + s_part[w][f]);
        uint32_t *box = reinterpret_cast<uint32_t *>(info + 2);
        if (is_min) { if (a != kFresh) atomicMin(box + (f - lX0), a); }
        else if (is_max) { if (a) atomicMax(box + (f - lX0), a); }
        else if (a) atomicAdd(info + (f == lHeld ? 4u : f), (unsigned long long)a);
    } else if (LOSSY && threadIdx.x == lFields) {
        unsigned long long a = s_sse[0];
#pragma unroll
        for (uint32_t w = 1; w < kPassWaves; ++w) a += s_sse[w];
        if (a) atomicAdd(info + 5, a);
    }
}

template <typename T, bool LOSSY>
hipError_t frame_local_typed(const void *src, const void *index, const void *palette, void *shown, void *held, void *delta, uint64_t n,
                             uint32_t width, uint32_t row0, uint32_t k, uint32_t tolerance, const float *lut, unsigned long long *info,
                             hipStream_t st)
{
    const uint32_t grid = pass_grid((n + kPassTile - 1) / kPassTile);
    // the vector accesses: the RGBA8 streams 16-byte aligned, the two index streams for their own (u8: 4, u16: 8 bytes)
    const uintptr_t im = 4u * sizeof(T) - 1u;
    const uintptr_t words = reinterpret_cast<uintptr_t>(shown) | (LOSSY ? reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(held) : 0u);
    const uintptr_t idx = reinterpret_cast<uintptr_t>(index) | reinterpret_cast<uintptr_t>(delta);
    const int aligned = ((words & 15u) == 0 && (idx & im) == 0) ? 1 : 0;
    hipLaunchKernelGGL((k_frame_local<T, LOSSY>), dim3(grid), dim3(kPassBlock), 0, st, static_cast<const uint32_t *>(src),
                       static_cast<const T *>(index), static_cast<const uint32_t *>(palette), static_cast<uint32_t *>(shown),
                       static_cast<uint32_t *>(held), static_cast<T *>(delta), n, width, row0, k, tolerance, lut, aligned, kPassTile % width,
                       kPassTile / width, info);
    return hipGetLastError();
}

}  // namespace

int frame_local_impl(kmg_processor *p, const uint8_t *d_src_rgba, const void *d_index, const uint8_t *d_palette_rgba, uint8_t *d_shown_rgba,
                     uint8_t *d_held_rgba, uint32_t width, uint32_t rows, uint32_t row0, int format, uint32_t k, bool lossy, uint32_t tolerance,
                     void *d_delta, void *d_info, hipStream_t st)
{
    const char *name = lossy ? "frame_delta_colour_lossy" : "frame_delta_colour";
    const int rc = check_index_band(name, lossy, p, d_index, d_shown_rgba, d_delta, d_src_rgba, d_held_rgba, d_info, width, rows, row0, format, k);
    if (rc != KMG_OK) return rc;
    if (!d_palette_rgba) return fail(KMG_ERR_INVALID_ARGUMENT, "%s: a pointer is NULL", name);
    if ((reinterpret_cast<uintptr_t>(d_palette_rgba) | reinterpret_cast<uintptr_t>(d_shown_rgba)) & 3u)
        return fail(KMG_ERR_INVALID_ARGUMENT, "the palette and the shown words must be 4-byte aligned");
    const uint64_t n = (uint64_t)width * rows;
    HIP_TRY(hipSetDevice(p->device));
    unsigned long long *info = reinterpret_cast<unsigned long long *>(d_info);
    hipError_t e = hipErrorInvalidValue;
    if (!lossy) { d_src_rgba = nullptr; d_held_rgba = nullptr; tolerance = 0u; }                // (the exact rule reads none of them)
    with_index_type(format, [&](auto t) { with_bool(lossy, [&](auto L) {
        e = frame_local_typed<typename decltype(t)::type, L()>(d_src_rgba, d_index, d_palette_rgba, d_shown_rgba, d_held_rgba, d_delta, n, width,
                                                               row0, k, tolerance, p->d_lut, info, st);
    }); });
    HIP_TRY(e);
    return KMG_OK;
}

}  // namespace kmg

extern "C" int kmg_dev_frame_delta_colour(kmg_processor *p, const void *d_index, const uint8_t *d_palette_rgba, uint8_t *d_shown_rgba,
                                          uint32_t width, uint32_t rows, uint32_t row0, int format, uint32_t k, void *d_delta,
                                          kmg_frame_delta *d_info, void *stream)
try {
    return frame_local_impl(p, nullptr, d_index, d_palette_rgba, d_shown_rgba, nullptr, width, rows, row0, format, k, false, 0u, d_delta, d_info,
                            S(stream));
}
KMG_ABI_CATCH

extern "C" int kmg_dev_frame_delta_colour_lossy(kmg_processor *p, const uint8_t *d_src_rgba, const void *d_index, const uint8_t *d_palette_rgba,
                                                uint8_t *d_shown_rgba, uint8_t *d_held_rgba, uint32_t width, uint32_t rows, uint32_t row0,
                                                int format, uint32_t k, uint32_t tolerance, void *d_delta, kmg_frame_hold *d_info, void *stream)
try {
    return frame_local_impl(p, d_src_rgba, d_index, d_palette_rgba, d_shown_rgba, d_held_rgba, width, rows, row0, format, k, true, tolerance,
                            d_delta, d_info, S(stream));
}
KMG_ABI_CATCH
