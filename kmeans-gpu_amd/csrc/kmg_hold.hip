// kmg_hold.hip -- lossy delta frames (kmg_dev_frame_delta_lossy, include/kmeans_hip.h): the delta pass of
// kmg_sequence.hip with a second per-pixel state, the held source, and a tolerance on the integer Lab grid of kmg_error.hip.
//
//   k_frame_hold     one template over the index type (u8 / u16), on the skeleton of kmg_pass.h.  A lane takes four consecutive
//                    pixels per tile: one 16-byte non-temporal load of the source, one 16-byte load of the held source, one 4- /
//                    8-byte load of the frame's indices and of the canvas.  The decode table is staged once per workgroup in LDS.
//                    A pixel whose R, G, B bytes equal its held word's has D = 0 without a conversion; a pixel that cannot be
//                    held (slot k on either side) needs no D at all.  The delta map is stored for every group of four, the
//                    canvas and the held source only where a pixel of the group changes them.  Coordinates: one division per lane
//                    and launch, every further tile adds the tile's (columns, rows) step (k_frame_delta).  Seven u32 fields and
//                    the u64 held_sse are reduced as kmg_pass.h says: at most 8 x 2048 atomics per launch.
// An element outside the band reads as 0 in all four buffers: held with D = 0 and equal indices, it adds nothing anywhere.

#include "kmg_pass.h"
#include "kmg_state.h"

namespace kmg {

namespace {

// n < 2^32 pixels are at most 2^22 tiles; a full grid gives a workgroup at most 2048 of them, a lane 8192 pixels: the counts are
// 32-bit, held_sse (up to 347 973 309 per pixel) is 64-bit throughout.
enum { hChanged = 0, hCleared = 1, hX0 = 2, hY0 = 3, hX1 = 4, hY1 = 5, hHeld = 6, hFields = 7 };

// one lane's four pixels of a tile: source, held source, frame index, canvas index
struct HoldGroup { uint32_t s[4], h[4], c[4], v[4]; };

template <typename T>
__device__ __forceinline__ void hold_load(const uint32_t *src, const uint32_t *held, const T *index, const T *canvas, uint64_t i0, uint64_t n,
                                          bool aligned, HoldGroup &g)
{
    load4_stream(src, i0, n, aligned, g.s);
    load4(held, i0, n, aligned, g.h);
    load4_index<T, true>(index, i0, n, aligned, g.c);
    load4_index<T, false>(canvas, i0, n, aligned, g.v);
}

template <typename T>
__global__ __launch_bounds__(kPassBlock) void k_frame_hold(const uint32_t *src, const T *index, T *canvas, uint32_t *held,
                                                           T *__restrict__ delta, uint64_t n, uint32_t width, uint32_t row0, uint32_t k,
                                                           uint32_t tolerance, const float *__restrict__ lut, int aligned, uint32_t step_x,
                                                           uint32_t step_y, unsigned long long *__restrict__ info)
{
    __shared__ float s_lut[256];
    __shared__ uint32_t s_part[kPassWaves][hFields];
    __shared__ unsigned long long s_sse[kPassWaves];
    s_lut[threadIdx.x] = lut[threadIdx.x];
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
        HoldGroup nx;
        hold_load<T>(src, held, index, canvas, i0, n, aligned != 0, nx);
        for (uint64_t t = t0; t < t1; ++t) {
            const HoldGroup g = nx;
            if (t + 1 < t1) hold_load<T>(src, held, index, canvas, i0 + kPassTile, n, aligned != 0, nx);   // the next tile, in flight meanwhile
            uint32_t out_d[4], out_c[4], out_h[4], ch_mask = 0;
            bool put_canvas = false, put_held = false;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t s = g.s[j], h = g.h[j], c = g.c[j], v = g.v[j];
                const bool holdable = v != k && c != k;
                uint32_t D = 0;
                if (holdable && ((s ^ h) & 0x00FFFFFFu) != 0u) {    // equal bytes have equal q: D = 0 without a conversion
                    int32_t qs[3], qh[3];
                    px_to_q(s_lut, s, qs);
                    px_to_q(s_lut, h, qh);
                    const int32_t dL = qs[0] - qh[0], da = qs[1] - qh[1], db = qs[2] - qh[2];
                    D = (uint32_t)(dL * dL) + (uint32_t)(da * da) + (uint32_t)(db * db);                   // < 2^29
                }
                const bool hold = holdable && D <= tolerance;
                const bool differs = c != v;
                const bool ch = !hold && differs;
                n_held += (hold && differs) ? 1u : 0u;
                held_sse += (hold && differs) ? D : 0u;
                cleared += (ch && c == k) ? 1u : 0u;
                ch_mask |= ch ? 1u << j : 0u;
                out_d[j] = ch ? c : k;
                out_c[j] = hold ? v : c;
                out_h[j] = hold ? h : s;
                put_canvas |= ch;
                put_held |= !hold && s != h;
            }
            store4_index<T, true>(delta, i0, n, aligned != 0, out_d);
            if (put_canvas) store4_index<T, false>(canvas, i0, n, aligned != 0, out_c);
            if (put_held) store4(held, i0, n, aligned != 0, out_h);
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

    const uint32_t v[hFields] = {changed, cleared, bx0, by0, bx1, by1, n_held};
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
    for (int f = 0; f < hFields; ++f) {
        uint32_t a = v[f];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const uint32_t b = __shfl_xor(a, o);
            a = (f == hX0 || f == hY0) ? min(a, b) : ((f == hX1 || f == hY1) ? max(a, b) : a + b);
        }
        if (lane == 0) s_part[wave][f] = a;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) held_sse += __shfl_xor(held_sse, o);
    if (lane == 0) s_sse[wave] = held_sse;
    __syncthreads();
    // kmg_frame_hold: changed, cleared (u64 sums), x0, y0 (minima), x1, y1 (maxima) as u32, held, held_sse (u64 sums); a field this
    // workgroup cannot move is left alone
    if (threadIdx.x < hFields) {
        const uint32_t f = threadIdx.x;
        const bool is_min = f == hX0 || f == hY0, is_max = f == hX1 || f == hY1;
        uint32_t a = s_part[0][f];
#pragma unroll
        for (uint32_t w = 1; w < kPassWaves; ++w) a = is_min ? min(a, s_part[w][f]) : (is_max ? max(a, s_part[w][f]) : a + s_part[w][f]);
        uint32_t *box = reinterpret_cast<uint32_t *>(info + 2);
        if (is_min) { if (a != kFresh) atomicMin(box + (f - hX0), a); }
        else if (is_max) { if (a) atomicMax(box + (f - hX0), a); }
        else if (a) atomicAdd(info + (f == hHeld ? 4u : f), (unsigned long long)a);
    } else if (threadIdx.x == hFields) {
        unsigned long long a = s_sse[0];
#pragma unroll
        for (uint32_t w = 1; w < kPassWaves; ++w) a += s_sse[w];
        if (a) atomicAdd(info + 5, a);
    }
}

template <typename T>
hipError_t frame_hold_typed(const void *src, const void *index, void *canvas, void *held, void *delta, uint64_t n, uint32_t width,
                            uint32_t row0, uint32_t k, uint32_t tolerance, const float *lut, unsigned long long *info, hipStream_t st)
{
    const uint32_t grid = pass_grid((n + kPassTile - 1) / kPassTile);
    // the vector accesses: the two RGBA8 streams 16-byte aligned, the three index streams for their own (u8: 4, u16: 8 bytes)
    const uintptr_t im = 4u * sizeof(T) - 1u;
    const uintptr_t words = reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(held);
    const uintptr_t idx = reinterpret_cast<uintptr_t>(index) | reinterpret_cast<uintptr_t>(canvas) | reinterpret_cast<uintptr_t>(delta);
    const int aligned = ((words & 15u) == 0 && (idx & im) == 0) ? 1 : 0;
    hipLaunchKernelGGL((k_frame_hold<T>), dim3(grid), dim3(kPassBlock), 0, st, static_cast<const uint32_t *>(src), static_cast<const T *>(index),
                       static_cast<T *>(canvas), static_cast<uint32_t *>(held), static_cast<T *>(delta), n, width, row0, k, tolerance, lut,
                       aligned, kPassTile % width, kPassTile / width, info);
    return hipGetLastError();
}

}  // namespace

int frame_hold_impl(kmg_processor *p, const uint8_t *d_src_rgba, const void *d_index, void *d_canvas, uint8_t *d_held_rgba, uint32_t width,
                    uint32_t rows, uint32_t row0, int format, uint32_t k, uint32_t tolerance, void *d_delta, kmg_frame_hold *d_info,
                    hipStream_t st)
{
    static_assert(sizeof(kmg_frame_hold) == 48, "kmg_frame_hold is 48 bytes");
    const int rc = check_index_band("frame_delta_lossy", true, p, d_index, d_canvas, d_delta, d_src_rgba, d_held_rgba, d_info, width, rows, row0,
                                    format, k);
    if (rc != KMG_OK) return rc;
    const uint64_t n = (uint64_t)width * rows;
    HIP_TRY(hipSetDevice(p->device));
    unsigned long long *info = reinterpret_cast<unsigned long long *>(d_info);
    hipError_t e = hipErrorInvalidValue;
    with_index_type(format, [&](auto t) {
        e = frame_hold_typed<typename decltype(t)::type>(d_src_rgba, d_index, d_canvas, d_held_rgba, d_delta, n, width, row0, k, tolerance, p->d_lut, info, st);
    });
    HIP_TRY(e);
    return KMG_OK;
}

}  // namespace kmg

extern "C" int kmg_dev_frame_delta_lossy(kmg_processor *p, const uint8_t *d_src_rgba, const void *d_index, void *d_canvas,
                                         uint8_t *d_held_rgba, uint32_t width, uint32_t rows, uint32_t row0, int format, uint32_t k,
                                         uint32_t tolerance, void *d_delta, kmg_frame_hold *d_info, void *stream)
try {
    return frame_hold_impl(p, d_src_rgba, d_index, d_canvas, d_held_rgba, width, rows, row0, format, k, tolerance, d_delta, d_info, S(stream));
}
KMG_ABI_CATCH
