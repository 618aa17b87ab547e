// kmg_clip.hip -- all frames of a clip through the delta passes in one launch chain (kmg_dev_frame_delta_clip, include/kmeans_hip.h;
// DESIGN.md 4.19).  The per-frame passes of kmg_sequence.hip (k_frame_delta) and kmg_hold.hip (k_frame_hold) stay as they are: they
// are what this file is compared against, byte for byte.
//
//   k_clip_cleared   frames x tiles, only with KMG_CLIP_FULL_ON_CLEAR: frame t has cleared > 0 exactly when some pixel has I_t == k and
//                    I_{t-1} != k (t = 0: the canvas in place of I_{t-1}) -- after any frame the canvas shows slot k where that
//                    frame's map does, whatever was held.  A streaming pass over the maps alone; one atomic OR per wave that has
//                    such a pixel.
//   k_clip_hold      one template over the index type and over exact / lossy, on the skeleton of kmg_pass.h.  A lane takes four
//                    consecutive pixels per tile, loads their canvas indices (and held sources) ONCE, and walks the frames of the
//                    launch itself: per frame it loads the source and the map, applies the rule of k_frame_hold (k_frame_delta)
//                    statement for statement and stores the delta group; the next frame's loads are in flight meanwhile.  The canvas
//                    and the held source are stored once, after the last frame, where some frame changed them.  A frame whose word
//                    of d_full is set writes its map, and re-anchors every pixel (canvas = I_t, held source = the frame).
//                    The records are per frame: a table of kClipFrames partial records in LDS, updated with LDS integer atomics by
//                    the lanes that have something to report, flushed once per workgroup with the global integer atomics of
//                    k_frame_hold.  A clip of more frames runs as several launches over the same pixels; the state passes through
//                    the canvas and the held source.
// An element outside the band reads as 0 in every buffer: held with D = 0 and equal indices, it adds nothing anywhere.

#include "kmg_pass.h"
#include "kmg_state.h"

namespace kmg {

namespace {

// frames per launch of k_clip_hold: 32 records of 40 bytes are 1.25 KiB of LDS, beside the decode table's 1 KiB
constexpr uint32_t kClipFrames = KMG_CLIP_FRAMES;

enum { cChanged = 0, cCleared = 1, cX0 = 2, cY0 = 3, cX1 = 4, cY1 = 5, cHeld = 6, cFields = 8 };
static_assert(kClipFrames * cFields == kPassBlock, "one lane per field of the table, at its set-up and at its flush");
enum { cvSrc = 1u, cvIndex = 2u, cvOut = 4u };          // ClipFrame::vec: which of the frame's pointers allow the vector access

// one frame of the clip, as the kernels read it from device memory
struct alignas(16) ClipFrame {
    const uint32_t *src;             // (NULL in an exact clip)
    const void *index;
    void *out;
    uint32_t tolerance;
    uint32_t vec;
};
static_assert(sizeof(ClipFrame) == 32, "ClipFrame layout");

template <typename T>
__global__ __launch_bounds__(kPassBlock) void k_clip_cleared(const ClipFrame *__restrict__ fr, uint32_t n_frames, const T *canvas,
                                                             uint32_t canvas_vec, uint64_t n, uint32_t k, uint32_t *d_full)
{
    uint64_t t0, t1;
    tile_run((n + kPassTile - 1) / kPassTile, t0, t1);
    for (uint32_t f = blockIdx.y; f < n_frames; f += gridDim.y) {
        const T *cur = static_cast<const T *>(fr[f].index);
        const bool cur_vec = (fr[f].vec & cvIndex) != 0;
        const T *prev = f ? static_cast<const T *>(fr[f - 1].index) : canvas;
        const bool prev_vec = f ? (fr[f - 1].vec & cvIndex) != 0 : canvas_vec != 0;
        bool hit = false;
        for (uint64_t t = t0; t < t1; ++t) {
            const uint64_t i0 = t * kPassTile + (uint64_t)threadIdx.x * 4u;
            uint32_t c[4], v[4];
            load4_index<T, false>(cur, i0, n, cur_vec, c);
            load4_index<T, false>(prev, i0, n, prev_vec, v);
#pragma unroll
            for (int j = 0; j < 4; ++j) hit |= c[j] == k && v[j] != k;
        }
        if (__ballot(hit) != 0ull && (threadIdx.x & 63u) == 0) atomicOr(d_full + f, 1u);
    }
}

// one lane's four pixels of one frame: source and frame index
struct ClipGroup { uint32_t s[4], c[4]; };

template <typename T, bool LOSSY>
__device__ __forceinline__ void clip_load(const ClipFrame &f, uint64_t i0, uint64_t n, ClipGroup &g)
{
    if (LOSSY) load4_stream(f.src, i0, n, (f.vec & cvSrc) != 0, g.s);
    else g.s[0] = g.s[1] = g.s[2] = g.s[3] = 0u;                       // (an exact clip has no sources)
    load4_index<T, true>(static_cast<const T *>(f.index), i0, n, (f.vec & cvIndex) != 0, g.c);
}

// frames [f0, f0 + nf) of the table, nf <= kClipFrames; info: the record of frame 0 of the table
template <typename T, bool LOSSY>
__global__ __launch_bounds__(kPassBlock) void k_clip_hold(const ClipFrame *__restrict__ fr, uint32_t f0, uint32_t nf, T *canvas, uint32_t *held,
                                                          uint64_t n, uint32_t width, uint32_t k, const float *__restrict__ lut,
                                                          uint32_t canvas_vec, uint32_t held_vec, uint32_t step_x, uint32_t step_y,
                                                          const uint32_t *__restrict__ full, unsigned long long *info)
{
    __shared__ float s_lut[256];
    __shared__ uint32_t s_rec[kClipFrames][cFields];
    __shared__ unsigned long long s_sse[kClipFrames];
    if (LOSSY) s_lut[threadIdx.x] = lut[threadIdx.x];
    {
        const uint32_t f = threadIdx.x % cFields;
        s_rec[threadIdx.x / cFields][f] = (f == cX0 || f == cY0) ? kFresh : 0u;
        if (threadIdx.x < kClipFrames) s_sse[threadIdx.x] = 0ull;
    }
    __syncthreads();

    uint64_t t0, t1;
    tile_run((n + kPassTile - 1) / kPassTile, t0, t1);
    if (t0 >= t1) return;                                              // (the whole workgroup: no barrier is left behind)

    uint64_t i0 = t0 * kPassTile + (uint64_t)threadIdx.x * 4u;
    // (x, y) of pixel i0: the one division of this lane
    uint32_t y = (uint32_t)(i0 / width), x = (uint32_t)(i0 - (uint64_t)y * width);
    for (uint64_t t = t0; t < t1; ++t) {
        uint32_t v[4], h[4] = {0u, 0u, 0u, 0u};
        load4_index<T, false>(canvas, i0, n, canvas_vec != 0, v);
        if (LOSSY) load4(held, i0, n, held_vec != 0, h);
        bool put_canvas = false, put_held = false;
        ClipGroup nx;
        clip_load<T, LOSSY>(fr[f0], i0, n, nx);
        for (uint32_t f = 0; f < nf; ++f) {
            const ClipGroup g = nx;
            const ClipFrame cf = fr[f0 + f];
            if (f + 1 < nf) clip_load<T, LOSSY>(fr[f0 + f + 1], i0, n, nx);                                // the next frame, in flight meanwhile
            const bool is_full = full != nullptr && full[f0 + f] != 0u;
            uint32_t out_d[4], ch_mask = 0, ncl = 0, n_held = 0;
            unsigned long long held_sse = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t s = g.s[j], c = g.c[j];
                bool hold = false;
                uint32_t D = 0;
                if (LOSSY) {
                    const bool holdable = v[j] != k && c != k;
                    if (holdable && ((s ^ h[j]) & 0x00FFFFFFu) != 0u) {    // equal bytes have equal q: D = 0 without a conversion
                        int32_t qs[3], qh[3];
                        px_to_q(s_lut, s, qs);
                        px_to_q(s_lut, h[j], qh);
                        const int32_t dL = qs[0] - qh[0], da = qs[1] - qh[1], db = qs[2] - qh[2];
                        D = (uint32_t)(dL * dL) + (uint32_t)(da * da) + (uint32_t)(db * db);               // < 2^29
                    }
                    hold = holdable && D <= cf.tolerance;
                }
                const bool differs = c != v[j];
                const bool ch = !hold && differs;
                n_held += (hold && differs) ? 1u : 0u;
                held_sse += (hold && differs) ? D : 0u;
                ncl += (ch && c == k) ? 1u : 0u;
                ch_mask |= ch ? 1u << j : 0u;
                out_d[j] = (ch || is_full) ? c : k;
                // the state after this frame; a full frame re-anchors every pixel
                const bool take = !hold || is_full;
                put_canvas |= take && differs;
                if (take) v[j] = c;
                if (LOSSY) {
                    put_held |= take && s != h[j];
                    if (take) h[j] = s;
                }
            }
            store4_index<T, true>(static_cast<T *>(cf.out), i0, n, (cf.vec & cvOut) != 0, out_d);
            if (ch_mask) {
                uint32_t bx0 = kFresh, by0 = kFresh, bx1 = 0, by1 = 0, xe = x, ye = y;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if ((ch_mask >> j) & 1u) {
                        bx0 = min(bx0, xe); bx1 = max(bx1, xe + 1u);
                        by0 = min(by0, ye); by1 = max(by1, ye + 1u);
                    }
                    if (++xe == width) { xe = 0; ++ye; }
                }
                atomicAdd(&s_rec[f][cChanged], (uint32_t)__builtin_popcount(ch_mask));
                if (ncl) atomicAdd(&s_rec[f][cCleared], ncl);
                atomicMin(&s_rec[f][cX0], bx0);
                atomicMin(&s_rec[f][cY0], by0);
                atomicMax(&s_rec[f][cX1], bx1);
                atomicMax(&s_rec[f][cY1], by1);
            }
            if (LOSSY && n_held) {
                atomicAdd(&s_rec[f][cHeld], n_held);
                if (held_sse) atomicAdd(&s_sse[f], held_sse);
            }
        }
        if (put_canvas) store4_index<T, false>(canvas, i0, n, canvas_vec != 0, v);
        if (LOSSY && put_held) store4(held, i0, n, held_vec != 0, h);
        // the same lane's pixels of the next tile
        i0 += kPassTile;
        const uint64_t xs = (uint64_t)x + step_x;
        y += step_y;
        if (xs >= width) { x = (uint32_t)(xs - width); ++y; } else x = (uint32_t)xs;
    }

    __syncthreads();
    // kmg_frame_hold of frame f0 + threadIdx.x / 8: changed, cleared (u64 sums), x0, y0 (minima), x1, y1 (maxima) as u32, held,
    // held_sse (u64 sums); a field this workgroup cannot move is left alone
    const uint32_t f = threadIdx.x / cFields, fld = threadIdx.x % cFields;
    if (f < nf) {
        unsigned long long *rec = info + (uint64_t)(f0 + f) * (sizeof(kmg_frame_hold) / 8u);
        uint32_t *box = reinterpret_cast<uint32_t *>(rec + 2);
        const uint32_t a = s_rec[f][fld];
        if (fld == cChanged || fld == cCleared) { if (a) atomicAdd(rec + fld, (unsigned long long)a); }
        else if (fld == cX0 || fld == cY0) { if (a != kFresh) atomicMin(box + (fld - cX0), a); }
        else if (fld == cX1 || fld == cY1) { if (a) atomicMax(box + (fld - cX0), a); }
        else if (fld == cHeld) { if (a) atomicAdd(rec + 4, (unsigned long long)a); }
        else if (s_sse[f]) atomicAdd(rec + 5, s_sse[f]);
    }
}

template <typename T>
int clip_typed(kmg_processor *p, uint32_t n_frames, const uint8_t *const *d_src, const void *const *d_index, void *d_canvas, uint8_t *d_held,
               uint64_t n, uint32_t width, uint32_t k, const uint32_t *tolerances, bool full_on_clear, void *const *d_out,
               kmg_frame_hold *d_info, uint32_t *d_full, uint32_t *launches, hipStream_t st)
{
    const bool lossy = tolerances != nullptr;
    // the vector accesses, buffer by buffer: an RGBA8 stream 16-byte aligned, an index stream for its own (u8: 4, u16: 8 bytes)
    const uintptr_t im = 4u * sizeof(T) - 1u;
    std::vector<ClipFrame> host(n_frames);
    for (uint32_t t = 0; t < n_frames; ++t) {
        ClipFrame &f = host[t];
        f.src = lossy ? reinterpret_cast<const uint32_t *>(d_src[t]) : nullptr;
        f.index = d_index[t];
        f.out = d_out[t];
        f.tolerance = lossy ? tolerances[t] : 0u;
        f.vec = ((lossy && (reinterpret_cast<uintptr_t>(d_src[t]) & 15u) == 0) ? cvSrc : 0u) |
                ((reinterpret_cast<uintptr_t>(d_index[t]) & im) == 0 ? cvIndex : 0u) | ((reinterpret_cast<uintptr_t>(d_out[t]) & im) == 0 ? cvOut : 0u);
    }
    // the table: one stream-ordered block, one copy; it goes back to the pool behind the last launch
    StreamBuf table;
    HIP_TRY(table.alloc(p, sizeof(ClipFrame) * (size_t)n_frames, st));
    HIP_TRY(upload_host_copy(table.ptr, host.data(), sizeof(ClipFrame) * (size_t)n_frames, st));
    const ClipFrame *fr = static_cast<const ClipFrame *>(table.ptr);
    const uint32_t canvas_vec = (reinterpret_cast<uintptr_t>(d_canvas) & im) == 0 ? 1u : 0u;
    const uint32_t held_vec = (reinterpret_cast<uintptr_t>(d_held) & 15u) == 0 ? 1u : 0u;
    const uint32_t grid = pass_grid((n + kPassTile - 1) / kPassTile);
    if (full_on_clear) {
        HIP_TRY(hipMemsetAsync(d_full, 0, sizeof(uint32_t) * (size_t)n_frames, st));
        hipLaunchKernelGGL((k_clip_cleared<T>), dim3(grid, std::min(n_frames, 4096u)), dim3(kPassBlock), 0, st, fr, n_frames,
                           static_cast<const T *>(d_canvas), canvas_vec, n, k, d_full);
        HIP_TRY(hipGetLastError());
        ++*launches;
    }
    unsigned long long *info = reinterpret_cast<unsigned long long *>(d_info);
    for (uint32_t f0 = 0; f0 < n_frames; f0 += kClipFrames) {
        const uint32_t nf = std::min(kClipFrames, n_frames - f0);
        with_bool(lossy, [&](auto L) {                                  // (an exact clip has no held source)
            hipLaunchKernelGGL((k_clip_hold<T, L()>), dim3(grid), dim3(kPassBlock), 0, st, fr, f0, nf, static_cast<T *>(d_canvas),
                               lossy ? reinterpret_cast<uint32_t *>(d_held) : nullptr, n, width, k, p->d_lut, canvas_vec, lossy ? held_vec : 0u,
                               kPassTile % width, kPassTile / width, full_on_clear ? d_full : nullptr, info);
        });
        HIP_TRY(hipGetLastError());
        ++*launches;
    }
    // an exact clip leaves the canvas equal to the last map everywhere: its held source is the last frame
    if (!lossy && d_held && d_src)
        HIP_TRY(hipMemcpyAsync(d_held, d_src[n_frames - 1], (size_t)n * 4, hipMemcpyDeviceToDevice, st));
    return KMG_OK;
}

}  // namespace

int frame_clip_impl(kmg_processor *p, uint32_t n_frames, const uint8_t *const *d_src_rgba, const void *const *d_index, void *d_canvas,
                    uint8_t *d_held_rgba, uint32_t width, uint32_t height, int format, uint32_t k, const uint32_t *tolerances, uint32_t flags,
                    void *const *d_out, kmg_frame_hold *d_info, uint32_t *d_full, uint32_t *launches, hipStream_t st)
{
    const bool lossy = tolerances != nullptr;
    // the refusals of kmg_dev_frame_delta_lossy in their order, the arrays standing where their entries will; then the clip's own
    KMG_TRY(check_index_band("frame_delta_clip", lossy, p, d_index ? d_canvas : nullptr, d_canvas, d_out ? d_canvas : nullptr,
                             lossy && d_src_rgba ? d_held_rgba : nullptr, lossy ? d_held_rgba : nullptr, d_info, width, height, 0, format, k));
    if (n_frames == 0) return fail(KMG_ERR_INVALID_ARGUMENT, "frame_delta_clip: the clip has no frames");
    const uintptr_t em = format == KMG_FORMAT_INDEX16 ? 1u : 0u;
    for (uint32_t t = 0; t < n_frames; ++t) {
        if (!d_index[t] || !d_out[t] || (lossy && !d_src_rgba[t])) return fail(KMG_ERR_INVALID_ARGUMENT, "frame_delta_clip: a pointer of frame %u is NULL", t);
        if ((reinterpret_cast<uintptr_t>(d_index[t]) | reinterpret_cast<uintptr_t>(d_out[t])) & em)
            return fail(KMG_ERR_INVALID_ARGUMENT, "frame %u: INDEX16 buffers must be 2-byte aligned", t);
        if (lossy && (reinterpret_cast<uintptr_t>(d_src_rgba[t]) & 3u)) return fail(KMG_ERR_INVALID_ARGUMENT, "frame %u: the source must be 4-byte aligned", t);
    }
    if (!lossy && d_held_rgba && d_src_rgba)
        for (uint32_t t = 0; t < n_frames; ++t)
            if (!d_src_rgba[t]) return fail(KMG_ERR_INVALID_ARGUMENT, "frame_delta_clip: a pointer of frame %u is NULL", t);
    if (flags & ~KMG_CLIP_FULL_ON_CLEAR) return fail(KMG_ERR_INVALID_ARGUMENT, "unknown flags %u", flags);
    const bool full_on_clear = (flags & KMG_CLIP_FULL_ON_CLEAR) != 0;
    if (full_on_clear && !d_full) return fail(KMG_ERR_INVALID_ARGUMENT, "KMG_CLIP_FULL_ON_CLEAR needs d_full");
    if (full_on_clear && (reinterpret_cast<uintptr_t>(d_full) & 3u)) return fail(KMG_ERR_INVALID_ARGUMENT, "d_full is not 4-byte aligned");
    const uint64_t n = (uint64_t)width * height;
    HIP_TRY(hipSetDevice(p->device));
    uint32_t none = 0;
    if (!launches) launches = &none;
    int rc = KMG_OK;                                                  // (check_index_band has refused every other format)
    with_index_type(format, [&](auto t) {
        rc = clip_typed<typename decltype(t)::type>(p, n_frames, d_src_rgba, d_index, d_canvas, d_held_rgba, n, width, k, tolerances, full_on_clear, d_out,
                                                    d_info, d_full, launches, st);
    });
    return rc;
}

}  // namespace kmg

extern "C" int kmg_dev_frame_delta_clip(kmg_processor *p, uint32_t n_frames, const uint8_t *const *d_src_rgba, const void *const *d_index,
                                        void *d_canvas, uint8_t *d_held_rgba, uint32_t width, uint32_t height, int format, uint32_t k,
                                        const uint32_t *tolerances, uint32_t flags, void *const *d_out, kmg_frame_hold *d_info,
                                        uint32_t *d_full, void *stream)
try {
    return frame_clip_impl(p, n_frames, d_src_rgba, d_index, d_canvas, d_held_rgba, width, height, format, k, tolerances, flags, d_out, d_info,
                           d_full, nullptr, S(stream));
}
KMG_ABI_CATCH
