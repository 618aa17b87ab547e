// kmg_sequence.hip -- frame sequences (include/kmeans_hip.h at kmg_sequence): one palette for many frames, and
// index maps as delta frames.
//
//   k_frame_delta    one template over the index type (u8 / u16), on the skeleton of kmg_pass.h.  The band is one flat run of
//                    width x rows elements in each of its three buffers.  A lane takes 16 bytes of each per tile -- 16 or 8
//                    consecutive elements: one 16-byte load of the frame's indices and of the canvas, one 16-byte store of the
//                    delta map and, where the chunk changed at all, of the canvas.  The chunks are laid out from the 16-byte
//                    boundary below the pointers, so the first and the last chunk of a band may be partial: those go element by
//                    element, as every chunk does when the three pointers do not share one offset within 16 bytes.  A changed
//                    chunk that lies within one row gets its box from the first and last set bit of its change mask, one that
//                    crosses a row end walks its elements; (x, y) costs one division per lane and launch, every further tile adds
//                    the tile's (columns, rows) step.  Six u32 fields are reduced as kmg_pass.h says.
//   kmg_sequence     host object: the working sequence W (one device block, grown geometrically), the palette step on it, and
//                    the frame output -- one apply plan, the frame buffers, the canvas and its held source (lossy frames:
//                    kmg_hold.hip) in one block.  kmg_sequence_output_frames takes a whole clip: the maps of its frames from the
//                    batched output launch (kmg_batch_apply.hip), the delta maps from one launch chain (kmg_clip.hip).

#include <initializer_list>
#include <utility>

#include "kmg_batch_layout.h"
#include "kmg_pass.h"
#include "kmg_state.h"

namespace kmg {

namespace {

// tiles of kPassBlock 16-byte chunks that cover the flat elements [-shift, n)
template <typename T>
__host__ __device__ constexpr uint64_t delta_tiles(uint64_t n, uint32_t shift)
{
    return ((n + shift + 16 / sizeof(T) - 1) / (16 / sizeof(T)) + kPassBlock - 1) / kPassBlock;
}

// one lane's 16 bytes of the frame's indices and of the canvas
struct DeltaChunk { uint32_t c[4], v[4]; };

// chunk `lo .. lo + E` of the flat band [0, n): 16-byte loads when it lies inside and the pointers allow, else per element
// (an element outside the band reads as 0 on both sides: unchanged)
template <typename T>
__device__ __forceinline__ void delta_load(const T *index, const T *canvas, int64_t lo, uint64_t n, bool vec, DeltaChunk &d)
{
    constexpr int E = 16 / sizeof(T), EPW = 4 / sizeof(T), BITS = 8 * sizeof(T);
    if (vec && lo >= 0 && (uint64_t)lo + E <= n) {
        const u32x4 c = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(index + lo));
        const u32x4 v = *reinterpret_cast<const u32x4 *>(canvas + lo);
        d.c[0] = c.x; d.c[1] = c.y; d.c[2] = c.z; d.c[3] = c.w;
        d.v[0] = v.x; d.v[1] = v.y; d.v[2] = v.z; d.v[3] = v.w;
    } else {
#pragma unroll
        for (int w = 0; w < 4; ++w) { d.c[w] = 0u; d.v[w] = 0u; }
#pragma unroll
        for (int j = 0; j < E; ++j) {
            const int64_t i = lo + j;
            if (i >= 0 && (uint64_t)i < n) {
                d.c[j / EPW] |= (uint32_t)index[i] << (BITS * (j % EPW));
                d.v[j / EPW] |= (uint32_t)canvas[i] << (BITS * (j % EPW));
            }
        }
    }
}

template <typename T>
__global__ __launch_bounds__(kPassBlock) void k_frame_delta(const T *index, T *canvas, T *__restrict__ delta, uint64_t n, uint32_t width,
                                                            uint32_t row0, uint32_t k, uint32_t shift, int vec, uint32_t step_x,
                                                            uint32_t step_y, unsigned long long *__restrict__ info)
{
    constexpr int E = 16 / sizeof(T), EPW = 4 / sizeof(T), BITS = 8 * sizeof(T);
    constexpr uint32_t MASK = (1u << BITS) - 1u;
    __shared__ uint32_t s_part[kPassWaves][6];

    // chunk c covers the flat elements [c E - shift, (c + 1) E - shift); tiles of kPassBlock chunks
    uint64_t t0, t1;
    tile_run(delta_tiles<T>(n, shift), t0, t1);

    uint32_t changed = 0, cleared = 0, bx0 = kFresh, by0 = kFresh, bx1 = 0, by1 = 0;
    if (t0 < t1) {
        int64_t lo = (int64_t)((t0 * kPassBlock + threadIdx.x) * E) - (int64_t)shift;
        // (x, y) of element `lo`: the one division of this lane (lo < 0, the partial first chunk, lies in the rows above the band)
        int64_t y = lo >= 0 ? (int64_t)((uint64_t)lo / width) : -(int64_t)(((uint64_t)(-lo) + width - 1) / width);
        uint32_t x = (uint32_t)(lo - y * (int64_t)width);
        DeltaChunk nx;
        delta_load<T>(index, canvas, lo, n, vec != 0, nx);
        for (uint64_t t = t0; t < t1; ++t) {
            const DeltaChunk d = nx;
            if (t + 1 < t1) delta_load<T>(index, canvas, lo + (int64_t)kPassBlock * E, n, vec != 0, nx);   // the next tile, in flight meanwhile
            uint32_t out[4] = {0u, 0u, 0u, 0u}, mask = 0, ncl = 0;
#pragma unroll
            for (int j = 0; j < E; ++j) {
                const uint32_t c = (d.c[j / EPW] >> (BITS * (j % EPW))) & MASK, v = (d.v[j / EPW] >> (BITS * (j % EPW))) & MASK;
                const bool ch = c != v;
                mask |= ch ? 1u << j : 0u;
                ncl += (ch && c == k) ? 1u : 0u;
                out[j / EPW] |= (ch ? c : k) << (BITS * (j % EPW));
            }
            if (vec && lo >= 0 && (uint64_t)lo + E <= n) {
                const u32x4 q = {out[0], out[1], out[2], out[3]};
                __builtin_nontemporal_store(q, reinterpret_cast<u32x4 *>(delta + lo));
                if (mask) *reinterpret_cast<u32x4 *>(canvas + lo) = u32x4{d.c[0], d.c[1], d.c[2], d.c[3]};   // (unchanged: canvas == index already)
            } else {
#pragma unroll
                for (int j = 0; j < E; ++j) {
                    const int64_t i = lo + j;
                    if (i >= 0 && (uint64_t)i < n) {
                        delta[i] = (T)((out[j / EPW] >> (BITS * (j % EPW))) & MASK);
                        if ((mask >> j) & 1u) canvas[i] = (T)((d.c[j / EPW] >> (BITS * (j % EPW))) & MASK);
                    }
                }
            }
            if (mask) {
                changed += (uint32_t)__builtin_popcount(mask);
                cleared += ncl;
                if ((uint64_t)x + E <= width) {                 // within one row (then lo >= 0)
                    const uint32_t yy = row0 + (uint32_t)y;
                    bx0 = min(bx0, x + (uint32_t)__builtin_ctz(mask));
                    bx1 = max(bx1, x + 32u - (uint32_t)__builtin_clz(mask));
                    by0 = min(by0, yy);
                    by1 = max(by1, yy + 1u);
                } else {
                    uint32_t xe = x;
                    int64_t ye = y;
#pragma unroll
                    for (int j = 0; j < E; ++j) {
                        if ((mask >> j) & 1u) {
                            const uint32_t yy = row0 + (uint32_t)ye;
                            bx0 = min(bx0, xe); bx1 = max(bx1, xe + 1u);
                            by0 = min(by0, yy); by1 = max(by1, yy + 1u);
                        }
                        if (++xe == width) { xe = 0; ++ye; }
                    }
                }
            }
            // the same lane's chunk of the next tile
            lo += (int64_t)kPassBlock * E;
            const uint64_t xs = (uint64_t)x + step_x;
            y += step_y;
            if (xs >= width) { x = (uint32_t)(xs - width); ++y; } else x = (uint32_t)xs;
        }
    }

    uint32_t v[6] = {changed, cleared, bx0, by0, bx1, by1};
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
    for (int f = 0; f < 6; ++f) {
        uint32_t a = v[f];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const uint32_t b = __shfl_xor(a, o);
            a = f < 2 ? a + b : (f < 4 ? min(a, b) : max(a, b));
        }
        if (lane == 0) s_part[wave][f] = a;
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        const uint32_t f = threadIdx.x;
        uint32_t a = s_part[0][f];
#pragma unroll
        for (uint32_t w = 1; w < kPassWaves; ++w) a = f < 2 ? a + s_part[w][f] : (f < 4 ? min(a, s_part[w][f]) : max(a, s_part[w][f]));
        // kmg_frame_delta: two u64 sums, then x0, y0 (minima), x1, y1 (maxima) as u32; a field this workgroup cannot move is left alone
        uint32_t *box = reinterpret_cast<uint32_t *>(info + 2);
        if (f < 2) { if (a) atomicAdd(info + f, (unsigned long long)a); }
        else if (f < 4) { if (a != kFresh) atomicMin(box + (f - 2), a); }
        else if (a) atomicMax(box + (f - 2), a);
    }
}

template <typename T>
hipError_t frame_delta_typed(const void *index, void *canvas, void *delta, uint64_t n, uint32_t width, uint32_t row0, uint32_t k,
                             unsigned long long *info, hipStream_t st)
{
    constexpr uint32_t E = 16 / sizeof(T);
    const uintptr_t a = reinterpret_cast<uintptr_t>(index) & 15u;
    const int vec = (a == (reinterpret_cast<uintptr_t>(canvas) & 15u) && a == (reinterpret_cast<uintptr_t>(delta) & 15u)) ? 1 : 0;
    const uint32_t shift = vec ? (uint32_t)(a / sizeof(T)) : 0u;
    const uint32_t grid = pass_grid(delta_tiles<T>(n, shift)), tile_elems = kPassBlock * E;
    hipLaunchKernelGGL((k_frame_delta<T>), dim3(grid), dim3(kPassBlock), 0, st, static_cast<const T *>(index), static_cast<T *>(canvas),
                       static_cast<T *>(delta), n, width, row0, k, shift, vec, tile_elems % width, tile_elems / width, info);
    return hipGetLastError();
}

int delta_needs_index() { return fail(KMG_ERR_INVALID_ARGUMENT, "a delta frame needs an index format (INDEX8 / INDEX16), not RGBA8"); }

int frame_delta_impl(kmg_processor *p, const void *d_index, void *d_canvas, uint32_t width, uint32_t rows, uint32_t row0, int format,
                     uint32_t k, void *d_delta, kmg_frame_delta *d_info, hipStream_t st)
{
    static_assert(sizeof(kmg_frame_delta) == 32, "kmg_frame_delta is 32 bytes");
    KMG_TRY(check_index_band("frame_delta", false, p, d_index, d_canvas, d_delta, nullptr, nullptr, d_info, width, rows, row0, format, k));
    const uint64_t n = (uint64_t)width * rows;
    HIP_TRY(hipSetDevice(p->device));
    unsigned long long *info = reinterpret_cast<unsigned long long *>(d_info);
    hipError_t e = hipErrorInvalidValue;
    with_index_type(format, [&](auto t) { e = frame_delta_typed<typename decltype(t)::type>(d_index, d_canvas, d_delta, n, width, row0, k, info, st); });
    HIP_TRY(e);
    return KMG_OK;
}

}  // namespace

int check_index_band(const char *name, bool lossy, const kmg_processor *p, const void *d_index, const void *d_canvas, const void *d_delta,
                     const void *d_src, const void *d_held, const void *d_info, uint32_t width, uint32_t rows, uint32_t row0, int format,
                     uint32_t k)
{
    if (format == KMG_FORMAT_RGBA8) return delta_needs_index();
    KMG_TRY(check_format(format));
    if (k == 0 || k > KMG_MAX_K) return fail(KMG_ERR_INVALID_ARGUMENT, "k = %u: 1 .. %u", k, KMG_MAX_K);
    KMG_TRY(check_index8_room(format == KMG_FORMAT_INDEX8, "k", k, true));
    if (!p || !d_index || !d_canvas || !d_delta || !d_info || (lossy && (!d_src || !d_held)))
        return fail(KMG_ERR_INVALID_ARGUMENT, "%s: a pointer is NULL", name);
    if (width == 0 || rows == 0) return fail(KMG_ERR_INVALID_ARGUMENT, "%s: the band has zero width or no rows", name);
    if ((uint64_t)width * rows > 0xFFFFFFFFull) return fail(KMG_ERR_UNSUPPORTED, "band has more than 2^32-1 pixels");
    if ((uint64_t)row0 + rows > 0xFFFFFFFFull) return fail(KMG_ERR_UNSUPPORTED, "row0 + rows exceeds 2^32-1");
    if (format == KMG_FORMAT_INDEX16 &&
        ((reinterpret_cast<uintptr_t>(d_index) | reinterpret_cast<uintptr_t>(d_canvas) | reinterpret_cast<uintptr_t>(d_delta)) & 1u))
        return fail(KMG_ERR_INVALID_ARGUMENT, "INDEX16 buffers must be 2-byte aligned");
    if (lossy && ((reinterpret_cast<uintptr_t>(d_src) | reinterpret_cast<uintptr_t>(d_held)) & 3u))
        return fail(KMG_ERR_INVALID_ARGUMENT, "the source and the held source must be 4-byte aligned");
    if (reinterpret_cast<uintptr_t>(d_info) & 7u) return fail(KMG_ERR_INVALID_ARGUMENT, "the %s record is not 8-byte aligned", lossy ? "hold" : "delta");
    return KMG_OK;
}

}  // namespace kmg

extern "C" int kmg_dev_frame_delta(kmg_processor *p, const void *d_index, void *d_canvas, uint32_t width, uint32_t rows, uint32_t row0,
                                   int format, uint32_t k, void *d_delta, kmg_frame_delta *d_info, void *stream)
try {
    return frame_delta_impl(p, d_index, d_canvas, width, rows, row0, format, k, d_delta, d_info, S(stream));
}
KMG_ABI_CATCH

// ---------------------------------------------------------------------------------------------
// the sequence object
// ---------------------------------------------------------------------------------------------
struct kmg_sequence {
    kmg_processor *p = nullptr;
    StreamGuard sg;                  // the sequence's own stream: host frames, the palette step, the frame output
    // W: the kept pixels of every frame added so far, in order (one block of the processor, grown geometrically)
    void *w_blk = nullptr;
    size_t w_cap = 0;                // bytes
    uint64_t n = 0;                  // |W| in pixels
    uint64_t frames = 0;
    uint32_t sw0 = 0, sh0 = 0;       // the first frame after its shrink
    bool first_whole = false;        // ... and every pixel of it was kept
    // the open output (kmg_sequence_output_begin), or plan == NULL
    kmg_apply_plan *plan = nullptr;
    uint32_t k = 0, width = 0, height = 0;
    int mode = 0, format = KMG_FORMAT_RGBA8;
    void *o_blk = nullptr;           // frame | map | canvas | delta map | held source | record
    size_t o_cap = 0;
    uint8_t *d_frame = nullptr, *d_map = nullptr, *d_canvas = nullptr, *d_delta = nullptr;
    // index formats: the held source of the canvas (kmg_dev_frame_delta_lossy).  After an exact frame it IS that frame, so the two
    // buffers swap instead of a copy.
    uint8_t *d_held = nullptr;
    kmg_frame_hold *d_info = nullptr;    // (an exact frame uses its first 32 bytes: a kmg_frame_delta)
    // an output with per-frame palettes (kmg_sequence_output_begin_local): no plan; the block is frame | map | delta map | shown |
    // held source | palette | record, and the canvas is what is SHOWN, an RGBA8 word per pixel (kmg_local.hip)
    bool local = false, have_prev = false;
    uint32_t local_flags = 0;
    int local_filter = 0;               // kmg_processor_set_diffusion when the per-frame output was opened
    DitherPtr local_dither;             // kmg_processor_set_dither[_custom] likewise (null: the default)
    uint8_t *d_shown = nullptr, *d_pal = nullptr;
    std::vector<float> prev_c4;      // C_{t-1}: where a warm frame's Lloyd loop starts
    std::vector<float> c4;           // the open output's centroids (shared palette): what a clip's batched output launch takes
};

namespace {

// ends the open output: the plan and the frame block go back to the processor (the sequence's stream is drained first)
void output_end(kmg_sequence *s)
{
    if (!s->plan && !s->o_blk) return;
    (void)hipSetDevice(s->p->device);
    (void)hipStreamSynchronize(s->sg.st);
    if (s->plan) kmg_apply_plan_destroy(s->plan, 0);
    s->plan = nullptr;
    block_give(s->p, s->o_blk, s->o_cap);
    s->o_blk = nullptr;
    s->o_cap = 0;
    s->local = s->have_prev = false;
}

// room for `extra` more pixels behind W: a new block of at least twice the size, then a device-to-device copy of what is there
int reserve(kmg_sequence *s, uint64_t extra, hipStream_t st)
{
    const size_t need = (size_t)(s->n + extra) * 4;
    if (need <= s->w_cap) return KMG_OK;
    void *blk = nullptr;
    size_t cap = 0;
    HIP_TRY(block_take(s->p, std::max(need, 2 * s->w_cap), &blk, &cap));
    if (s->n) {
        hipError_t e = hipMemcpyAsync(blk, s->w_blk, (size_t)s->n * 4, hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);             // (the old block is idle before it goes back)
        if (e != hipSuccess) {
            (void)hipStreamSynchronize(st);
            block_give(s->p, blk, cap);
            return fail(KMG_ERR_HIP, "growing the working sequence failed: %s", hipGetErrorString(e));
        }
    }
    block_give(s->p, s->w_blk, s->w_cap);
    s->w_blk = blk;
    s->w_cap = cap;
    return KMG_OK;
}

// One frame (host: uploaded through copy_host_image; device: read in place) -> the tail of W: the shrink of kmg_palette, then -- alpha
// mode -- the kept pixels in raster order.  Returns with `st` drained, so W is complete whatever stream the next call uses.
int add_frame(kmg_sequence *s, const uint8_t *rgba, bool on_host, uint32_t w, uint32_t h, hipStream_t st)
{
    kmg_processor *p = s->p;
    KMG_TRY(check_image_buffer(rgba, w, h));
    HIP_TRY(hipSetDevice(p->device));
    // (alpha weighting, as it is now, cuts this frame's working pixels at max(alpha_cutoff, 1): kmg_processor_set_weighting)
    const uint32_t cutoff = working_cutoff(p->alpha_cutoff.load(std::memory_order_relaxed), processor_weighting(p));
    uint32_t sw = w, sh = h;
    const uint32_t m = p->opt.shrink_max_dim;
    const bool shrink = m && (w > m || h > m);                         // structures.rs:67-74
    if (shrink) kmg_resized_dims(w, h, m, &sw, &sh);
    const uint64_t ns = (uint64_t)sw * sh;
    if (!cutoff && s->n + ns > 0xFFFFFFFFull) return fail(KMG_ERR_UNSUPPORTED, "the working sequence would reach 2^32 pixels");
    KMG_TRY(reserve(s, ns, st));
    uint8_t *tail = (uint8_t *)s->w_blk + (size_t)s->n * 4;
    const size_t bytes = (size_t)w * h * 4;

    // S_i: in the tail itself unless the compaction still has to read it
    StreamBuf up, small, count;
    const uint8_t *src = rgba;                                         // device pointer to the frame at full size
    if (on_host) {
        uint8_t *dst = tail;
        if (shrink || cutoff) { HIP_TRY(up.alloc(p, bytes, st)); dst = (uint8_t *)up.ptr; }
        HIP_TRY(copy_host_image(p, dst, rgba, bytes, hipMemcpyHostToDevice, st));
        src = dst;
    }
    if (shrink) {
        uint8_t *dst = tail;
        if (cutoff) { HIP_TRY(small.alloc(p, (size_t)ns * 4, st)); dst = (uint8_t *)small.ptr; }
        KMG_TRY(kmg_dev_resize(p, src, w, h, sw, sh, dst, st));
        src = dst;
    }
    uint64_t n_kept = ns;
    if (cutoff) {
        HIP_TRY(count.alloc(p, 256, st));
        KMG_TRY(kmg_dev_alpha_compact(p, src, ns, cutoff, tail, (uint64_t *)count.ptr, st));
        HIP_TRY(hipMemcpyAsync(&n_kept, count.ptr, sizeof n_kept, hipMemcpyDeviceToHost, st));
    } else if (src != tail) {
        HIP_TRY(hipMemcpyAsync(tail, src, (size_t)ns * 4, hipMemcpyDeviceToDevice, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    if (s->n + n_kept > 0xFFFFFFFFull) return fail(KMG_ERR_UNSUPPORTED, "the working sequence would reach 2^32 pixels");
    if (s->frames == 0) { s->sw0 = sw; s->sh0 = sh; s->first_whole = n_kept == ns; }
    s->frames += 1;
    s->n += n_kept;
    return KMG_OK;
}

// the palette step on W: a new Lloyd problem of k centroids
int sequence_centroids(kmg_sequence *s, uint32_t k, float *c4)
{
    KMG_TRY(check_k(k));
    if (s->n == 0) return fail(KMG_ERR_INVALID_ARGUMENT, "no pixel reaches alpha_cutoff (the working sequence is empty)");
    // (the processor's fixed colours, as they are when this call starts: kmg_processor_set_fixed_colors)
    const std::shared_ptr<const std::vector<float>> fixed = fixed_snapshot(s->p);
    const uint32_t f = fixed_count(fixed);
    if (k < f) return fail(KMG_ERR_INVALID_ARGUMENT, "k = %u is below the %u fixed colours of the processor", k, f);
    const int weighting = processor_weighting(s->p);                   // (as it is when this call starts)
    HIP_TRY(hipSetDevice(s->p->device));
    const bool as_image = s->frames == 1 && s->first_whole;
    return palette_of_working(s->p, (const uint8_t *)s->w_blk, as_image ? s->sw0 : (uint32_t)s->n, as_image ? s->sh0 : 1u, k, s->sg.st, c4,
                              nullptr, f ? fixed->data() : nullptr, f, weighting);
}

}  // namespace

extern "C" int kmg_sequence_create(kmg_processor *p, kmg_sequence **out)
try {
    if (!p || !out) return fail(KMG_ERR_INVALID_ARGUMENT, "sequence_create: a pointer is NULL");
    *out = nullptr;
    HIP_TRY(hipSetDevice(p->device));
    kmg_sequence *s = new kmg_sequence();
    s->p = p;
    const hipError_t e = s->sg.acquire(p);
    if (e != hipSuccess) {
        delete s;
        return fail(KMG_ERR_HIP, "no stream for the sequence: %s", hipGetErrorString(e));
    }
    *out = s;
    return KMG_OK;
}
KMG_ABI_CATCH

extern "C" void kmg_sequence_destroy(kmg_sequence *s)
try {
    if (!s) return;
    output_end(s);
    (void)hipSetDevice(s->p->device);
    (void)hipStreamSynchronize(s->sg.st);
    block_give(s->p, s->w_blk, s->w_cap);
    delete s;                                                          // (~StreamGuard returns the stream)
}
KMG_ABI_CATCH_VOID

extern "C" int kmg_sequence_add(kmg_sequence *s, const uint8_t *rgba, uint32_t w, uint32_t h)
try {
    if (!s) return fail(KMG_ERR_INVALID_ARGUMENT, "sequence is NULL");
    return add_frame(s, rgba, true, w, h, s->sg.st);
}
KMG_ABI_CATCH

extern "C" int kmg_sequence_add_device(kmg_sequence *s, const uint8_t *d_rgba, uint32_t w, uint32_t h, void *stream)
try {
    if (!s) return fail(KMG_ERR_INVALID_ARGUMENT, "sequence is NULL");
    return add_frame(s, d_rgba, false, w, h, S(stream));
}
KMG_ABI_CATCH

extern "C" int kmg_sequence_clear(kmg_sequence *s)
try {
    if (!s) return fail(KMG_ERR_INVALID_ARGUMENT, "sequence is NULL");
    s->n = 0;                                                          // (the block stays: the next frames fill it again)
    s->frames = 0;
    s->first_whole = false;
    return KMG_OK;
}
KMG_ABI_CATCH

extern "C" int kmg_sequence_info(kmg_sequence *s, uint64_t out[2])
try {
    if (!s || !out) return fail(KMG_ERR_INVALID_ARGUMENT, "sequence_info: a pointer is NULL");
    out[0] = s->frames;
    out[1] = s->n;
    return KMG_OK;
}
KMG_ABI_CATCH

extern "C" int kmg_sequence_centroids(kmg_sequence *s, uint32_t k, float *centroids4)
try {
    if (!s || !centroids4) return fail(KMG_ERR_INVALID_ARGUMENT, "sequence_centroids: a pointer is NULL");
    return sequence_centroids(s, k, centroids4);
}
KMG_ABI_CATCH

extern "C" int kmg_sequence_palette(kmg_sequence *s, uint32_t k, uint8_t *out_rgba, uint32_t *out_count)
try {
    if (!s || !out_rgba || !out_count) return fail(KMG_ERR_INVALID_ARGUMENT, "sequence_palette: a pointer is NULL");
    KMG_TRY(check_k(k));
    std::vector<float> c4(4 * (size_t)k);
    KMG_TRY(sequence_centroids(s, k, c4.data()));
    sorted_palette_of(c4.data(), k, out_rgba);
    *out_count = k;
    return KMG_OK;
}
KMG_ABI_CATCH

namespace {

// what both kinds of output ask of the mode, the format and the colour count they are opened with (index_only: per-frame palettes)
int check_output_form(uint32_t k, int mode, int format, bool index_only)
{
    KMG_TRY(check_mode(mode));
    if (index_only && format == KMG_FORMAT_RGBA8)
        return fail(KMG_ERR_INVALID_ARGUMENT, "per-frame palettes need an index format (INDEX8 / INDEX16), not RGBA8");
    KMG_TRY(check_format(format));
    KMG_TRY(check_meld_format(mode, format));
    return check_index8_room(format == KMG_FORMAT_INDEX8, "k", k, true);
}

// The output block: one sub-buffer per entry of `parts` (where its pointer goes, its bytes), each padded to 256 bytes, one behind
// the other, then the record.
int output_block(kmg_sequence *s, std::initializer_list<std::pair<uint8_t **, size_t>> parts)
{
    size_t total = 256;
    for (const auto &part : parts) total += pad256(part.second);
    HIP_TRY(block_take(s->p, total, &s->o_blk, &s->o_cap));
    uint8_t *at = (uint8_t *)s->o_blk;
    for (const auto &part : parts) {
        *part.first = at;
        at += pad256(part.second);
    }
    s->d_info = (kmg_frame_hold *)at;
    return KMG_OK;
}

// the last step of a begin: the canvas fill `e`, enqueued on the sequence's stream, has run; the output is open
int output_opened(kmg_sequence *s, hipError_t e, uint32_t k, int mode, int format, uint32_t width, uint32_t height)
{
    if (e == hipSuccess) e = hipStreamSynchronize(s->sg.st);
    if (e != hipSuccess) {
        output_end(s);
        return fail(KMG_ERR_HIP, "filling the canvas failed: %s", hipGetErrorString(e));
    }
    s->k = k; s->mode = mode; s->format = format; s->width = width; s->height = height;
    return KMG_OK;
}

}  // namespace

extern "C" int kmg_sequence_output_begin(kmg_sequence *s, uint32_t k, int mode, int format, uint32_t width, uint32_t height,
                                         uint8_t *out_palette_rgba, uint32_t *out_count)
try {
    if (!s || !out_palette_rgba || !out_count) return fail(KMG_ERR_INVALID_ARGUMENT, "sequence_output_begin: a pointer is NULL");
    output_end(s);                                                     // a second begin ends the first
    KMG_TRY(check_image_size(width, height));
    KMG_TRY(check_output_form(k, mode, format, false));
    std::vector<float> c4(4 * (size_t)std::max(k, 1u));
    KMG_TRY(sequence_centroids(s, k, c4.data()));
    hipStream_t st = s->sg.st;
    const size_t n = (size_t)width * height, es = format_bytes(format);
    s->d_canvas = s->d_delta = s->d_held = nullptr;                    // (a canvas of k holds nothing: no fill of the held source)
    if (format == KMG_FORMAT_RGBA8) KMG_TRY(output_block(s, {{&s->d_frame, n * 4}, {&s->d_map, n * es}}));
    else KMG_TRY(output_block(s, {{&s->d_frame, n * 4}, {&s->d_map, n * es}, {&s->d_canvas, n * es}, {&s->d_delta, n * es}, {&s->d_held, n * 4}}));
    const int rc = kmg_apply_plan_create_format(s->p, c4.data(), k, mode, format, n, st, &s->plan);
    if (rc != KMG_OK) {
        s->plan = nullptr;
        output_end(s);
        return rc;
    }
    hipError_t e = hipSuccess;
    if (format == KMG_FORMAT_INDEX8) e = hipMemsetD8Async((hipDeviceptr_t)s->d_canvas, (unsigned char)k, n, st);
    else if (format == KMG_FORMAT_INDEX16) e = hipMemsetD16Async((hipDeviceptr_t)s->d_canvas, (unsigned short)k, n, st);
    KMG_TRY(output_opened(s, e, k, mode, format, width, height));
    s->c4.assign(c4.begin(), c4.begin() + 4 * (size_t)k);
    for (uint32_t i = 0; i < k; ++i) shader_lab_to_rgba8(&c4[4 * i], out_palette_rgba + 4 * i);
    *out_count = k;
    return KMG_OK;
}
KMG_ABI_CATCH

namespace {

// the fresh record on the device: zero sums and maxima, all-ones minima
hipError_t fresh_record(kmg_frame_hold *d_info, size_t bytes, hipStream_t st)
{
    const hipError_t e = hipMemsetAsync(d_info, 0, bytes, st);
    return e != hipSuccess ? e : hipMemsetAsync(&d_info->x0, 0xFF, 2 * sizeof(uint32_t), st);
}

// the flags of a frame call (lossy: the call holds pixels within a tolerance)
int check_frame_flags(uint32_t flags, bool lossy)
{
    if (flags & ~KMG_FRAME_DELTA) return fail(KMG_ERR_INVALID_ARGUMENT, "unknown flags %u", flags);
    if (lossy && !(flags & KMG_FRAME_DELTA)) return fail(KMG_ERR_INVALID_ARGUMENT, "a lossy frame is a delta frame: KMG_FRAME_DELTA is required");
    return KMG_OK;
}

// what kmg_sequence_output_frame and _lossy ask of the open output and of their arguments
int check_shared_frame(const kmg_sequence *s, bool lossy, const void *rgba, uint32_t flags, const void *out, const void *info, const void *is_full)
{
    if (!s) return fail(KMG_ERR_INVALID_ARGUMENT, "sequence is NULL");
    if (s->local) return fail(KMG_ERR_INVALID_ARGUMENT, "the open output has per-frame palettes: its frames go through kmg_sequence_output_frame_local");
    if (!s->plan) return fail(KMG_ERR_INVALID_ARGUMENT, "no output is open (kmg_sequence_output_begin)");
    if (!rgba || !out) return fail(KMG_ERR_INVALID_ARGUMENT, "sequence_output_frame%s: a pointer is NULL", lossy ? "_lossy" : "");
    KMG_TRY(check_frame_flags(flags, lossy));
    if (!(flags & KMG_FRAME_DELTA)) return KMG_OK;
    if (s->format == KMG_FORMAT_RGBA8) return delta_needs_index();
    if (!info || !is_full) return fail(KMG_ERR_INVALID_ARGUMENT, "KMG_FRAME_DELTA needs info and is_full");
    return KMG_OK;
}

// One frame through the open output (the callers have checked their arguments): upload, plan run, then -- delta -- the exact pass
// (tolerance == NULL) or the lossy one on a fresh record, its read-back, and the download of the full map or the delta map.
int output_frame(kmg_sequence *s, const uint8_t *rgba, bool delta, const uint32_t *tolerance, void *out, kmg_frame_hold *rec, bool *is_full)
{
    kmg_processor *p = s->p;
    hipStream_t st = s->sg.st;
    const bool lossy = tolerance != nullptr;
    HIP_TRY(hipSetDevice(p->device));
    const size_t n = (size_t)s->width * s->height, map_bytes = n * format_bytes(s->format);
    HIP_TRY(copy_host_image(p, s->d_frame, rgba, n * 4, hipMemcpyHostToDevice, st));
    if (s->mode == KMG_MODE_DIFFUSE) apply_plan_restart(s->plan);      // every frame is an image of its own
    KMG_TRY_DRAIN(st, kmg_apply_plan_run(s->plan, s->d_frame, s->width, s->height, 0, s->d_map, st));
    *rec = kmg_frame_hold{0, 0, kFresh, kFresh, 0, 0, 0, 0};
    const size_t rec_bytes = lossy ? sizeof(kmg_frame_hold) : sizeof(kmg_frame_delta);     // (the exact record is the first 32 bytes)
    if (delta) {
        HIP_TRY(fresh_record(s->d_info, rec_bytes, st));
        KMG_TRY_DRAIN(st, lossy ? frame_hold_impl(p, s->d_frame, s->d_map, s->d_canvas, s->d_held, s->width, s->height, 0, s->format, s->k,
                                                  *tolerance, s->d_delta, s->d_info, st)
                                : frame_delta_impl(p, s->d_map, s->d_canvas, s->width, s->height, 0, s->format, s->k, s->d_delta,
                                                   reinterpret_cast<kmg_frame_delta *>(s->d_info), st));
        if (!lossy) std::swap(s->d_frame, s->d_held);                 // the canvas equals this frame's map: its held source is this frame
        HIP_TRY(hipMemcpyAsync(rec, s->d_info, rec_bytes, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    const bool full = !delta || rec->cleared > 0;                      // "over" cannot show a pixel that turns transparent
    // Index formats.  The canvas is made this frame's map where no pass did that: a frame without delta (a later delta frame starts
    // from it), and a lossy frame that is sent in full (the viewer then shows I_t everywhere: the state of an exact frame).  Its held
    // source then IS this frame: the two buffers swap instead of a copy.
    if (s->d_canvas && (lossy ? full : !delta)) {
        HIP_TRY(hipMemcpyAsync(s->d_canvas, s->d_map, map_bytes, hipMemcpyDeviceToDevice, st));
        std::swap(s->d_frame, s->d_held);
    }
    HIP_TRY(copy_host_image(p, out, full ? s->d_map : s->d_delta, map_bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    KMG_TRY(kmg_apply_plan_status(s->plan));
    *is_full = full;
    return KMG_OK;
}

// The smallest clip that takes the launch chain: staging, the table and the extra synchronisation of the batched output cost about
// three single-frame calls of 256 x 256 pixels; measured (profiles/r12_clip_time.txt), two frames are up to 1.63 of
// the per-frame path, eight at most 0.80.  Shorter clips go frame by frame through output_frame.
constexpr uint32_t kClipMinFrames = KMG_CLIP_MIN_FRAMES;

// A clip of kClipMinFrames frames or more through the open output (the caller has checked its arguments and ends the output when this fails):
// per sub-clip the frames in one stream-ordered block, their maps from apply_batch, the delta maps and records from
// frame_clip_impl, one read-back of the records, the downloads.
int output_clip(kmg_sequence *s, uint32_t n_frames, const uint8_t *const *rgba, bool delta, const uint32_t *tolerances, uint64_t max_resident_bytes,
                void *const *out, kmg_frame_hold *info, int *is_full, kmg_clip_report *rep)
{
    kmg_processor *p = s->p;
    hipStream_t st = s->sg.st;
    const bool lossy = tolerances != nullptr;
    HIP_TRY(hipSetDevice(p->device));
    const size_t n = (size_t)s->width * s->height, map_bytes = n * format_bytes(s->format);
    const uint32_t cutoff = apply_plan_cutoff(s->plan);                // (the plan's, not the processor's current one)
    // a frame keeps its source, its map and its delta map on the device
    const std::vector<uint64_t> bytes(n_frames, (uint64_t)n * 4 + 2 * (uint64_t)map_bytes);
    const std::vector<uint32_t> cuts = batch_cuts(bytes.data(), n_frames, max_resident_bytes);
    rep->sub_clips = (uint32_t)cuts.size() - 1u;
    const size_t fs = pad256(n * 4), ms = pad256(map_bytes);
    for (size_t c = 0; c + 1 < cuts.size(); ++c) {
        const uint32_t a = cuts[c], m = cuts[c + 1] - a;
        // the block: m frames | m maps | m delta maps | m records | m words
        const size_t rec_at = (size_t)m * (fs + 2 * ms), full_at = rec_at + pad256(sizeof(kmg_frame_hold) * (size_t)m);
        StreamBuf blk;
        HIP_TRY(blk.alloc(p, full_at + pad256(sizeof(uint32_t) * (size_t)m), st));
        uint8_t *base = (uint8_t *)blk.ptr;
        std::vector<const uint8_t *> src(m);
        std::vector<void *> maps(m), outs(m);
        const std::vector<uint32_t> widths(m, s->width), heights(m, s->height);
        for (uint32_t t = 0; t < m; ++t) {
            src[t] = base + (size_t)t * fs;
            maps[t] = base + (size_t)m * fs + (size_t)t * ms;
            outs[t] = base + (size_t)m * (fs + ms) + (size_t)t * ms;
            HIP_TRY_DRAIN(st, copy_host_image(p, const_cast<uint8_t *>(src[t]), rgba[a + t], n * 4, hipMemcpyHostToDevice, st));
        }
        kmg_batch_apply_report arep = {0u, 0u, 0u, 0u};
        KMG_TRY_DRAIN(st, apply_batch(p, m, src.data(), widths.data(), heights.data(), s->c4.data(), 1u, s->k, s->mode, s->format, cutoff,
                                      maps.data(), &arep, st, apply_plan_filter(s->plan), &apply_plan_dither(s->plan)));
        rep->launches += arep.launches;
        rep->batched += arep.batched;
        rep->per_image += arep.per_image;
        if (!delta) {
            for (uint32_t t = 0; t < m; ++t) {
                HIP_TRY_DRAIN(st, copy_host_image(p, out[a + t], maps[t], map_bytes, hipMemcpyDeviceToHost, st));
                if (info) info[a + t] = kmg_frame_hold{0, 0, kFresh, kFresh, 0, 0, 0, 0};
                if (is_full) is_full[a + t] = 1;
            }
            // index formats: a later delta frame starts from the last map, with the last frame as every pixel's held source
            if (s->d_canvas && a + m == n_frames) {
                HIP_TRY_DRAIN(st, hipMemcpyAsync(s->d_canvas, maps[m - 1], map_bytes, hipMemcpyDeviceToDevice, st));
                HIP_TRY_DRAIN(st, hipMemcpyAsync(s->d_held, src[m - 1], n * 4, hipMemcpyDeviceToDevice, st));
            }
            HIP_TRY(hipStreamSynchronize(st));
            continue;
        }
        kmg_frame_hold *d_info = (kmg_frame_hold *)(base + rec_at);
        uint32_t *d_full = (uint32_t *)(base + full_at);
        // the fresh records: zero sums and maxima, all-ones minima
        HIP_TRY_DRAIN(st, hipMemsetAsync(d_info, 0, sizeof(kmg_frame_hold) * (size_t)m, st));
        HIP_TRY_DRAIN(st, hipMemset2DAsync(&d_info->x0, sizeof(kmg_frame_hold), 0xFF, 2 * sizeof(uint32_t), m, st));
        // with cutoff 0 no map holds slot k: no frame is full.  An exact clip needs no flags either: its canvas is I_t in both cases.
        const uint32_t clip_flags = lossy && cutoff ? KMG_CLIP_FULL_ON_CLEAR : 0u;
        KMG_TRY_DRAIN(st, frame_clip_impl(p, m, src.data(), maps.data(), s->d_canvas, s->d_held, s->width, s->height, s->format, s->k,
                                          lossy ? tolerances + a : nullptr, clip_flags, outs.data(), d_info, d_full, &rep->launches, st));
        HIP_TRY_DRAIN(st, hipMemcpyAsync(info + a, d_info, sizeof(kmg_frame_hold) * (size_t)m, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        for (uint32_t t = 0; t < m; ++t) {
            const bool full = info[a + t].cleared > 0;                 // "over" cannot show a pixel that turns transparent
            // (a lossy frame that is full has its map in the out block already)
            HIP_TRY_DRAIN(st, copy_host_image(p, out[a + t], !lossy && full ? maps[t] : outs[t], map_bytes, hipMemcpyDeviceToHost, st));
            is_full[a + t] = full ? 1 : 0;
        }
        HIP_TRY(hipStreamSynchronize(st));
    }
    return KMG_OK;
}

}  // namespace

extern "C" int kmg_sequence_output_frames(kmg_sequence *s, uint32_t n_frames, const uint8_t *const *rgba, uint32_t flags,
                                          const uint32_t *tolerances, uint64_t max_resident_bytes, void *const *out, kmg_frame_hold *info,
                                          int *is_full, kmg_clip_report *report)
try {
    const bool lossy = tolerances != nullptr, delta = (flags & KMG_FRAME_DELTA) != 0;
    KMG_TRY(check_shared_frame(s, lossy, rgba, flags, out, info, is_full));
    if (n_frames == 0) return fail(KMG_ERR_INVALID_ARGUMENT, "sequence_output_frames: the clip has no frames");
    for (uint32_t t = 0; t < n_frames; ++t)
        if (!rgba[t] || !out[t]) return fail(KMG_ERR_INVALID_ARGUMENT, "sequence_output_frames: a pointer of frame %u is NULL", t);
    kmg_clip_report rep = {0u, 0u, 0u, 1u};
    if (n_frames < kClipMinFrames) {                                   // a short clip: the single-frame call itself, frame by frame
        for (uint32_t t = 0; t < n_frames; ++t) {
            kmg_frame_hold rec;
            bool full;
            const int rc = output_frame(s, rgba[t], delta, lossy ? tolerances + t : nullptr, out[t], &rec, &full);
            if (rc != KMG_OK) {
                output_end(s);                                         // (as the chain below: no clip is left half done on an open output)
                return rc;
            }
            if (info) info[t] = rec;
            if (is_full) is_full[t] = full ? 1 : 0;
        }
        rep.per_image = n_frames;
    } else {
        const int rc = output_clip(s, n_frames, rgba, delta, tolerances, max_resident_bytes, out, info, is_full, &rep);
        if (rc != KMG_OK) {
            output_end(s);                                             // no half-updated canvas can be used
            return rc;
        }
    }
    if (report) *report = rep;
    return KMG_OK;
}
KMG_ABI_CATCH

extern "C" int kmg_sequence_output_frame(kmg_sequence *s, const uint8_t *rgba, uint32_t flags, void *out, kmg_frame_delta *info,
                                         int *is_full)
try {
    KMG_TRY(check_shared_frame(s, false, rgba, flags, out, info, is_full));
    kmg_frame_hold rec;
    bool full;
    KMG_TRY(output_frame(s, rgba, (flags & KMG_FRAME_DELTA) != 0, nullptr, out, &rec, &full));
    if (info) *info = kmg_frame_delta{rec.changed, rec.cleared, rec.x0, rec.y0, rec.x1, rec.y1};
    if (is_full) *is_full = full ? 1 : 0;
    return KMG_OK;
}
KMG_ABI_CATCH

extern "C" int kmg_sequence_output_frame_lossy(kmg_sequence *s, const uint8_t *rgba, uint32_t flags, uint32_t tolerance, void *out,
                                               kmg_frame_hold *info, int *is_full)
try {
    KMG_TRY(check_shared_frame(s, true, rgba, flags, out, info, is_full));
    kmg_frame_hold rec;
    bool full;
    KMG_TRY(output_frame(s, rgba, true, &tolerance, out, &rec, &full));
    *info = rec;
    *is_full = full ? 1 : 0;
    return KMG_OK;
}
KMG_ABI_CATCH

extern "C" int kmg_sequence_output_end(kmg_sequence *s)
try {
    if (!s) return fail(KMG_ERR_INVALID_ARGUMENT, "sequence is NULL");
    output_end(s);
    return KMG_OK;
}
KMG_ABI_CATCH

// ---------------------------------------------------------------------------------------------
// per-frame palettes (include/kmeans_hip.h at kmg_sequence_output_begin_local)
// ---------------------------------------------------------------------------------------------
extern "C" int kmg_sequence_output_begin_local(kmg_sequence *s, uint32_t k, int mode, int format, uint32_t width, uint32_t height,
                                               uint32_t flags)
try {
    if (!s) return fail(KMG_ERR_INVALID_ARGUMENT, "sequence is NULL");
    output_end(s);                                                     // a second begin of either kind ends the first
    KMG_TRY(check_image_size(width, height));
    if (flags & ~KMG_LOCAL_WARM) return fail(KMG_ERR_INVALID_ARGUMENT, "unknown flags %u", flags);
    KMG_TRY(check_k(k));
    KMG_TRY(check_output_form(k, mode, format, true));
    HIP_TRY(hipSetDevice(s->p->device));
    const size_t n = (size_t)width * height, es = format_bytes(format);
    s->d_canvas = nullptr;
    KMG_TRY(output_block(s, {{&s->d_frame, n * 4}, {&s->d_map, n * es}, {&s->d_delta, n * es}, {&s->d_shown, n * 4}, {&s->d_held, n * 4},
                             {&s->d_pal, ((size_t)k + 1u) * 4}}));
    // nothing is shown (and nothing is held: no fill)
    KMG_TRY(output_opened(s, hipMemsetAsync(s->d_shown, 0, n * 4, s->sg.st), k, mode, format, width, height));
    s->local = true; s->have_prev = false; s->local_flags = flags;
    s->local_filter = s->p->diffusion.load(std::memory_order_relaxed);
    s->local_dither = dither_snapshot(s->p);
    return KMG_OK;
}
KMG_ABI_CATCH

extern "C" int kmg_sequence_output_frame_local(kmg_sequence *s, const uint8_t *rgba, uint32_t flags, const uint32_t *tolerance, void *out,
                                               uint8_t *out_palette_rgba, uint32_t *out_count, kmg_frame_hold *info, int *is_full)
try {
    if (!s) return fail(KMG_ERR_INVALID_ARGUMENT, "sequence is NULL");
    if (!s->local) {
        if (s->plan) return fail(KMG_ERR_INVALID_ARGUMENT, "the open output has one shared palette: its frames go through kmg_sequence_output_frame");
        return fail(KMG_ERR_INVALID_ARGUMENT, "no output is open (kmg_sequence_output_begin_local)");
    }
    if (!rgba || !out || !out_palette_rgba || !out_count || !info || !is_full)
        return fail(KMG_ERR_INVALID_ARGUMENT, "sequence_output_frame_local: a pointer is NULL");
    const bool delta = (flags & KMG_FRAME_DELTA) != 0, lossy = tolerance != nullptr;
    KMG_TRY(check_frame_flags(flags, lossy));
    kmg_processor *p = s->p;
    hipStream_t st = s->sg.st;
    const uint32_t k = s->k;
    // alpha cutoff and fixed colours: as they are when this call starts
    const uint32_t cutoff = p->alpha_cutoff.load(std::memory_order_relaxed);
    const int weighting = processor_weighting(p);
    const std::shared_ptr<const std::vector<float>> fixed = fixed_snapshot(p);
    const uint32_t f = fixed_count(fixed);
    const bool warm_output = (s->local_flags & KMG_LOCAL_WARM) != 0;
    if (warm_output && f) return fail(KMG_ERR_UNSUPPORTED, "a warm start moves every centroid: it has no fixed colours (%u are set on the processor)", f);
    if (k < f) return fail(KMG_ERR_INVALID_ARGUMENT, "k = %u is below the %u fixed colours of the processor", k, f);
    HIP_TRY(hipSetDevice(p->device));
    const size_t n = (size_t)s->width * s->height, map_bytes = n * format_bytes(s->format);
    // the frame and its centroids: nothing below touches shown or held before the palette step has succeeded
    const bool warm = warm_output && s->have_prev;
    s->have_prev = false;                                              // (the frame after one that failed starts cold)
    HIP_TRY(copy_host_image(p, s->d_frame, rgba, n * 4, hipMemcpyHostToDevice, st));
    std::vector<float> c4(4 * (size_t)k);
    KMG_TRY_DRAIN(st, local_frame_centroids(p, s->d_frame, s->width, s->height, k, cutoff, st, c4.data(), f ? fixed->data() : nullptr, f,
                                            warm ? s->prev_c4.data() : nullptr, weighting));
    KMG_TRY_DRAIN(st, dev_apply(p, s->d_frame, s->width, s->height, 0, c4.data(), k, s->mode, s->d_map, st, cutoff, s->format, s->local_filter, &s->local_dither));
    // P_t: the bytes the output pass writes for each centroid, to the caller and -- one small stream-ordered copy -- to the device
    std::vector<uint8_t> pal(4 * (size_t)k);
    for (uint32_t i = 0; i < k; ++i) shader_lab_to_rgba8(&c4[4 * i], &pal[4 * i]);
    HIP_TRY_DRAIN(st, hipMemcpyAsync(s->d_pal, pal.data(), pal.size(), hipMemcpyHostToDevice, st));
    kmg_frame_hold rec{0, 0, kFresh, kFresh, 0, 0, 0, 0};
    const size_t rec_bytes = lossy ? sizeof(kmg_frame_hold) : sizeof(kmg_frame_delta);     // (the exact record is the first 32 bytes)
    HIP_TRY_DRAIN(st, fresh_record(s->d_info, rec_bytes, st));
    // without KMG_FRAME_DELTA the exact pass still runs: it leaves shown = P_t[I_t] everywhere; its delta map and record are not used
    KMG_TRY_DRAIN(st, frame_local_impl(p, lossy ? s->d_frame : nullptr, s->d_map, s->d_pal, s->d_shown, lossy ? s->d_held : nullptr, s->width,
                                       s->height, 0, s->format, k, lossy, lossy ? *tolerance : 0u, s->d_delta, s->d_info, st));
    if (delta) HIP_TRY_DRAIN(st, hipMemcpyAsync(&rec, s->d_info, rec_bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY_DRAIN(st, hipStreamSynchronize(st));
    const bool full = !delta || rec.cleared > 0;                       // "over" cannot show a pixel that turns transparent
    // a lossy frame that is sent in full: the viewer then shows P_t[I_t] everywhere -- the exact pass makes the canvas that
    if (lossy && full) {
        HIP_TRY_DRAIN(st, fresh_record(s->d_info, sizeof(kmg_frame_delta), st));
        KMG_TRY_DRAIN(st, frame_local_impl(p, nullptr, s->d_map, s->d_pal, s->d_shown, nullptr, s->width, s->height, 0, s->format, k, false, 0u,
                                           s->d_delta, s->d_info, st));
    }
    // after an exact frame or a full one every pixel's held source IS this frame: the two buffers swap instead of a copy
    if (!lossy || full) std::swap(s->d_frame, s->d_held);
    HIP_TRY_DRAIN(st, copy_host_image(p, out, full ? s->d_map : s->d_delta, map_bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY_DRAIN(st, hipStreamSynchronize(st));
    memcpy(out_palette_rgba, pal.data(), pal.size());
    *out_count = k;
    *info = rec;
    *is_full = full ? 1 : 0;
    s->prev_c4.swap(c4);
    s->have_prev = true;
    return KMG_OK;
}
KMG_ABI_CATCH
