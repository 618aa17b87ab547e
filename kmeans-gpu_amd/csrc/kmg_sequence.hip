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
//                    kmg_hold.hip) in one block.

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

int frame_delta_impl(kmg_processor *p, const void *d_index, void *d_canvas, uint32_t width, uint32_t rows, uint32_t row0, int format,
                     uint32_t k, void *d_delta, kmg_frame_delta *d_info, hipStream_t st)
{
    static_assert(sizeof(kmg_frame_delta) == 32, "kmg_frame_delta is 32 bytes");
    const int rc = check_index_band("frame_delta", false, p, d_index, d_canvas, d_delta, nullptr, nullptr, d_info, width, rows, row0, format, k);
    if (rc != KMG_OK) return rc;
    const uint64_t n = (uint64_t)width * rows;
    HIP_TRY(hipSetDevice(p->device));
    unsigned long long *info = reinterpret_cast<unsigned long long *>(d_info);
    if (format == KMG_FORMAT_INDEX8) HIP_TRY(frame_delta_typed<uint8_t>(d_index, d_canvas, d_delta, n, width, row0, k, info, st));
    else HIP_TRY(frame_delta_typed<uint16_t>(d_index, d_canvas, d_delta, n, width, row0, k, info, st));
    return KMG_OK;
}

}  // namespace

int check_index_band(const char *name, bool lossy, const kmg_processor *p, const void *d_index, const void *d_canvas, const void *d_delta,
                     const void *d_src, const void *d_held, const void *d_info, uint32_t width, uint32_t rows, uint32_t row0, int format,
                     uint32_t k)
{
    if (format == KMG_FORMAT_RGBA8) return fail(KMG_ERR_INVALID_ARGUMENT, "a delta frame needs an index format (INDEX8 / INDEX16), not RGBA8");
    if (format != KMG_FORMAT_INDEX8 && format != KMG_FORMAT_INDEX16) return fail(KMG_ERR_INVALID_ARGUMENT, "unknown output format %d", format);
    if (k == 0 || k > KMG_MAX_K) return fail(KMG_ERR_INVALID_ARGUMENT, "k = %u: 1 .. %u", k, KMG_MAX_K);
    if (format == KMG_FORMAT_INDEX8 && k > 255u) return fail(KMG_ERR_INVALID_ARGUMENT, "INDEX8 holds 256 indices; k = %u plus the transparent slot needs INDEX16", k);
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
    uint8_t *d_shown = nullptr, *d_pal = nullptr;
    std::vector<float> prev_c4;      // C_{t-1}: where a warm frame's Lloyd loop starts
};

namespace {

size_t format_bytes(int format) { return format == KMG_FORMAT_INDEX8 ? 1u : format == KMG_FORMAT_INDEX16 ? 2u : 4u; }

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
    int rc;
    kmg_processor *p = s->p;
    if (!rgba) return fail(KMG_ERR_INVALID_ARGUMENT, "image pointer is NULL");
    if (w == 0 || h == 0) return fail(KMG_ERR_INVALID_ARGUMENT, "image has zero width or height");
    if ((uint64_t)w * h > 0xFFFFFFFFull) return fail(KMG_ERR_UNSUPPORTED, "image has more than 2^32-1 pixels");
    HIP_TRY(hipSetDevice(p->device));
    // (alpha weighting, as it is now, cuts this frame's working pixels at max(alpha_cutoff, 1): kmg_processor_set_weighting)
    const uint32_t cutoff = working_cutoff(p->alpha_cutoff.load(std::memory_order_relaxed), processor_weighting(p));
    uint32_t sw = w, sh = h;
    const uint32_t m = p->opt.shrink_max_dim;
    const bool shrink = m && (w > m || h > m);                         // structures.rs:67-74
    if (shrink) kmg_resized_dims(w, h, m, &sw, &sh);
    const uint64_t ns = (uint64_t)sw * sh;
    if (!cutoff && s->n + ns > 0xFFFFFFFFull) return fail(KMG_ERR_UNSUPPORTED, "the working sequence would reach 2^32 pixels");
    if ((rc = reserve(s, ns, st)) != KMG_OK) return rc;
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
        if ((rc = kmg_dev_resize(p, src, w, h, sw, sh, dst, st)) != KMG_OK) return rc;
        src = dst;
    }
    uint64_t n_kept = ns;
    if (cutoff) {
        HIP_TRY(count.alloc(p, 256, st));
        if ((rc = kmg_dev_alpha_compact(p, src, ns, cutoff, tail, (uint64_t *)count.ptr, st)) != KMG_OK) return rc;
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
    if (k == 0) return fail(KMG_ERR_INVALID_ARGUMENT, "k must be an integer higher than 0");
    if (k > KMG_MAX_K) return fail(KMG_ERR_UNSUPPORTED, "k = %u exceeds KMG_MAX_K = %u", k, KMG_MAX_K);
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
    int rc;
    if (!s || !out_rgba || !out_count) return fail(KMG_ERR_INVALID_ARGUMENT, "sequence_palette: a pointer is NULL");
    if (k == 0) return fail(KMG_ERR_INVALID_ARGUMENT, "k must be an integer higher than 0");
    if (k > KMG_MAX_K) return fail(KMG_ERR_UNSUPPORTED, "k = %u exceeds KMG_MAX_K = %u", k, KMG_MAX_K);
    std::vector<float> c4(4 * (size_t)k);
    if ((rc = sequence_centroids(s, k, c4.data())) != KMG_OK) return rc;
    sorted_palette_of(c4.data(), k, out_rgba);
    *out_count = k;
    return KMG_OK;
}
KMG_ABI_CATCH

extern "C" int kmg_sequence_output_begin(kmg_sequence *s, uint32_t k, int mode, int format, uint32_t width, uint32_t height,
                                         uint8_t *out_palette_rgba, uint32_t *out_count)
try {
    int rc;
    if (!s || !out_palette_rgba || !out_count) return fail(KMG_ERR_INVALID_ARGUMENT, "sequence_output_begin: a pointer is NULL");
    output_end(s);                                                     // a second begin ends the first
    if (width == 0 || height == 0) return fail(KMG_ERR_INVALID_ARGUMENT, "image has zero width or height");
    if ((uint64_t)width * height > 0xFFFFFFFFull) return fail(KMG_ERR_UNSUPPORTED, "image has more than 2^32-1 pixels");
    if (mode < KMG_MODE_REPLACE || mode > KMG_MODE_DIFFUSE) return fail(KMG_ERR_INVALID_ARGUMENT, "unknown mode %d", mode);
    if (format < KMG_FORMAT_RGBA8 || format > KMG_FORMAT_INDEX16) return fail(KMG_ERR_INVALID_ARGUMENT, "unknown output format %d", format);
    if (format != KMG_FORMAT_RGBA8 && mode == KMG_MODE_MELD) return fail(KMG_ERR_INVALID_ARGUMENT, "meld blends two colours: it has no index output");
    if (format == KMG_FORMAT_INDEX8 && k > 255u)
        return fail(KMG_ERR_INVALID_ARGUMENT, "INDEX8 holds 256 indices; k = %u plus the transparent slot needs INDEX16", k);
    std::vector<float> c4(4 * (size_t)std::max(k, 1u));
    if ((rc = sequence_centroids(s, k, c4.data())) != KMG_OK) return rc;
    kmg_processor *p = s->p;
    hipStream_t st = s->sg.st;
    const size_t n = (size_t)width * height, es = format_bytes(format);
    const bool indexed = format != KMG_FORMAT_RGBA8;
    const size_t frame_b = pad256(n * 4), map_b = pad256(n * es);
    HIP_TRY(block_take(p, frame_b + map_b * (indexed ? 3u : 1u) + (indexed ? frame_b : 0u) + 256, &s->o_blk, &s->o_cap));
    s->d_frame = (uint8_t *)s->o_blk;
    s->d_map = s->d_frame + frame_b;
    s->d_canvas = indexed ? s->d_map + map_b : nullptr;
    s->d_delta = indexed ? s->d_canvas + map_b : nullptr;
    s->d_held = indexed ? s->d_delta + map_b : nullptr;                // (a canvas of k holds nothing: no fill)
    s->d_info = (kmg_frame_hold *)(s->d_map + map_b * (indexed ? 3u : 1u) + (indexed ? frame_b : 0u));
    if ((rc = kmg_apply_plan_create_format(p, c4.data(), k, mode, format, n, st, &s->plan)) != KMG_OK) {
        s->plan = nullptr;
        output_end(s);
        return rc;
    }
    hipError_t e = hipSuccess;
    if (format == KMG_FORMAT_INDEX8) e = hipMemsetD8Async((hipDeviceptr_t)s->d_canvas, (unsigned char)k, n, st);
    else if (format == KMG_FORMAT_INDEX16) e = hipMemsetD16Async((hipDeviceptr_t)s->d_canvas, (unsigned short)k, n, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        output_end(s);
        return fail(KMG_ERR_HIP, "filling the canvas failed: %s", hipGetErrorString(e));
    }
    s->k = k; s->mode = mode; s->format = format; s->width = width; s->height = height;
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

// One frame through the open output (the callers have checked their arguments): upload, plan run, then -- delta -- the exact pass
// (tolerance == NULL) or the lossy one on a fresh record, its read-back, and the download of the full map or the delta map.
int output_frame(kmg_sequence *s, const uint8_t *rgba, bool delta, const uint32_t *tolerance, void *out, kmg_frame_hold *rec, bool *is_full)
{
    int rc;
    kmg_processor *p = s->p;
    hipStream_t st = s->sg.st;
    const bool lossy = tolerance != nullptr;
    HIP_TRY(hipSetDevice(p->device));
    const size_t n = (size_t)s->width * s->height, map_bytes = n * format_bytes(s->format);
    HIP_TRY(copy_host_image(p, s->d_frame, rgba, n * 4, hipMemcpyHostToDevice, st));
    if (s->mode == KMG_MODE_DIFFUSE) apply_plan_restart(s->plan);      // every frame is an image of its own
    if ((rc = kmg_apply_plan_run(s->plan, s->d_frame, s->width, s->height, 0, s->d_map, st)) != KMG_OK) {
        (void)hipStreamSynchronize(st);
        return rc;
    }
    *rec = kmg_frame_hold{0, 0, kFresh, kFresh, 0, 0, 0, 0};
    const size_t rec_bytes = lossy ? sizeof(kmg_frame_hold) : sizeof(kmg_frame_delta);     // (the exact record is the first 32 bytes)
    if (delta) {
        HIP_TRY(fresh_record(s->d_info, rec_bytes, st));
        if (lossy) rc = frame_hold_impl(p, s->d_frame, s->d_map, s->d_canvas, s->d_held, s->width, s->height, 0, s->format, s->k, *tolerance,
                                        s->d_delta, s->d_info, st);
        else rc = frame_delta_impl(p, s->d_map, s->d_canvas, s->width, s->height, 0, s->format, s->k, s->d_delta,
                                   reinterpret_cast<kmg_frame_delta *>(s->d_info), st);
        if (rc != KMG_OK) {
            (void)hipStreamSynchronize(st);
            return rc;
        }
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
    if ((rc = kmg_apply_plan_status(s->plan)) != KMG_OK) return rc;
    *is_full = full;
    return KMG_OK;
}

}  // namespace

extern "C" int kmg_sequence_output_frame(kmg_sequence *s, const uint8_t *rgba, uint32_t flags, void *out, kmg_frame_delta *info,
                                         int *is_full)
try {
    if (!s) return fail(KMG_ERR_INVALID_ARGUMENT, "sequence is NULL");
    if (s->local) return fail(KMG_ERR_INVALID_ARGUMENT, "the open output has per-frame palettes: its frames go through kmg_sequence_output_frame_local");
    if (!s->plan) return fail(KMG_ERR_INVALID_ARGUMENT, "no output is open (kmg_sequence_output_begin)");
    if (!rgba || !out) return fail(KMG_ERR_INVALID_ARGUMENT, "sequence_output_frame: a pointer is NULL");
    if (flags & ~KMG_FRAME_DELTA) return fail(KMG_ERR_INVALID_ARGUMENT, "unknown flags %u", flags);
    const bool delta = (flags & KMG_FRAME_DELTA) != 0;
    if (delta && s->format == KMG_FORMAT_RGBA8) return fail(KMG_ERR_INVALID_ARGUMENT, "a delta frame needs an index format (INDEX8 / INDEX16), not RGBA8");
    if (delta && (!info || !is_full)) return fail(KMG_ERR_INVALID_ARGUMENT, "KMG_FRAME_DELTA needs info and is_full");
    kmg_frame_hold rec;
    bool full;
    const int rc = output_frame(s, rgba, delta, nullptr, out, &rec, &full);
    if (rc != KMG_OK) return rc;
    if (info) *info = kmg_frame_delta{rec.changed, rec.cleared, rec.x0, rec.y0, rec.x1, rec.y1};
    if (is_full) *is_full = full ? 1 : 0;
    return KMG_OK;
}
KMG_ABI_CATCH

extern "C" int kmg_sequence_output_frame_lossy(kmg_sequence *s, const uint8_t *rgba, uint32_t flags, uint32_t tolerance, void *out,
                                               kmg_frame_hold *info, int *is_full)
try {
    if (!s) return fail(KMG_ERR_INVALID_ARGUMENT, "sequence is NULL");
    if (s->local) return fail(KMG_ERR_INVALID_ARGUMENT, "the open output has per-frame palettes: its frames go through kmg_sequence_output_frame_local");
    if (!s->plan) return fail(KMG_ERR_INVALID_ARGUMENT, "no output is open (kmg_sequence_output_begin)");
    if (!rgba || !out) return fail(KMG_ERR_INVALID_ARGUMENT, "sequence_output_frame_lossy: a pointer is NULL");
    if (flags & ~KMG_FRAME_DELTA) return fail(KMG_ERR_INVALID_ARGUMENT, "unknown flags %u", flags);
    if (!(flags & KMG_FRAME_DELTA)) return fail(KMG_ERR_INVALID_ARGUMENT, "a lossy frame is a delta frame: KMG_FRAME_DELTA is required");
    if (s->format == KMG_FORMAT_RGBA8) return fail(KMG_ERR_INVALID_ARGUMENT, "a delta frame needs an index format (INDEX8 / INDEX16), not RGBA8");
    if (!info || !is_full) return fail(KMG_ERR_INVALID_ARGUMENT, "KMG_FRAME_DELTA needs info and is_full");
    kmg_frame_hold rec;
    bool full;
    const int rc = output_frame(s, rgba, true, &tolerance, out, &rec, &full);
    if (rc != KMG_OK) return rc;
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
    if (width == 0 || height == 0) return fail(KMG_ERR_INVALID_ARGUMENT, "image has zero width or height");
    if ((uint64_t)width * height > 0xFFFFFFFFull) return fail(KMG_ERR_UNSUPPORTED, "image has more than 2^32-1 pixels");
    if (flags & ~KMG_LOCAL_WARM) return fail(KMG_ERR_INVALID_ARGUMENT, "unknown flags %u", flags);
    if (k == 0) return fail(KMG_ERR_INVALID_ARGUMENT, "k must be an integer higher than 0");
    if (k > KMG_MAX_K) return fail(KMG_ERR_UNSUPPORTED, "k = %u exceeds KMG_MAX_K = %u", k, KMG_MAX_K);
    if (mode < KMG_MODE_REPLACE || mode > KMG_MODE_DIFFUSE) return fail(KMG_ERR_INVALID_ARGUMENT, "unknown mode %d", mode);
    if (format == KMG_FORMAT_RGBA8) return fail(KMG_ERR_INVALID_ARGUMENT, "per-frame palettes need an index format (INDEX8 / INDEX16), not RGBA8");
    if (format != KMG_FORMAT_INDEX8 && format != KMG_FORMAT_INDEX16) return fail(KMG_ERR_INVALID_ARGUMENT, "unknown output format %d", format);
    if (mode == KMG_MODE_MELD) return fail(KMG_ERR_INVALID_ARGUMENT, "meld blends two colours: it has no index output");
    if (format == KMG_FORMAT_INDEX8 && k > 255u)
        return fail(KMG_ERR_INVALID_ARGUMENT, "INDEX8 holds 256 indices; k = %u plus the transparent slot needs INDEX16", k);
    kmg_processor *p = s->p;
    hipStream_t st = s->sg.st;
    HIP_TRY(hipSetDevice(p->device));
    const size_t n = (size_t)width * height, es = format_bytes(format);
    const size_t frame_b = pad256(n * 4), map_b = pad256(n * es), pal_b = pad256(((size_t)k + 1u) * 4);
    HIP_TRY(block_take(p, 3 * frame_b + 2 * map_b + pal_b + 256, &s->o_blk, &s->o_cap));
    s->d_frame = (uint8_t *)s->o_blk;
    s->d_map = s->d_frame + frame_b;
    s->d_delta = s->d_map + map_b;
    s->d_shown = s->d_delta + map_b;
    s->d_held = s->d_shown + frame_b;
    s->d_pal = s->d_held + frame_b;
    s->d_info = (kmg_frame_hold *)(s->d_pal + pal_b);
    s->d_canvas = nullptr;
    hipError_t e = hipMemsetAsync(s->d_shown, 0, n * 4, st);           // nothing is shown (and nothing is held: no fill)
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        output_end(s);
        return fail(KMG_ERR_HIP, "filling the canvas failed: %s", hipGetErrorString(e));
    }
    s->k = k; s->mode = mode; s->format = format; s->width = width; s->height = height;
    s->local = true; s->have_prev = false; s->local_flags = flags;
    return KMG_OK;
}
KMG_ABI_CATCH

// HIP_TRY for a call that has copies in flight to or from its own locals: the stream is drained before the early return
#define HIP_TRY_DRAIN(st_, expr)                                                               \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess) {                                                                \
            (void)hipStreamSynchronize(st_);                                                   \
            return fail(e_ == hipErrorOutOfMemory ? KMG_ERR_OUT_OF_MEMORY : KMG_ERR_HIP,       \
                        "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
        }                                                                                      \
    } while (0)

extern "C" int kmg_sequence_output_frame_local(kmg_sequence *s, const uint8_t *rgba, uint32_t flags, const uint32_t *tolerance, void *out,
                                               uint8_t *out_palette_rgba, uint32_t *out_count, kmg_frame_hold *info, int *is_full)
try {
    int rc;
    if (!s) return fail(KMG_ERR_INVALID_ARGUMENT, "sequence is NULL");
    if (!s->local) {
        if (s->plan) return fail(KMG_ERR_INVALID_ARGUMENT, "the open output has one shared palette: its frames go through kmg_sequence_output_frame");
        return fail(KMG_ERR_INVALID_ARGUMENT, "no output is open (kmg_sequence_output_begin_local)");
    }
    if (!rgba || !out || !out_palette_rgba || !out_count || !info || !is_full)
        return fail(KMG_ERR_INVALID_ARGUMENT, "sequence_output_frame_local: a pointer is NULL");
    if (flags & ~KMG_FRAME_DELTA) return fail(KMG_ERR_INVALID_ARGUMENT, "unknown flags %u", flags);
    const bool delta = (flags & KMG_FRAME_DELTA) != 0, lossy = tolerance != nullptr;
    if (lossy && !delta) return fail(KMG_ERR_INVALID_ARGUMENT, "a lossy frame is a delta frame: KMG_FRAME_DELTA is required");
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
    if ((rc = local_frame_centroids(p, s->d_frame, s->width, s->height, k, cutoff, st, c4.data(), f ? fixed->data() : nullptr, f,
                                    warm ? s->prev_c4.data() : nullptr, weighting)) != KMG_OK) {
        (void)hipStreamSynchronize(st);
        return rc;
    }
    if ((rc = dev_apply(p, s->d_frame, s->width, s->height, 0, c4.data(), k, s->mode, s->d_map, st, cutoff, s->format)) != KMG_OK) {
        (void)hipStreamSynchronize(st);
        return rc;
    }
    // P_t: the bytes the output pass writes for each centroid, to the caller and -- one small stream-ordered copy -- to the device
    std::vector<uint8_t> pal(4 * (size_t)k);
    for (uint32_t i = 0; i < k; ++i) shader_lab_to_rgba8(&c4[4 * i], &pal[4 * i]);
    HIP_TRY_DRAIN(st, hipMemcpyAsync(s->d_pal, pal.data(), pal.size(), hipMemcpyHostToDevice, st));
    kmg_frame_hold rec{0, 0, kFresh, kFresh, 0, 0, 0, 0};
    const size_t rec_bytes = lossy ? sizeof(kmg_frame_hold) : sizeof(kmg_frame_delta);     // (the exact record is the first 32 bytes)
    HIP_TRY_DRAIN(st, fresh_record(s->d_info, rec_bytes, st));
    // without KMG_FRAME_DELTA the exact pass still runs: it leaves shown = P_t[I_t] everywhere; its delta map and record are not used
    rc = frame_local_impl(p, lossy ? s->d_frame : nullptr, s->d_map, s->d_pal, s->d_shown, lossy ? s->d_held : nullptr, s->width, s->height, 0,
                          s->format, k, lossy, lossy ? *tolerance : 0u, s->d_delta, s->d_info, st);
    if (rc != KMG_OK) {
        (void)hipStreamSynchronize(st);
        return rc;
    }
    if (delta) HIP_TRY_DRAIN(st, hipMemcpyAsync(&rec, s->d_info, rec_bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY_DRAIN(st, hipStreamSynchronize(st));
    const bool full = !delta || rec.cleared > 0;                       // "over" cannot show a pixel that turns transparent
    // a lossy frame that is sent in full: the viewer then shows P_t[I_t] everywhere -- the exact pass makes the canvas that
    if (lossy && full) {
        HIP_TRY_DRAIN(st, fresh_record(s->d_info, sizeof(kmg_frame_delta), st));
        if ((rc = frame_local_impl(p, nullptr, s->d_map, s->d_pal, s->d_shown, nullptr, s->width, s->height, 0, s->format, k, false, 0u, s->d_delta,
                                   s->d_info, st)) != KMG_OK) {
            (void)hipStreamSynchronize(st);
            return rc;
        }
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
