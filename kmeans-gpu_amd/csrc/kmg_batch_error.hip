// kmg_batch_error.hip -- the error record of many images in one launch: the segmented version of k_error_stats (kmg_error.hip) and
// kmg_dev_compare_batch on top of it (include/kmeans_hip.h at kmg_batch_quality_report).
//
// A launch reads a table of BatchErrorImage records in device memory, one per image.  Its grid is the sum of the images' tiles
// (kPassTile pixels each); a workgroup finds its image by the bounded binary search over the records' first-workgroup column
// (batch_image_of, kmg_device.h), stages that image's palette entries in LDS, runs the arithmetic of k_error_stats on ONE tile of
// it and COMBINES into that image's record: sums by 64-bit atomic adds, maxima by atomic maxima.  The fields are exact integers,
// so how the pixels of an image are dealt to workgroups changes no field: record i is what kmg_dev_compare leaves for image i.
// k_error_stats keeps its own text (the per-image kernels keep their code, as k_apply beside apply_tiles).
//
// Synchronisation: the launch boundary, nothing else.  No workgroup waits for another, every loop has a bound known at launch.

#include "kmg_state.h"

#include "kmg_batch_layout.h"
#include "kmg_pass.h"

namespace kmg {

namespace {

constexpr uint32_t kErrFields = 14;                     // kmg_error_stats as 14 x u64
enum { fPixels = 0, fChanged = 1, fInvalid = 2, fSse = 3, fSad = 6, fMax = 9, fLabSse = 12, fLabMax = 13 };

__host__ __device__ constexpr bool field_is_max(uint32_t f) { return (f >= fMax && f < fMax + 3) || f == fLabMax; }

// One image of a batched error launch.  entries / pal: the image's part of the concatenated (word, qL, qa, qb) entries and palette
// words (index formats; NULL for RGBA8).  aligned: both pointers allow the vector loads of k_error_stats.
struct alignas(16) BatchErrorImage {
    const uint32_t *src;           // n source pixels
    const void *out;               // n outputs of the launch's format
    const int4 *entries;           // k
    const uint32_t *pal;           // k
    unsigned long long *stats;     // the image's record, 14 words
    uint32_t n;                    // pixels
    uint32_t first_wg;             // index of the image's first workgroup in the grid
    uint32_t k;
    uint32_t aligned;
};
static_assert(sizeof(BatchErrorImage) == 64, "BatchErrorImage layout");

template <int FORM>
__device__ __forceinline__ void load4_out(const void *out, uint64_t i0, uint64_t n, bool aligned, uint32_t v[4])
{
    if (FORM == kErrorIndex8) load4_index<uint8_t, true>(static_cast<const uint8_t *>(out), i0, n, aligned, v);
    else if (FORM == kErrorIndex16) load4_index<uint16_t, true>(static_cast<const uint16_t *>(out), i0, n, aligned, v);
    else load4_stream(static_cast<const uint32_t *>(out), i0, n, aligned, v);
}

// workgroup wg0 + blockIdx.x of the batch's grid: one tile of its image (a lane: four consecutive pixels, so its 32-bit sums hold)
template <int FORM, uint32_t WHAT>
__global__ __launch_bounds__(kPassBlock) void k_batch_error_stats(const BatchErrorImage *__restrict__ img, uint32_t n_images, uint32_t wg0,
                                                                uint32_t cutoff, const float *__restrict__ lut)
{
    constexpr bool RGB = (WHAT & KMG_ERROR_RGB) != 0, LAB = (WHAT & KMG_ERROR_LAB) != 0, INDEXED = FORM != kErrorRgba8;
    extern __shared__ uint4 s_dyn[];                            // index forms: k words, or -- LAB -- k (word, qL, qa, qb) entries
    __shared__ float s_lut[LAB ? 256 : 1];
    __shared__ unsigned long long s_part[kPassWaves][kErrFields];
    const uint32_t wg = wg0 + blockIdx.x;
    const BatchErrorImage im = img[batch_image_of(img, n_images, wg)];
    const uint32_t k = im.k;
    const uint64_t n = im.n;
    const bool aligned = im.aligned != 0u;
    const uint32_t *s_pal = reinterpret_cast<const uint32_t *>(s_dyn);
    const int4 *s_ent = reinterpret_cast<const int4 *>(s_dyn);
    if (LAB) s_lut[threadIdx.x] = lut[threadIdx.x];
    if (INDEXED) {
        if (LAB) for (uint32_t i = threadIdx.x; i < k; i += kPassBlock) reinterpret_cast<int4 *>(s_dyn)[i] = im.entries[i];
        else for (uint32_t i = threadIdx.x; i < k; i += kPassBlock) reinterpret_cast<uint32_t *>(s_dyn)[i] = im.pal[i];
    }
    if (LAB || INDEXED) __syncthreads();

    uint32_t pixels = 0, changed = 0, invalid = 0, lab_max = 0;
    uint32_t sse[3] = {0u, 0u, 0u}, sad[3] = {0u, 0u, 0u}, mx[3] = {0u, 0u, 0u};
    unsigned long long lab_sse = 0;

    const uint64_t i0 = (uint64_t)(wg - im.first_wg) * kPassTile + (uint64_t)threadIdx.x * 4u;
    uint32_t ps[4], po[4];
    load4_stream(im.src, i0, n, aligned, ps);
    load4_out<FORM>(im.out, i0, n, aligned, po);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint32_t s = ps[q];
        const bool counted = i0 + (uint64_t)q < n && (s >> 24) >= cutoff;
        bool valid = true;
        uint32_t o = po[q];
        int4 e = make_int4(0, 0, 0, 0);
        if (INDEXED) {
            valid = o < k;
            const uint32_t idx = valid ? o : 0u;
            if (LAB) { e = s_ent[idx]; o = (uint32_t)e.x; }
            else o = s_pal[idx];
        }
        const bool use = counted && valid;
        pixels += use ? 1u : 0u;
        invalid += (counted && !valid) ? 1u : 0u;
        o = use ? o : s;                                    // a pixel that does not count is compared with itself
        const bool differs = ((s ^ o) & 0x00FFFFFFu) != 0u;
        changed += differs ? 1u : 0u;
        if (RGB) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int d = (int)((s >> (8 * c)) & 255u) - (int)((o >> (8 * c)) & 255u);
                const uint32_t ad = (uint32_t)(d < 0 ? -d : d);
                sse[c] += ad * ad;
                sad[c] += ad;
                mx[c] = max(mx[c], ad);
            }
        }
        if (LAB) {
            if (differs) {                                  // equal colours have equal q: the term is 0
                int32_t qs[3], qo[3];
                px_to_q(s_lut, s, qs);
                if (INDEXED) { qo[0] = e.y; qo[1] = e.z; qo[2] = e.w; }
                else px_to_q(s_lut, o, qo);
                const int32_t dL = qs[0] - qo[0], da = qs[1] - qo[1], db = qs[2] - qo[2];
                const uint32_t term = (uint32_t)(dL * dL) + (uint32_t)(da * da) + (uint32_t)(db * db);   // < 2^29
                lab_sse += term;
                lab_max = max(lab_max, term);
            }
        }
    }

    unsigned long long v[kErrFields];
    v[fPixels] = pixels; v[fChanged] = changed; v[fInvalid] = invalid;
#pragma unroll
    for (int c = 0; c < 3; ++c) { v[fSse + c] = sse[c]; v[fSad + c] = sad[c]; v[fMax + c] = mx[c]; }
    v[fLabSse] = lab_sse; v[fLabMax] = lab_max;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
    for (uint32_t f = 0; f < kErrFields; ++f) {
        const bool wanted = f < fSse || (f < fLabSse ? RGB : LAB);
        if (!wanted) continue;
        unsigned long long x = v[f];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long y = __shfl_xor(x, o);
            x = field_is_max(f) ? max(x, y) : x + y;
        }
        if (lane == 0) s_part[wave][f] = x;
    }
    __syncthreads();
    if (threadIdx.x < kErrFields) {
        const uint32_t f = threadIdx.x;
        const bool wanted = f < fSse || (f < fLabSse ? RGB : LAB);
        if (wanted) {
            unsigned long long x = 0;
#pragma unroll
            for (uint32_t w = 0; w < kPassWaves; ++w) x = field_is_max(f) ? max(x, s_part[w][f]) : x + s_part[w][f];
            if (x != 0) {                                       // (adding 0 or maxing with 0 changes nothing)
                if (field_is_max(f)) atomicMax(im.stats + f, x);
                else atomicAdd(im.stats + f, x);
            }
        }
    }
}

hipError_t launch_batch_error(int form, uint32_t what, const BatchErrorImage *rec, uint32_t m, BatchLaunch cut, uint32_t k_max, uint32_t cutoff,
                              const float *lut, hipStream_t st)
{
    const bool lab = (what & KMG_ERROR_LAB) != 0;
    const size_t lds = form == kErrorRgba8 ? 0 : (size_t)k_max * (lab ? sizeof(int4) : sizeof(uint32_t));
    bool launched = false;                                            // (stays false for a form or `what` that does not exist)
    with_value<kErrorRgba8, kErrorIndex8, kErrorIndex16>(form, [&](auto F) {
        with_value<KMG_ERROR_RGB, KMG_ERROR_LAB, KMG_ERROR_RGB | KMG_ERROR_LAB>((int)what, [&](auto W) {
            hipLaunchKernelGGL((k_batch_error_stats<F(), W()>), dim3(cut.count), dim3(kPassBlock), lds, st, rec, m, cut.first, cutoff, lut);
            launched = true;
        });
    });
    return launched ? hipGetLastError() : hipErrorInvalidValue;
}

}  // namespace

int dev_compare_batch(kmg_processor *p, uint32_t n_images, const uint8_t *const *d_src, const void *const *d_out, const uint64_t *n_pixels,
                      int format, const uint8_t *palettes, const uint32_t *ks, uint32_t cutoff, uint32_t what, kmg_error_stats *d_stats,
                      hipStream_t st, uint32_t *launches)
{
    static_assert(sizeof(kmg_error_stats) == kErrFields * sizeof(uint64_t), "kmg_error_stats is 14 x uint64_t");
    const int form = format == KMG_FORMAT_RGBA8 ? kErrorRgba8 : format == KMG_FORMAT_INDEX8 ? kErrorIndex8 : kErrorIndex16;
    const bool indexed = form != kErrorRgba8, lab = (what & KMG_ERROR_LAB) != 0;
    std::vector<uint64_t> pixels(n_pixels, n_pixels + n_images);
    std::vector<uint32_t> first_wg;
    uint64_t grid = 0;
    if (!batch_grid(pixels.data(), n_images, kPassTile, first_wg, &grid)) return fail(KMG_ERR_UNSUPPORTED, "the batch has more than 2^32-1 tiles");
    size_t k_sum = 0;
    uint32_t k_max = 0;
    for (uint32_t i = 0; indexed && i < n_images; ++i) { k_sum += ks[i]; k_max = std::max(k_max, ks[i]); }

    // the scratch: [records][entries of all palettes][words of all palettes]
    const size_t rec_bytes = pad256(sizeof(BatchErrorImage) * (size_t)n_images), ent_bytes = pad256(error_palette_bytes((uint32_t)k_sum));
    StreamBuf tab;
    HIP_TRY(tab.alloc(p, rec_bytes + ent_bytes + k_sum * 4 + 4, st));
    uint8_t *base = (uint8_t *)tab.ptr;
    const int4 *d_ent = (const int4 *)(base + rec_bytes);
    uint32_t *d_pal = (uint32_t *)(base + rec_bytes + ent_bytes);
    const uintptr_t out_mask = form == kErrorIndex8 ? 3u : (form == kErrorIndex16 ? 7u : 15u);
    std::vector<BatchErrorImage> rec(n_images);
    size_t before = 0;
    for (uint32_t i = 0; i < n_images; ++i) {
        BatchErrorImage &r = rec[i];
        r.src = (const uint32_t *)d_src[i];
        r.out = d_out[i];
        r.entries = indexed ? d_ent + before : nullptr;
        r.pal = indexed ? d_pal + before : nullptr;
        r.stats = reinterpret_cast<unsigned long long *>(d_stats + i);
        r.n = (uint32_t)n_pixels[i];
        r.first_wg = first_wg[i];
        r.k = indexed ? ks[i] : 0u;
        r.aligned = ((reinterpret_cast<uintptr_t>(r.src) & 15u) == 0 && (reinterpret_cast<uintptr_t>(r.out) & out_mask) == 0) ? 1u : 0u;
        before += r.k;
    }
    HIP_TRY(upload_host_copy(base, rec.data(), sizeof(BatchErrorImage) * (size_t)n_images, st));
    if (indexed) {
        HIP_TRY(upload_host_copy(d_pal, palettes, k_sum * 4, st));
        // (the q triples of every palette: one launch over the concatenated words)
        if (lab) HIP_TRY(launch_error_palette(d_pal, (uint32_t)k_sum, p->d_lut, base + rec_bytes, st));
    }
    for (const BatchLaunch &cut : batch_launches(grid)) {
        const BatchErrorImage *d_rec = (const BatchErrorImage *)base;
        HIP_TRY(launch_batch_error(form, what, d_rec, n_images, cut, k_max, cutoff, p->d_lut, st));
        if (launches) ++*launches;
    }
    return KMG_OK;
}

}  // namespace kmg

extern "C" int kmg_dev_compare_batch(kmg_processor *p, uint32_t n_images, const uint8_t *const *d_src_rgba, const void *const *d_out,
                                     const uint64_t *n_pixels, int format, const uint8_t *palettes_rgba, const uint32_t *ks,
                                     uint32_t alpha_cutoff, uint32_t what, kmg_error_stats *d_stats, void *stream)
try {
    // the refusals, for the whole batch, before any device work (the order is part of the contract: include/kmeans_hip.h)
    if (!p) return fail(KMG_ERR_INVALID_ARGUMENT, "processor is NULL");
    if (n_images == 0) return fail(KMG_ERR_INVALID_ARGUMENT, "the batch is empty");
    if (!d_src_rgba || !d_out || !n_pixels || !d_stats) return fail(KMG_ERR_INVALID_ARGUMENT, "a batch array is NULL");
    KMG_TRY(check_format(format));
    if (what == 0 || (what & ~(KMG_ERROR_RGB | KMG_ERROR_LAB))) return fail(KMG_ERR_INVALID_ARGUMENT, "what = %u: KMG_ERROR_RGB | KMG_ERROR_LAB", what);
    if (alpha_cutoff > 255u) return fail(KMG_ERR_INVALID_ARGUMENT, "alpha cutoff %u is above 255", alpha_cutoff);
    if (format != KMG_FORMAT_RGBA8 && (!palettes_rgba || !ks)) return fail(KMG_ERR_INVALID_ARGUMENT, "an index format needs the palettes and their counts");
    for (uint32_t i = 0; i < n_images; ++i) {
        if (!d_src_rgba[i] || !d_out[i]) return fail(KMG_ERR_INVALID_ARGUMENT, "image %u: image or output pointer is NULL", i);
        if (n_pixels[i] == 0) return fail(KMG_ERR_INVALID_ARGUMENT, "image %u has no pixel", i);
        KMG_TRY(check_pixel_count(n_pixels[i]));
        if (format == KMG_FORMAT_RGBA8) continue;
        if (ks[i] == 0 || ks[i] > KMG_MAX_K) return fail(KMG_ERR_INVALID_ARGUMENT, "image %u: an index format needs a palette of 1 .. %u colours", i, KMG_MAX_K);
        KMG_TRY(check_index8_room(format == KMG_FORMAT_INDEX8, "k", ks[i], alpha_cutoff != 0));
        if (format == KMG_FORMAT_INDEX16 && (reinterpret_cast<uintptr_t>(d_out[i]) & 1u))
            return fail(KMG_ERR_INVALID_ARGUMENT, "image %u: INDEX16 output is not 2-byte aligned", i);
    }
    if (reinterpret_cast<uintptr_t>(d_stats) & 7u) return fail(KMG_ERR_INVALID_ARGUMENT, "the statistics records are not 8-byte aligned");
    HIP_TRY(hipSetDevice(p->device));
    return dev_compare_batch(p, n_images, d_src_rgba, d_out, n_pixels, format, palettes_rgba, ks, alpha_cutoff, what, d_stats, S(stream), nullptr);
}
KMG_ABI_CATCH
