// kmg_batch_apply.hip -- the output pass of many small images in one launch: the segmented version of the per-pixel output pass
// k_apply<PPT, DITHER, CHUNKED, ALPHA, OutT> of kmg_kernels.hip (replace and dither; RGBA8, INDEX8, INDEX16; alpha mode on and off;
// the chunked scan from k = 32) and kmg_dev_apply_batch on top of it (include/kmeans_hip.h at kmg_batch_apply_report).
//
// A launch reads a table of BatchApplyImage records in device memory, one per image.  Its grid is the sum of the images' tiles
// (kBlock * PPT pixels each); a workgroup finds its image by the bounded binary search over the records' first-workgroup column
// (batch_image_of, kmg_device.h) and then runs the per-image pass on ONE tile of that image (apply_tiles, kmg_apply_dev.h: the
// arithmetic of k_apply, operation for operation) with the image's own width, pixel count, threshold and tables, row0 = 0.  Pixels
// are independent, so every image gets the bytes the per-image call gives it.
//
// Synchronisation: the launch boundary, nothing else.  No workgroup waits for another, every loop has a bound known at launch,
// nothing is launched cooperatively.  More workgroups than kBatchMaxGrid run as several launches over the same records.
//
// Compile with -ffp-contract=off: arithmetic must match kmg_math.h operation for operation.

#include "kmg_state.h"

#include "kmg_apply_dev.h"
#include "kmg_apply_route.h"
#include "kmg_batch_layout.h"

namespace kmg {

// One image of a batched output launch.  cent / pal: the image's centroid table and palette words (k + 1: the dither sentinel's
// behind them), shared by all images or one per image.  aligned: what k_apply takes as `aligned` for this image's pointers (bit 0;
// index formats: the alpha cutoff in bits 8..15).  k, mode_format (mode | format << 8) and alpha_cutoff are common to the launch.
struct alignas(16) BatchApplyImage {
    const uint32_t *rgba;          // n pixels
    void *out;                     // n outputs of the launch's format
    const Centroid *cent;          // k
    const uint32_t *pal;           // k + 1
    uint32_t n;                    // pixels
    uint32_t w;                    // width: the Bayer index is that of the image's own coordinates
    uint32_t first_wg;             // index of the image's first workgroup in the grid
    float threshold;               // dither threshold of the image's table
    uint32_t aligned;
    uint32_t k;
    uint32_t mode_format;
    uint32_t alpha_cutoff;
};
static_assert(sizeof(BatchApplyImage) == 64, "BatchApplyImage layout");

// workgroup wg0 + blockIdx.x of the batch's grid: one tile of its image
template <int PPT, bool DITHER, bool CHUNKED, bool ALPHA, typename OutT>
__global__ __launch_bounds__(kBlock) void k_batch_apply(const BatchApplyImage *__restrict__ img, uint32_t n_images, uint32_t wg0,
                                                        const float *__restrict__ lut)
{
    const uint32_t wg = wg0 + blockIdx.x;
    const BatchApplyImage im = img[batch_image_of(img, n_images, wg)];
    // (one tile: the stride leaves the image)
    apply_tiles<PPT, DITHER, CHUNKED, ALPHA, OutT>(im.rgba, im.w, (uint64_t)im.n, 0u, im.cent, im.k, lut, im.pal, im.threshold,
                                                   static_cast<OutT *>(im.out), (int)im.aligned, (uint64_t)(wg - im.first_wg),
                                                   0x100000000ull);
}

}  // namespace kmg

namespace {

// pixels per thread of the batched output pass: 4 (tiles of 1024 pixels), or 8, the per-image pass's.  Measured on the batches of
// tools/batch_probe.py (the `ppt 4/8` rows of profiles/r10_batch_apply_time.txt): 4 takes 0.85 - 1.03 of 8, 0.87 -
// 0.96 at k = 64.  The tools build takes the other from the environment.
constexpr int kBatchApplyPPT = 4;

int batch_apply_ppt()
{
    const int ppt = tools_env_int(KMG_TOOLS_ENV("KMG_BATCH_APPLY_PPT"), kBatchApplyPPT);
    return ppt == 4 || ppt == 8 ? ppt : kBatchApplyPPT;
}

template <int PPT, typename OutT>
void launch_batch_apply_t(const BatchApplyImage *rec, uint32_t m, kmg::BatchLaunch cut, uint32_t k, const float *lut, bool dither, bool alpha,
                          hipStream_t st)
{
    const uint32_t kpad = (k + 3u) & ~3u;
    const bool chunked = k >= 32;
    const size_t lds = sizeof(float4) * kpad + (256 + 16) * sizeof(float);
#define KMG_BATCH_APPLY(D, C, A) \
    hipLaunchKernelGGL((k_batch_apply<PPT, D, C, A, OutT>), dim3(cut.count), dim3(kBlock), lds, st, rec, m, cut.first, lut)
    if (alpha) {
        if (dither) { if (chunked) KMG_BATCH_APPLY(true, true, true); else KMG_BATCH_APPLY(true, false, true); }
        else        { if (chunked) KMG_BATCH_APPLY(false, true, true); else KMG_BATCH_APPLY(false, false, true); }
    } else {
        if (dither) { if (chunked) KMG_BATCH_APPLY(true, true, false); else KMG_BATCH_APPLY(true, false, false); }
        else        { if (chunked) KMG_BATCH_APPLY(false, true, false); else KMG_BATCH_APPLY(false, false, false); }
    }
#undef KMG_BATCH_APPLY
}

template <int PPT>
hipError_t launch_batch_apply(const BatchApplyImage *rec, uint32_t m, kmg::BatchLaunch cut, uint32_t k, const float *lut, bool dither,
                              bool alpha, int format, hipStream_t st)
{
    if (format == KMG_FORMAT_INDEX8) launch_batch_apply_t<PPT, uint8_t>(rec, m, cut, k, lut, dither, alpha, st);
    else if (format == KMG_FORMAT_INDEX16) launch_batch_apply_t<PPT, uint16_t>(rec, m, cut, k, lut, dither, alpha, st);
    else launch_batch_apply_t<PPT, uint32_t>(rec, m, cut, k, lut, dither, alpha, st);
    return hipGetLastError();
}

// what k_apply's launchers pass as `aligned` for (src, out) in `format` (kmg_kernels.hip launch_apply / launch_apply_index_t)
uint32_t aligned_word(const void *src, const void *out, int format, uint32_t cutoff)
{
    if (format == KMG_FORMAT_INDEX8) return (uint32_t)output_aligned<uint8_t>(src, out) | ((cutoff & 255u) << 8);
    if (format == KMG_FORMAT_INDEX16) return (uint32_t)output_aligned<uint16_t>(src, out) | ((cutoff & 255u) << 8);
    return (uint32_t)output_aligned<uint32_t>(src, out);
}

// The joined images idx[0 .. m) of the caller's arrays through the batched kernel: records and tables in one block of the
// processor, one upload, the launches.  Only enqueues; *blk holds the block until the caller has drained the stream.
int batch_apply_run(kmg_processor *p, const uint32_t *idx, uint32_t m, const uint8_t *const *d_src, const uint32_t *widths,
                    const uint32_t *heights, const float *c4, uint32_t n_tables, uint32_t k, int mode, int format, uint32_t cutoff,
                    void *const *d_out, uint32_t *launches, ArenaGuard *blk, hipStream_t st)
{
    const int ppt = batch_apply_ppt();
    const bool dither = mode == KMG_MODE_DITHER && k > 1;              // mix_colors.wgsl:104-108
    std::vector<uint64_t> pixels(m);
    for (uint32_t q = 0; q < m; ++q) pixels[q] = (uint64_t)widths[idx[q]] * heights[idx[q]];
    std::vector<uint32_t> first_wg;
    uint64_t grid = 0;
    if (!batch_grid(pixels.data(), m, (uint64_t)kBlock * ppt, first_wg, &grid))
        return fail(KMG_ERR_UNSUPPORTED, "the batch has more than 2^32-1 tiles");

    // the block: [records][table 0: k centroids, k + 1 palette words][table 1] ...
    const uint32_t tables = n_tables == 1 ? 1u : m;
    const size_t rec_bytes = pad256(sizeof(BatchApplyImage) * (size_t)m);
    const size_t cent_bytes = sizeof(Centroid) * (size_t)k, table_bytes = pad256(cent_bytes + sizeof(uint32_t) * ((size_t)k + 1));
    const size_t bytes = rec_bytes + table_bytes * tables;
    {
        const hipError_t e = blk->acquire(p, bytes);
        if (e != hipSuccess) { blk->base = nullptr; return fail_hip(e, "batch output tables allocation"); }
    }
    uint8_t *base = (uint8_t *)blk->base;
    std::vector<uint8_t> host(bytes, 0);
    std::vector<float> thr(tables);
    const float sentinel[3] = {10000.0f, 10000.0f, 10000.0f};
    for (uint32_t t = 0; t < tables; ++t) {
        // per-centroid work on the host, as a plan does it (kmg_apply.hip plan_create)
        const float *mine = c4 + (n_tables == 1 ? 0 : 4ull * k * idx[t]);
        Centroid *hc = (Centroid *)(host.data() + rec_bytes + table_bytes * t);
        uint8_t *pal = (uint8_t *)hc + cent_bytes;
        for (uint32_t i = 0; i < k; ++i) hc[i] = {mine[4 * i], mine[4 * i + 1], mine[4 * i + 2], chroma(mine[4 * i + 1], mine[4 * i + 2])};
        for (uint32_t i = 0; i <= k; ++i) shader_lab_to_rgba8(i < k ? mine + 4 * i : sentinel, pal + 4 * i);
        thr[t] = dither ? dither_threshold(mine, k) : 0.0f;
    }
    BatchApplyImage *rec = (BatchApplyImage *)host.data();
    for (uint32_t q = 0; q < m; ++q) {
        const uint32_t t = n_tables == 1 ? 0u : q;
        BatchApplyImage &r = rec[q];
        r.rgba = (const uint32_t *)d_src[idx[q]];
        r.out = d_out[idx[q]];
        r.cent = (const Centroid *)(base + rec_bytes + table_bytes * t);
        r.pal = (const uint32_t *)((const uint8_t *)r.cent + cent_bytes);
        r.n = (uint32_t)pixels[q];
        r.w = widths[idx[q]];
        r.first_wg = first_wg[q];
        r.threshold = thr[t];
        r.aligned = aligned_word(r.rgba, r.out, format, cutoff);
        r.k = k;
        r.mode_format = (uint32_t)mode | ((uint32_t)format << 8);
        r.alpha_cutoff = cutoff;
    }
    HIP_TRY(upload_host_copy(base, host.data(), bytes, st));
    for (const BatchLaunch &cut : batch_launches(grid)) {
#ifdef KMG_TOOLS
        if (ppt != kBatchApplyPPT) {
            HIP_TRY(launch_batch_apply<12 - kBatchApplyPPT>((const BatchApplyImage *)base, m, cut, k, p->d_lut, dither, cutoff != 0, format, st));
            ++*launches;
            continue;
        }
#endif
        HIP_TRY(launch_batch_apply<kBatchApplyPPT>((const BatchApplyImage *)base, m, cut, k, p->d_lut, dither, cutoff != 0, format, st));
        ++*launches;
    }
    return KMG_OK;
}

}  // namespace

int kmg::apply_batch(kmg_processor *p, uint32_t n_images, const uint8_t *const *d_src, const uint32_t *widths, const uint32_t *heights,
                     const float *c4, uint32_t n_tables, uint32_t k, int mode, int format, uint32_t cutoff, void *const *d_out,
                     kmg_batch_apply_report *report, hipStream_t st)
{
    // which images join the launch (kmg_apply_route.h): the others take their own output pass, after the launch is on its way
    const int forced = forced_strategy(p);
    const bool mask_words_only = (p->strategy.load(std::memory_order_relaxed) & KMG_STRATEGY_MASK_WORDS) != 0;
    std::vector<uint32_t> joined, alone;
    for (uint32_t i = 0; i < n_images; ++i)
        (batch_apply_joins(mode, k, (uint64_t)widths[i] * heights[i], forced, mask_words_only, n_images) ? joined : alone).push_back(i);
    ArenaGuard blk;
    uint32_t launches = 0;
    if (!joined.empty())
        KMG_TRY_DRAIN(st, batch_apply_run(p, joined.data(), (uint32_t)joined.size(), d_src, widths, heights, c4, n_tables, k, mode, format, cutoff,
                                          d_out, &launches, &blk, st));
    for (const uint32_t i : alone)
        KMG_TRY_DRAIN(st, dev_apply(p, d_src[i], widths[i], heights[i], 0, c4 + (n_tables == 1 ? 0 : 4ull * k * i), k, mode, (uint8_t *)d_out[i], st,
                                    cutoff, format));
    HIP_TRY(hipStreamSynchronize(st));                                 // (the block is idle again)
    if (report) {
        report->launches += launches;
        report->batched += (uint32_t)joined.size();
        report->per_image += (uint32_t)alone.size();
    }
    return KMG_OK;
}

int kmg::apply_batch_download(kmg_processor *p, uint32_t n_images, const uint8_t *const *d_src, const uint32_t *widths,
                              const uint32_t *heights, const float *c4, uint32_t n_tables, uint32_t k, int mode, int format, uint32_t cutoff,
                              uint8_t *const *out, kmg_batch_apply_report *report, hipStream_t st)
{
    const uint32_t bpp = format_bytes(format);
    std::vector<uint64_t> pixels(n_images), offset;
    for (uint32_t i = 0; i < n_images; ++i) pixels[i] = (uint64_t)widths[i] * heights[i];
    uint64_t total = 0;
    if (!batch_offsets(pixels.data(), n_images, bpp, offset, &total, (uint64_t)SIZE_MAX / 2))
        return fail(KMG_ERR_OUT_OF_MEMORY, "the outputs of the sub-batch do not fit one block");
    StreamBuf block;
    HIP_TRY(block.alloc(p, (size_t)total, st));
    std::vector<void *> d_out(n_images);
    for (uint32_t i = 0; i < n_images; ++i) d_out[i] = (uint8_t *)block.ptr + offset[i];
    KMG_TRY(apply_batch(p, n_images, d_src, widths, heights, c4, n_tables, k, mode, format, cutoff, d_out.data(), report, st));
    for (uint32_t i = 0; i < n_images; ++i)
        HIP_TRY_DRAIN(st, copy_host_image(p, out[i], d_out[i], (size_t)pixels[i] * bpp, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return KMG_OK;
}

extern "C" int kmg_dev_apply_batch(kmg_processor *p, uint32_t n_images, const uint8_t *const *d_rgba, const uint32_t *widths,
                                   const uint32_t *heights, const float *centroids4, uint32_t n_tables, uint32_t k, int mode, int format,
                                   void *const *d_out, kmg_batch_apply_report *report, void *stream)
try {
    // the refusals, for the whole batch, before any device work (the order is part of the contract: include/kmeans_hip.h)
    KMG_TRY(check_batch_prefix(p, n_images, !d_rgba || !widths || !heights || !centroids4 || !d_out, "a batch array is NULL", d_rgba, widths, heights, d_out));
    KMG_TRY(check_k_nonzero(k));
    KMG_TRY(check_mode(mode));
    KMG_TRY(check_format(format));
    KMG_TRY(check_k_limit(k));
    const uint32_t cutoff = p->alpha_cutoff.load(std::memory_order_relaxed);
    // (the index formats' rules table by table, over the tables the caller says it has -- n_tables itself is judged after them)
    if (format != KMG_FORMAT_RGBA8)
        for (uint32_t t = 0; t < std::max(1u, std::min(n_tables, n_images)); ++t)
            KMG_TRY(check_index_format(centroids4 + 4ull * k * t, k, mode, format, cutoff));
    if (n_tables != 1 && n_tables != n_images)
        return fail(KMG_ERR_INVALID_ARGUMENT, "n_tables = %u: 1 (one table for all images) or n_images = %u", n_tables, n_images);
    if (format == KMG_FORMAT_INDEX16)
        for (uint32_t i = 0; i < n_images; ++i)
            if (reinterpret_cast<uintptr_t>(d_out[i]) & 1u) return fail(KMG_ERR_INVALID_ARGUMENT, "image %u: INDEX16 output must be 2-byte aligned", i);
    HIP_TRY(hipSetDevice(p->device));
    kmg_batch_apply_report rep = {0u, 0u, 0u, 1u};
    KMG_TRY(apply_batch(p, n_images, d_rgba, widths, heights, centroids4, n_tables, k, mode, format, cutoff, d_out, &rep, S(stream)));
    if (report) *report = rep;
    return KMG_OK;
}
KMG_ABI_CATCH
