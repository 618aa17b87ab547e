// kmg_batch_apply.hip -- the output pass of many small images in one launch: the segmented version of the per-pixel output pass
// k_apply<PPT, DITHER, CHUNKED, ALPHA, OutT, BayerOffsets> of kmg_kernels.hip (replace and dither with the reference's matrix; RGBA8,
// INDEX8, INDEX16; alpha mode on and off; the chunked scan from k = 32) and kmg_dev_apply_batch on top of it (include/kmeans_hip.h at kmg_batch_apply_report).
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

#include <functional>

#include "kmg_apply_dev.h"
#include "kmg_apply_route.h"
#include "kmg_batch_layout.h"

namespace kmg {

// One image of a batched output launch.  cent / pal: the image's centroid table and palette words (k + 1: the dither sentinel's
// behind them), shared by all images or one per image.  aligned: what k_apply takes as `aligned` for this image's pointers (bit 0;
// index formats: the alpha cutoff in bits 8..15).  k: the image's own colour count (kmg_dev_apply_batch_counts; the other calls
// fill in the same for every image).  mode_format (mode | format << 8) and alpha_cutoff are common to the launch.
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

// workgroup wg0 + blockIdx.x of the batch's grid: one tile of its image.  ONE (a dither launch whose images have counts of their
// own, one of them k = 1): such an image is not dithered (mix_colors.wgsl:104-108) -- its workgroups, uniformly, take the replace pass.
template <int PPT, bool DITHER, bool CHUNKED, bool ALPHA, typename OutT, bool ONE = false>
__global__ __launch_bounds__(kBlock) void k_batch_apply(const BatchApplyImage *__restrict__ img, uint32_t n_images, uint32_t wg0,
                                                        const float *__restrict__ lut)
{
    static_assert(!ONE || (DITHER && !CHUNKED), "ONE: a dither launch below k = 32");
    const uint32_t wg = wg0 + blockIdx.x;
    const BatchApplyImage im = img[batch_image_of(img, n_images, wg)];
    if (ONE && im.k == 1u) {
        apply_tiles<PPT, false, false, ALPHA, OutT>(im.rgba, im.w, (uint64_t)im.n, 0u, im.cent, im.k, lut, im.pal, im.threshold,
                                                    static_cast<OutT *>(im.out), (int)im.aligned, (uint64_t)(wg - im.first_wg),
                                                    0x100000000ull);
        return;
    }
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

// k: the largest count of the launch's images (all below 32, or all from 32 on); one: dither, and an image of the launch has k = 1
template <int PPT>
hipError_t launch_batch_apply(const BatchApplyImage *rec, uint32_t m, kmg::BatchLaunch cut, uint32_t k, const float *lut, bool dither,
                              bool alpha, bool one, int format, hipStream_t st)
{
    const uint32_t kpad = (k + 3u) & ~3u;
    const bool chunked = k >= 32;
    const size_t lds = sizeof(float4) * kpad + (256 + 16) * sizeof(float);
    const bool known = with_out_type(format, [&](auto t) { with_bool(alpha, [&](auto A) {
        using OutT = typename decltype(t)::type;
        if (one) {
            hipLaunchKernelGGL((k_batch_apply<PPT, true, false, A(), OutT, true>), dim3(cut.count), dim3(kBlock), lds, st, rec, m, cut.first, lut);
            return;
        }
        with_bool(dither, [&](auto D) { with_bool(chunked, [&](auto C) {
            hipLaunchKernelGGL((k_batch_apply<PPT, D(), C(), A(), OutT>), dim3(cut.count), dim3(kBlock), lds, st, rec, m, cut.first, lut);
        }); });
    }); });
    return known ? hipGetLastError() : hipErrorInvalidValue;
}

// Images idx[0 .. m) of the caller's arrays through ONE chain of the batched kernel (their counts all below 32, or all from 32
// on): records and tables in one block of the processor, one upload, the launches.  Image i has ks[i] colours and the table at
// c4[at[i]]; shared: one table for all (that of idx[0]).  Only enqueues; *blk holds the block until the caller has drained the stream.
int batch_apply_run(kmg_processor *p, const uint32_t *idx, uint32_t m, const uint8_t *const *d_src, const uint32_t *widths,
                    const uint32_t *heights, const float *c4, const size_t *at, const uint32_t *ks, bool shared, int mode, int format,
                    uint32_t cutoff, void *const *d_out, uint32_t *launches, ArenaGuard *blk, hipStream_t st)
{
    const int ppt = batch_apply_ppt();
    std::vector<uint64_t> pixels(m);
    for (uint32_t q = 0; q < m; ++q) pixels[q] = (uint64_t)widths[idx[q]] * heights[idx[q]];
    std::vector<uint32_t> first_wg;
    uint64_t grid = 0;
    if (!batch_grid(pixels.data(), m, (uint64_t)kBlock * ppt, first_wg, &grid))
        return fail(KMG_ERR_UNSUPPORTED, "the batch has more than 2^32-1 tiles");

    // the block: [records][table 0: k centroids, k + 1 palette words][table 1] ... -- each table by its own k
    const uint32_t tables = shared ? 1u : m;
    const size_t rec_bytes = pad256(sizeof(BatchApplyImage) * (size_t)m);
    std::vector<size_t> table_at(tables + 1u, rec_bytes);
    uint32_t k = 0;                                                    // the largest count: the launch's LDS
    bool dither = false, one = false;                                  // mix_colors.wgsl:104-108: an image with k = 1 is not dithered
    for (uint32_t q = 0; q < m; ++q) {
        const uint32_t kq = ks[idx[q]];
        if (q < tables) table_at[q + 1u] = table_at[q] + pad256(sizeof(Centroid) * (size_t)kq + sizeof(uint32_t) * ((size_t)kq + 1));
        k = std::max(k, kq);
        if (mode == KMG_MODE_DITHER) (kq > 1 ? dither : one) = true;
    }
    one = one && dither;
    const size_t bytes = table_at[tables];
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
        const uint32_t kt = ks[idx[t]];
        const float *mine = c4 + at[idx[t]];
        Centroid *hc = (Centroid *)(host.data() + table_at[t]);
        uint8_t *pal = (uint8_t *)hc + sizeof(Centroid) * (size_t)kt;
        for (uint32_t i = 0; i < kt; ++i) hc[i] = {mine[4 * i], mine[4 * i + 1], mine[4 * i + 2], chroma(mine[4 * i + 1], mine[4 * i + 2])};
        for (uint32_t i = 0; i <= kt; ++i) shader_lab_to_rgba8(i < kt ? mine + 4 * i : sentinel, pal + 4 * i);
        thr[t] = mode == KMG_MODE_DITHER && kt > 1 ? dither_threshold(mine, kt) : 0.0f;
    }
    BatchApplyImage *rec = (BatchApplyImage *)host.data();
    for (uint32_t q = 0; q < m; ++q) {
        const uint32_t t = shared ? 0u : q;
        BatchApplyImage &r = rec[q];
        r.rgba = (const uint32_t *)d_src[idx[q]];
        r.out = d_out[idx[q]];
        r.cent = (const Centroid *)(base + table_at[t]);
        r.pal = (const uint32_t *)((const uint8_t *)r.cent + sizeof(Centroid) * (size_t)ks[idx[q]]);
        r.n = (uint32_t)pixels[q];
        r.w = widths[idx[q]];
        r.first_wg = first_wg[q];
        r.threshold = thr[t];
        with_out_type(format, [&](auto t) { r.aligned = (uint32_t)output_flags<typename decltype(t)::type>(r.rgba, r.out, cutoff); });
        r.k = ks[idx[q]];
        r.mode_format = (uint32_t)mode | ((uint32_t)format << 8);
        r.alpha_cutoff = cutoff;
    }
    HIP_TRY(upload_host_copy(base, host.data(), bytes, st));
    for (const BatchLaunch &cut : batch_launches(grid)) {
#ifdef KMG_TOOLS
        if (ppt != kBatchApplyPPT) {
            HIP_TRY(launch_batch_apply<12 - kBatchApplyPPT>((const BatchApplyImage *)base, m, cut, k, p->d_lut, dither, cutoff != 0, one, format, st));
            ++*launches;
            continue;
        }
#endif
        HIP_TRY(launch_batch_apply<kBatchApplyPPT>((const BatchApplyImage *)base, m, cut, k, p->d_lut, dither, cutoff != 0, one, format, st));
        ++*launches;
    }
    return KMG_OK;
}

}  // namespace

int kmg::apply_batch_counts(kmg_processor *p, uint32_t n_images, const uint8_t *const *d_src, const uint32_t *widths, const uint32_t *heights,
                            const float *c4, const size_t *at, const uint32_t *ks, bool shared, int mode, int format, uint32_t cutoff,
                            void *const *d_out, kmg_batch_apply_report *report, hipStream_t st, int filter, const DitherPtr *dither)
{
    // the diffusion filter: the processor's switch as it is when the call starts, for every per-image pass of the call
    if (filter < 0) filter = p->diffusion.load(std::memory_order_relaxed);
    // the dither choice likewise.  The batched kernel carries the reference's matrix: with any other choice the dither images take
    // their own pass, as meld and diffusion images do (a batched map kernel: DESIGN.md 7)
    const DitherPtr choice = dither ? *dither : dither_snapshot(p);
    const bool mapped = mode == KMG_MODE_DITHER && choice != nullptr;
    // which images join a launch (kmg_apply_route.h), each asked with its own k: the others take their own output pass, after the
    // launches are on their way.  The chunked scan is a launch's: the joined images below k = 32 go out as one chain, the others
    // as a second.
    const int forced = forced_strategy(p);
    const bool mask_words_only = (p->strategy.load(std::memory_order_relaxed) & KMG_STRATEGY_MASK_WORDS) != 0;
    std::vector<uint32_t> joined[2], alone;
    for (uint32_t i = 0; i < n_images; ++i)
        (!mapped && batch_apply_joins(mode, ks[i], (uint64_t)widths[i] * heights[i], forced, mask_words_only, n_images) ? joined[ks[i] >= 32u ? 1 : 0] : alone)
            .push_back(i);
    ArenaGuard blk[2];
    uint32_t launches = 0;
    for (int c = 0; c < 2; ++c)
        if (!joined[c].empty())
            KMG_TRY_DRAIN(st, batch_apply_run(p, joined[c].data(), (uint32_t)joined[c].size(), d_src, widths, heights, c4, at, ks, shared, mode,
                                              format, cutoff, d_out, &launches, &blk[c], st));
    for (const uint32_t i : alone)
        KMG_TRY_DRAIN(st, dev_apply(p, d_src[i], widths[i], heights[i], 0, c4 + at[i], ks[i], mode, (uint8_t *)d_out[i], st, cutoff, format, filter, &choice));
    HIP_TRY(hipStreamSynchronize(st));                                 // (the blocks are idle again)
    if (report) {
        report->launches += launches;
        report->batched += (uint32_t)(joined[0].size() + joined[1].size());
        report->per_image += (uint32_t)alone.size();
    }
    return KMG_OK;
}

// (the case where every table has k colours: n_tables = 1, one table for all images, or one per image)
int kmg::apply_batch(kmg_processor *p, uint32_t n_images, const uint8_t *const *d_src, const uint32_t *widths, const uint32_t *heights,
                     const float *c4, uint32_t n_tables, uint32_t k, int mode, int format, uint32_t cutoff, void *const *d_out,
                     kmg_batch_apply_report *report, hipStream_t st, int filter, const DitherPtr *dither)
{
    const std::vector<uint32_t> ks(n_images, k);
    std::vector<size_t> at(n_images, 0);
    for (uint32_t i = 0; n_tables != 1 && i < n_images; ++i) at[i] = 4ull * k * i;
    return apply_batch_counts(p, n_images, d_src, widths, heights, c4, at.data(), ks.data(), n_tables == 1, mode, format, cutoff, d_out, report, st, filter, dither);
}

// The outputs of apply_batch / apply_batch_counts in one stream-ordered block, then to the host
namespace {

int batch_download(kmg_processor *p, uint32_t n_images, const uint32_t *widths, const uint32_t *heights, int format, uint8_t *const *out,
                   hipStream_t st, const std::function<int(void *const *)> &apply)
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
    KMG_TRY(apply(d_out.data()));
    for (uint32_t i = 0; i < n_images; ++i)
        HIP_TRY_DRAIN(st, copy_host_image(p, out[i], d_out[i], (size_t)pixels[i] * bpp, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return KMG_OK;
}

}  // namespace

int kmg::apply_batch_download(kmg_processor *p, uint32_t n_images, const uint8_t *const *d_src, const uint32_t *widths,
                              const uint32_t *heights, const float *c4, uint32_t n_tables, uint32_t k, int mode, int format, uint32_t cutoff,
                              uint8_t *const *out, kmg_batch_apply_report *report, hipStream_t st)
{
    return batch_download(p, n_images, widths, heights, format, out, st, [&](void *const *d_out) {
        return apply_batch(p, n_images, d_src, widths, heights, c4, n_tables, k, mode, format, cutoff, d_out, report, st);
    });
}

int kmg::apply_batch_counts_download(kmg_processor *p, uint32_t n_images, const uint8_t *const *d_src, const uint32_t *widths,
                                     const uint32_t *heights, const float *c4, const size_t *at, const uint32_t *ks, int mode, int format,
                                     uint32_t cutoff, uint8_t *const *out, kmg_batch_apply_report *report, hipStream_t st)
{
    return batch_download(p, n_images, widths, heights, format, out, st, [&](void *const *d_out) {
        return apply_batch_counts(p, n_images, d_src, widths, heights, c4, at, ks, false, mode, format, cutoff, d_out, report, st);
    });
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

extern "C" int kmg_dev_apply_batch_counts(kmg_processor *p, uint32_t n_images, const uint8_t *const *d_rgba, const uint32_t *widths,
                                          const uint32_t *heights, const float *centroids4, const uint32_t *ks, int mode, int format,
                                          void *const *d_out, kmg_batch_apply_report *report, void *stream)
try {
    // the refusals of kmg_dev_apply_batch, image by image with its own count
    KMG_TRY(check_batch_prefix(p, n_images, !d_rgba || !widths || !heights || !centroids4 || !ks || !d_out, "a batch array is NULL", d_rgba, widths,
                               heights, d_out));
    for (uint32_t i = 0; i < n_images; ++i) KMG_TRY(check_k_nonzero(ks[i]));
    KMG_TRY(check_mode(mode));
    KMG_TRY(check_format(format));
    for (uint32_t i = 0; i < n_images; ++i) KMG_TRY(check_k_limit(ks[i]));
    const uint32_t cutoff = p->alpha_cutoff.load(std::memory_order_relaxed);
    std::vector<size_t> at(n_images, 0);
    for (uint32_t i = 1; i < n_images; ++i) at[i] = at[i - 1] + 4ull * ks[i - 1];
    if (format != KMG_FORMAT_RGBA8)
        for (uint32_t i = 0; i < n_images; ++i) KMG_TRY(check_index_format(centroids4 + at[i], ks[i], mode, format, cutoff));
    if (format == KMG_FORMAT_INDEX16)
        for (uint32_t i = 0; i < n_images; ++i)
            if (reinterpret_cast<uintptr_t>(d_out[i]) & 1u) return fail(KMG_ERR_INVALID_ARGUMENT, "image %u: INDEX16 output must be 2-byte aligned", i);
    HIP_TRY(hipSetDevice(p->device));
    kmg_batch_apply_report rep = {0u, 0u, 0u, 1u};
    KMG_TRY(apply_batch_counts(p, n_images, d_rgba, widths, heights, centroids4, at.data(), ks, false, mode, format, cutoff, d_out, &rep, S(stream)));
    if (report) *report = rep;
    return KMG_OK;
}
KMG_ABI_CATCH
