// kmg_api.hip -- the host-buffer calls of the C ABI (include/kmeans_hip.h): ImageProcessor::{palette, find, reduce}
// (core/src/lib.rs:67-164) -- argument checking (the shared checks: kmg_checks.h), upload, the host sequencing of operations.rs on
// top of kmg_lloyd_* / kmg_dev_apply, download.  A call starts with a CallStart; kmg_find / kmg_find_indexed and kmg_reduce /
// kmg_reduce_indexed are one body each; the palette / reduce batches are one BatchCall, a function per step (their cut rule and
// kmg_find_batch's: batch_cuts, kmg_batch_layout.h); the working image has one rule (working_enqueue, working_resolve).  There
// is no CPU data path in this file: every per-pixel step is a kernel launch.

#include "kmg_state.h"
#include "kmg_batch_layout.h"
#include "kmg_quality_search.h"

// ---------------------------------------------------------------------------------------------
// host-buffer API (ImageProcessor::{palette, find, reduce})
// ---------------------------------------------------------------------------------------------
namespace {

int check_image(const kmg_processor *p, const uint8_t *rgba, uint32_t w, uint32_t h)
{
    if (!p) return fail(KMG_ERR_INVALID_ARGUMENT, "processor is NULL");
    return check_image_buffer(rgba, w, h);
}

// The working image of the k-means palette step (operations.rs:15-88 extract_palette_kmeans before its loop): the image after the
// shrink, then -- alpha mode (alpha_cutoff != 0, include/kmeans_hip.h at kmg_options) -- its kept pixels, compacted in raster order,
// as an image of n_kept x 1 pixels, unless every pixel is kept.  Made once per call; the buffers live as long as the object.
// Alpha weighting (kmg_processor_set_weighting) composes here: the cutoff becomes max(alpha_cutoff, 1) -- a pixel of weight 0 is
// not kept -- and the compaction copies whole pixels, so the weights ride in the working image's alpha bytes.
// Made in two halves, so that a sub-batch reads the kept counts of its images back at once (BatchCall::stage_images):
// working_enqueue, then -- cutoff != 0, with the count read back from d_count -- working_resolve.
struct WorkingImage {
    StreamBuf small, kept;
    const uint8_t *src = nullptr;
    uint32_t sw = 0, sh = 0;
    int weighting = KMG_WEIGHT_NONE;
    uint32_t cutoff = 0;                 // the cutoff the compaction ran with; 0 = none ran, nothing to resolve
    uint64_t *d_count = nullptr;         // where the compaction leaves the number of kept pixels
};

// The enqueue half: the shrink (structures.rs:67-74) and the compaction on st, no synchronisation.  d_count: the device slot for
// the kept count, or NULL = one behind the kept pixels (256-byte aligned).  spent: the buffer of d_rgba where the caller needs it
// no longer once it is shrunk -- released as soon as the shrink is enqueued -- or NULL.
int working_enqueue(kmg_processor *p, const uint8_t *d_rgba, uint32_t w, uint32_t h, uint32_t alpha_cutoff, int weighting, hipStream_t st,
                    WorkingImage &wi, uint64_t *d_count = nullptr, StreamBuf *spent = nullptr)
{
    wi.cutoff = working_cutoff(alpha_cutoff, weighting); wi.weighting = weighting;
    wi.src = d_rgba; wi.sw = w; wi.sh = h;
    const uint32_t m = p->opt.shrink_max_dim;
    if (m && (w > m || h > m)) {
        kmg_resized_dims(w, h, m, &wi.sw, &wi.sh);
        HIP_TRY(wi.small.alloc(p, (size_t)wi.sw * wi.sh * 4, st));
        KMG_TRY(kmg_dev_resize(p, d_rgba, w, h, wi.sw, wi.sh, (uint8_t *)wi.small.ptr, st));
        wi.src = (const uint8_t *)wi.small.ptr;
        if (spent) {
            HIP_TRY(hipFreeAsync(spent->ptr, st));
            spent->ptr = nullptr;
        }
    }
    if (!wi.cutoff) return KMG_OK;
    const uint64_t n = (uint64_t)wi.sw * wi.sh;
    // (a count slot of the call's own lies behind the pixels, 256-byte aligned: room up to that boundary and for the slot --
    // n * 4 + 256 bytes ended 4 bytes inside the slot where n = 1 mod 64)
    HIP_TRY(wi.kept.alloc(p, d_count ? (size_t)n * 4 : pad256((size_t)n * 4) + 256u, st));
    wi.d_count = d_count ? d_count : (uint64_t *)((uint8_t *)wi.kept.ptr + pad256((size_t)n * 4));
    return kmg_dev_alpha_compact(p, wi.src, n, wi.cutoff, (uint8_t *)wi.kept.ptr, wi.d_count, st);
}

// The resolve half: with n_kept pixels kept, which buffer is the working image, and its shape.  false: the image is empty -- the
// caller refuses it in its own words.
bool working_resolve(WorkingImage &wi, uint64_t n_kept)
{
    if (n_kept && n_kept < (uint64_t)wi.sw * wi.sh) {
        wi.src = (const uint8_t *)wi.kept.ptr;
        wi.sw = (uint32_t)n_kept; wi.sh = 1;
    }
    return n_kept != 0;
}

int working_image(kmg_processor *p, const uint8_t *d_rgba, uint32_t w, uint32_t h, uint32_t alpha_cutoff, int weighting, hipStream_t st,
                  WorkingImage &wi)
{
    KMG_TRY(working_enqueue(p, d_rgba, w, h, alpha_cutoff, weighting, st, wi));
    if (wi.cutoff) {
        uint64_t n_kept = 0;
        HIP_TRY(hipMemcpyAsync(&n_kept, wi.d_count, sizeof n_kept, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (!working_resolve(wi, n_kept)) return fail(KMG_ERR_INVALID_ARGUMENT, "no pixel reaches alpha_cutoff = %u", wi.cutoff);
    }
    if (weighting && (uint64_t)wi.sw * wi.sh > kMaxWeightedPixels)
        return fail(KMG_ERR_UNSUPPORTED, "alpha weighting: the working image has %llu pixels, more than 2^28", (unsigned long long)((uint64_t)wi.sw * wi.sh));
    return KMG_OK;
}

}  // namespace

// operations.rs:15-88 extract_palette_kmeans on a working image -> host centroid table: a new Lloyd problem of k centroids.
// d_labels (optional): the u32 label of every pixel of the working image under the final centroids (find_centroid.wgsl:15-44, the
// label KMG_MODE_REPLACE gives the pixel).
int kmg::palette_of_working(kmg_processor *p, const uint8_t *src, uint32_t sw, uint32_t sh, uint32_t k, hipStream_t st, float *c4,
                            uint32_t *d_labels, const float *fixed4, uint32_t n_fixed, int weighting, uint32_t *iterations)
{
    LloydGuard g;
    if (weighting && (uint64_t)sw * sh > kMaxWeightedPixels)
        return fail(KMG_ERR_UNSUPPORTED, "alpha weighting: the working image has %llu pixels, more than 2^28", (unsigned long long)((uint64_t)sw * sh));
    if (n_fixed > k) return fail(KMG_ERR_INVALID_ARGUMENT, "k = %u is below the %u fixed colours of the processor", k, n_fixed);
    KMG_TRY(lloyd_create_impl(p, k, &g.s, st));
    KMG_TRY(kmg_lloyd_init_centroids_seeded(g.s, src, sw, sh, fixed4, n_fixed, st));   // operations.rs:73
    KMG_TRY(kmg_lloyd_set_fixed(g.s, n_fixed));
    // (after the initialisation, which is unweighted and may have bound the image: a weighted loop drops that binding)
    KMG_TRY(kmg_lloyd_set_weighting(g.s, weighting));
    if (log_debug()) {
        std::vector<float> c(4 * k);
        if (kmg_lloyd_get_centroids(g.s, c.data(), st) == KMG_OK) {
            fprintf(stderr, "[kmeans_hip] == Initial centroids: ==\n");
            for (uint32_t i = 0; i < k; ++i)
                fprintf(stderr, "[kmeans_hip] Centroid %u = [%g, %g, %g, %g]\n", i, c[4 * i], c[4 * i + 1], c[4 * i + 2], c[4 * i + 3]);
        }
    }
    uint32_t it = 0;
    KMG_TRY(kmg_lloyd_run(g.s, src, (uint64_t)sw * sh, nullptr, &it, st));  // operations.rs:85
    KMG_TRY(kmg_lloyd_get_centroids(g.s, c4, st));
    if (iterations) *iterations = it;
    if (log_debug()) {
        fprintf(stderr, "[kmeans_hip] == Final centroids at iteration %u: ==\n", it);
        for (uint32_t i = 0; i < k; ++i)
            fprintf(stderr, "[kmeans_hip] Centroid %u = [%g, %g, %g, %g]\n", i, c4[4 * i], c4[4 * i + 1], c4[4 * i + 2], c4[4 * i + 3]);
    }
    return d_labels ? kmg_lloyd_labels(g.s, src, (uint64_t)sw * sh, d_labels, st) : KMG_OK;
}

namespace {

typedef std::shared_ptr<const std::vector<float>> FixedList;

int palette_of_working(kmg_processor *p, const WorkingImage &wi, uint32_t k, hipStream_t st, float *c4, const FixedList &fixed,
                       uint32_t *d_labels = nullptr)
{
    return kmg::palette_of_working(p, wi.src, wi.sw, wi.sh, k, st, c4, d_labels, fixed ? fixed->data() : nullptr, fixed_count(fixed),
                                   wi.weighting);
}

int extract_palette_kmeans(kmg_processor *p, const uint8_t *d_rgba, uint32_t w, uint32_t h, uint32_t k, uint32_t alpha_cutoff,
                           int weighting, hipStream_t st, float *c4, const FixedList &fixed)
{
    WorkingImage wi;
    KMG_TRY(working_image(p, d_rgba, w, h, alpha_cutoff, weighting, st, wi));
    return palette_of_working(p, wi, k, st, c4, fixed);
}

}  // namespace

int kmg::local_frame_centroids(kmg_processor *p, const uint8_t *d_rgba, uint32_t w, uint32_t h, uint32_t k, uint32_t alpha_cutoff,
                               hipStream_t st, float *c4, const float *fixed4, uint32_t n_fixed, const float *warm4, int weighting)
{
    WorkingImage wi;
    KMG_TRY(working_image(p, d_rgba, w, h, alpha_cutoff, weighting, st, wi));
    if (!warm4) return kmg::palette_of_working(p, wi.src, wi.sw, wi.sh, k, st, c4, nullptr, fixed4, n_fixed, weighting);
    LloydGuard g;
    KMG_TRY(lloyd_create_impl(p, k, &g.s, st));
    KMG_TRY(kmg_lloyd_init_centroids_seeded(g.s, wi.src, wi.sw, wi.sh, warm4, k, st));
    KMG_TRY(kmg_lloyd_set_weighting(g.s, weighting));
    KMG_TRY(kmg_lloyd_run(g.s, wi.src, (uint64_t)wi.sw * wi.sh, nullptr, nullptr, st));
    return kmg_lloyd_get_centroids(g.s, c4, st);
}

namespace {

// the refusals of a palette step while the processor has fixed colours (include/kmeans_hip.h at kmg_processor_set_fixed_colors) or
// alpha weighting (at kmg_processor_set_weighting)
int check_fixed(const FixedList &fixed, uint32_t k, int algo, int weighting)
{
    if (weighting && algo == KMG_ALGO_OCTREE) return fail(KMG_ERR_INVALID_ARGUMENT, "the octree has no alpha weighting (it is on for the processor)");
    const uint32_t f = fixed_count(fixed);
    if (!f) return KMG_OK;
    if (algo == KMG_ALGO_OCTREE) return fail(KMG_ERR_INVALID_ARGUMENT, "the octree has no fixed colours (%u are set on the processor)", f);
    if (k < f) return fail(KMG_ERR_INVALID_ARGUMENT, "k = %u is below the %u fixed colours of the processor", k, f);
    return KMG_OK;
}

// An image between a caller's (pageable) buffer and the device.  The calls that use this return when the work is done, so a large
// image goes through a synchronous copy once `st` has drained: the runtime pipelines it through pinned staging at PCIe
// rate (256 MiB: 4.7 ms each way on the MI355X box between touched buffers), where hipMemcpyAsync of pageable memory takes
// 16-20 ms (tools/host_copy_probe.py, tools/reduce_host_probe.py).  A download into a result buffer whose pages do not exist yet
// still takes 16-40 ms, the caller's page faults; asking for those pages ahead (MADV_POPULATE_WRITE on helper threads during
// the GPU work) was measured and is not in: -6 ms per call in a fresh process, +8 ms in a long-running one.
// Round 4: the copy is ordered on the call's own stream (hipMemcpyWithStream), never on the legacy null stream -- that one
// synchronises with every blocking stream of the host application and serialises the calls this API lets run concurrently on
// one processor (examples/parallel.rs).  An image of 32 MiB or more is cut into kCopyParts row ranges copied by as many host
// threads, each on a stream of its own from the processor's idle list: the staging copies and -- for a result buffer whose
// pages do not exist yet -- the page faults of the ranges then proceed side by side (8192^2 download into fresh pages:
// 26-40 ms as one copy).
constexpr size_t kCopyParts = 4;

}  // namespace

hipError_t kmg::copy_host_image(kmg_processor *p, void *dst, const void *src, size_t bytes, hipMemcpyKind kind, hipStream_t st)
{
    if (bytes < ((size_t)1 << 20)) return hipMemcpyAsync(dst, src, bytes, kind, st);
    hipError_t e = hipStreamSynchronize(st);
    if (e != hipSuccess) return e;
    if (bytes < ((size_t)32 << 20)) return hipMemcpyWithStream(dst, src, bytes, kind, st);
    StreamGuard extra[kCopyParts - 1];
    hipStream_t streams[kCopyParts] = {st};
    for (size_t i = 1; i < kCopyParts; ++i) {
        if ((e = extra[i - 1].acquire(p)) != hipSuccess) return e;
        streams[i] = extra[i - 1].st;
    }
    const size_t part = ((bytes / kCopyParts) + 4095u) & ~(size_t)4095u;
    hipError_t results[kCopyParts];
    std::thread workers[kCopyParts - 1];
    const int device = p->device;
    auto copy_part = [&](size_t i) {
        const size_t off = i * part;
        if (off >= bytes) { results[i] = hipSuccess; return; }
        const size_t nb = std::min(part, bytes - off);
        hipError_t r = i ? hipSetDevice(device) : hipSuccess;          // (a fresh thread has no current device)
        if (r == hipSuccess) r = hipMemcpyWithStream((uint8_t *)dst + off, (const uint8_t *)src + off, nb, kind, streams[i]);
        results[i] = r;
    };
    // (a std::thread that cannot start throws std::system_error: the part is then copied on this thread, and the workers
    // already running are joined whatever happens -- a joinable std::thread that goes out of scope ends the process)
    for (size_t i = 1; i < kCopyParts; ++i) {
        results[i] = hipErrorUnknown;
        try { workers[i - 1] = std::thread(copy_part, i); } catch (const std::exception &) { copy_part(i); }
    }
    copy_part(0);
    for (size_t i = 1; i < kCopyParts; ++i)
        if (workers[i - 1].joinable()) workers[i - 1].join();
    for (size_t i = 0; i < kCopyParts; ++i)
        if (results[i] != hipSuccess) return results[i];
    return hipSuccess;
}

namespace {

int upload_image(kmg_processor *p, const uint8_t *rgba, uint32_t w, uint32_t h, hipStream_t st, StreamBuf &buf)
{
    const size_t bytes = (size_t)w * h * 4;
    HIP_TRY(buf.alloc(p, bytes, st));
    HIP_TRY(copy_host_image(p, buf.ptr, rgba, bytes, hipMemcpyHostToDevice, st));   // structures.rs:31-65
    return KMG_OK;
}

// find_colors / dither_colors + OutputTexture::pull_image (structures.rs:441-470)
// (format: kmg_output_format; out_rgba then holds 4, 1 or 2 bytes per pixel)
int apply_and_download(kmg_processor *p, const uint8_t *d_rgba, uint32_t w, uint32_t h, const float *c4,
                       uint32_t k, int mode, uint32_t alpha_cutoff, hipStream_t st, uint8_t *out_rgba, int format)
{
    StreamBuf out;
    const size_t bytes = (size_t)w * h * format_bytes(format);
    HIP_TRY(out.alloc(p, bytes, st));
    KMG_TRY(dev_apply(p, d_rgba, w, h, 0, c4, k, mode, (uint8_t *)out.ptr, st, alpha_cutoff, format));
    HIP_TRY(copy_host_image(p, out_rgba, out.ptr, bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return KMG_OK;
}

// octree_palette (lib.rs:288-331) on a device-resident image: shrink to <= 128 on the device, pull
// the <= 128x128 image, run the reference's CPU octree on it, sort ascending by palette-crate Lab L.  Alpha mode: the octree gets
// the kept pixels of the shrunk image, in raster order (image: the index by which a batch names an image without one, or -1).
int octree_palette_of(kmg_processor *p, const uint8_t *d_rgba, uint32_t w, uint32_t h, uint32_t color_count, uint32_t alpha_cutoff,
                      hipStream_t st, std::vector<std::array<uint8_t, 4>> &colors, int64_t image = -1)
{
    const uint32_t MAX_SIZE = 128;                                     // lib.rs:293
    uint32_t sw = w, sh = h;
    const uint8_t *src = d_rgba;
    StreamBuf small;
    if (w > MAX_SIZE || h > MAX_SIZE) {
        kmg_resized_dims(w, h, MAX_SIZE, &sw, &sh);
        HIP_TRY(small.alloc(p, (size_t)sw * sh * 4, st));
        KMG_TRY(kmg_dev_resize(p, d_rgba, w, h, sw, sh, (uint8_t *)small.ptr, st));
        src = (const uint8_t *)small.ptr;
    }
    std::vector<uint8_t> host((size_t)sw * sh * 4);
    HIP_TRY(hipMemcpyAsync(host.data(), src, host.size(), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    uint64_t n = (uint64_t)sw * sh;
    if (alpha_cutoff) {
        uint64_t n_kept = 0;
        for (uint64_t i = 0; i < n; ++i)
            if (host[4 * i + 3] >= alpha_cutoff) memmove(&host[4 * n_kept++], &host[4 * i], 4);
        if (n_kept == 0 && image >= 0) return fail(KMG_ERR_INVALID_ARGUMENT, "image %u: no pixel reaches alpha_cutoff = %u", (uint32_t)image, alpha_cutoff);
        if (n_kept == 0) return fail(KMG_ERR_INVALID_ARGUMENT, "no pixel reaches alpha_cutoff = %u", alpha_cutoff);
        n = n_kept;
    }
    colors = octree_sorted_palette(host.data(), n, color_count);
    return KMG_OK;
}

}  // namespace

std::vector<std::array<uint8_t, 4>> kmg::octree_sorted_palette(const uint8_t *host_rgba, uint64_t n_pixels, uint32_t color_count)
{
    std::vector<std::array<uint8_t, 4>> colors = octree_palette(host_rgba, n_pixels, color_count);   // operations.rs:90-97
    std::vector<float> L(colors.size());
    for (size_t i = 0; i < colors.size(); ++i) {
        float lab[3];
        crate_srgb8_to_lab(colors[i].data(), lab);
        L[i] = lab[0];
    }
    std::vector<size_t> order(colors.size());
    for (size_t i = 0; i < order.size(); ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return L[a] < L[b]; });   // lib.rs:320-328
    std::vector<std::array<uint8_t, 4>> sorted(colors.size());
    for (size_t i = 0; i < order.size(); ++i) sorted[i] = colors[order[i]];
    return sorted;
}

// lib.rs:255-286: pull_values (palette-crate Lab -> sRGB8) then sort ascending by Lab L
void kmg::sorted_palette_of(const float *c4, uint32_t color_count, uint8_t *out_rgba)
{
    struct Entry { float L; uint8_t px[4]; };
    std::vector<Entry> e(color_count);
    for (uint32_t i = 0; i < color_count; ++i) {
        uint8_t rgb[3];
        float lab[3];
        crate_lab_to_srgb8(&c4[4 * i], rgb);
        e[i].px[0] = rgb[0]; e[i].px[1] = rgb[1]; e[i].px[2] = rgb[2]; e[i].px[3] = 255;
        crate_srgb8_to_lab(rgb, lab);
        e[i].L = lab[0];
    }
    std::stable_sort(e.begin(), e.end(), [](const Entry &a, const Entry &b) { return a.L < b.L; });
    for (uint32_t i = 0; i < color_count; ++i) memcpy(out_rgba + 4 * i, e[i].px, 4);
}

// ColorTree::{add_color, reduce} (core/src/octree.rs): host helper, needs no device
extern "C" int kmg_octree_palette(const uint8_t *rgba, uint64_t n_pixels, uint32_t color_count, uint8_t *out_rgba,
                                  uint32_t *out_count)
try {
    if (!rgba || !out_rgba || !out_count || n_pixels == 0) return fail(KMG_ERR_INVALID_ARGUMENT, "bad octree arguments");
    const std::vector<std::array<uint8_t, 4>> c = octree_palette(rgba, n_pixels, color_count);
    for (size_t i = 0; i < c.size(); ++i) memcpy(out_rgba + 4 * i, c[i].data(), 4);
    *out_count = (uint32_t)c.size();
    return KMG_OK;
}
KMG_ABI_CATCH

namespace {

// What every host-buffer call on a processor takes at its start.  snapshot(): the processor's settings as they are now -- the
// call keeps them to its end -- taken before any device work, so that the refusals that need no device come first.  begin(): the
// device part -- the call's own stream and the image on the device.
struct CallStart {
    FixedList fixed;
    int weighting = KMG_WEIGHT_NONE;
    uint32_t alpha_cutoff = 0;
    StreamGuard sg;
    StreamBuf img;
    void snapshot(kmg_processor *p)
    {
        fixed = fixed_snapshot(p);
        weighting = p->weighting.load(std::memory_order_relaxed);
        alpha_cutoff = p->alpha_cutoff.load(std::memory_order_relaxed);
    }
    int begin(kmg_processor *p, const uint8_t *rgba, uint32_t w, uint32_t h)
    {
        HIP_TRY(hipSetDevice(p->device));
        HIP_TRY(sg.acquire(p));
        return upload_image(p, rgba, w, h, sg.st, img);
    }
    const uint8_t *d_rgba() const { return (const uint8_t *)img.ptr; }
};

double ms_between(std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b)
{
    return std::chrono::duration<double, std::milli>(b - a).count();
}

// kmg_find / kmg_find_indexed
int find_call(kmg_processor *p, const uint8_t *rgba, uint32_t w, uint32_t h, const uint8_t *palette_rgba, uint32_t n_colors, int mode,
              int format, uint8_t *out)
{
    KMG_TRY(check_image(p, rgba, w, h));
    if (!palette_rgba || n_colors == 0) return fail(KMG_ERR_INVALID_ARGUMENT, "palette is empty");
    if (!out) return fail(KMG_ERR_INVALID_ARGUMENT, "output pointer is NULL");
    KMG_TRY(check_format(format));
    CallStart c;
    c.snapshot(p);
    std::vector<float> c4(4 * (size_t)n_colors);
    KMG_TRY(kmg_palette_to_centroids(palette_rgba, n_colors, c4.data()));   // lib.rs:86-87
    KMG_TRY(c.begin(p, rgba, w, h));
    return apply_and_download(p, c.d_rgba(), w, h, c4.data(), n_colors, mode, c.alpha_cutoff, c.sg.st, out, format);
}

// kmg_reduce (no palette outputs) / kmg_reduce_indexed (palette_out: the palette comes back in index order as the bytes the
// output pass writes -- lab_to_rgb.wgsl of each centroid, kmg_apply.hip's plan palette)
int reduce_call(kmg_processor *p, const uint8_t *rgba, uint32_t w, uint32_t h, uint32_t color_count, int algo, int mode, int format,
                bool palette_out, uint8_t *out_palette_rgba, uint32_t *out_count, uint8_t *out)
{
    KMG_TRY(check_image(p, rgba, w, h));
    KMG_TRY(check_k_nonzero(color_count));
    if (!out || (palette_out && (!out_palette_rgba || !out_count))) return fail(KMG_ERR_INVALID_ARGUMENT, "output pointer is NULL");
    KMG_TRY(check_algo(algo));
    KMG_TRY(check_mode(mode));
    KMG_TRY(check_format(format));
    if (algo == KMG_ALGO_KMEANS) KMG_TRY(check_k_limit(color_count));
    CallStart c;
    c.snapshot(p);
    KMG_TRY(check_fixed(c.fixed, color_count, algo, c.weighting));
    const auto t0 = std::chrono::steady_clock::now();
    KMG_TRY(c.begin(p, rgba, w, h));
    const auto t1 = std::chrono::steady_clock::now();
    std::vector<float> c4;
    if (algo == KMG_ALGO_OCTREE) {                                     // lib.rs:133-136
        std::vector<std::array<uint8_t, 4>> colors;
        KMG_TRY(octree_palette_of(p, c.d_rgba(), w, h, color_count, c.alpha_cutoff, c.sg.st, colors));
        KMG_TRY(octree_centroids(colors, c4));
    } else {
        c4.resize(4 * (size_t)color_count);
        KMG_TRY(extract_palette_kmeans(p, c.d_rgba(), w, h, color_count, c.alpha_cutoff, c.weighting, c.sg.st, c4.data(), c.fixed));
    }
    const auto t2 = std::chrono::steady_clock::now();
    const uint32_t k = (uint32_t)(c4.size() / 4);
    KMG_TRY(apply_and_download(p, c.d_rgba(), w, h, c4.data(), k, mode, c.alpha_cutoff, c.sg.st, out, format));
    if (log_debug())
        fprintf(stderr, "[kmeans_hip] reduce %ux%u k=%u: upload %.2f ms, palette %.2f ms, output pass + download %.2f ms\n", w, h, k,
                ms_between(t0, t1), ms_between(t1, t2), ms_between(t2, std::chrono::steady_clock::now()));
    if (palette_out) {
        for (uint32_t i = 0; i < k; ++i) shader_lab_to_rgba8(&c4[4 * i], out_palette_rgba + 4 * i);
        *out_count = k;
    }
    return KMG_OK;
}

}  // namespace

int kmg::octree_centroids(const std::vector<std::array<uint8_t, 4>> &colors, std::vector<float> &c4)
{
    if (colors.empty()) return fail(KMG_ERR_INVALID_ARGUMENT, "the octree returned no colour");
    if (colors.size() > KMG_MAX_K) return fail(KMG_ERR_UNSUPPORTED, "the octree returned %zu colours, more than KMG_MAX_K = %u", colors.size(), KMG_MAX_K);
    c4.resize(4 * colors.size());
    return kmg_palette_to_centroids(colors[0].data(), (uint32_t)colors.size(), c4.data());
}

extern "C" int kmg_find(kmg_processor *p, const uint8_t *rgba, uint32_t w, uint32_t h, const uint8_t *palette_rgba,
                        uint32_t n_colors, int mode, uint8_t *out_rgba)
try {
    return find_call(p, rgba, w, h, palette_rgba, n_colors, mode, KMG_FORMAT_RGBA8, out_rgba);
}
KMG_ABI_CATCH

extern "C" int kmg_find_indexed(kmg_processor *p, const uint8_t *rgba, uint32_t w, uint32_t h, const uint8_t *palette_rgba,
                                uint32_t n_colors, int mode, int format, void *out_index)
try {
    return find_call(p, rgba, w, h, palette_rgba, n_colors, mode, format, (uint8_t *)out_index);
}
KMG_ABI_CATCH

extern "C" int kmg_reduce_indexed(kmg_processor *p, const uint8_t *rgba, uint32_t w, uint32_t h, uint32_t color_count, int algo,
                                  int mode, int format, uint8_t *out_palette_rgba, uint32_t *out_count, void *out_index)
try {
    return reduce_call(p, rgba, w, h, color_count, algo, mode, format, true, out_palette_rgba, out_count, (uint8_t *)out_index);
}
KMG_ABI_CATCH

extern "C" int kmg_reduce(kmg_processor *p, const uint8_t *rgba, uint32_t w, uint32_t h, uint32_t color_count,
                          int algo, int mode, uint8_t *out_rgba)
try {
    return reduce_call(p, rgba, w, h, color_count, algo, mode, KMG_FORMAT_RGBA8, false, nullptr, nullptr, out_rgba);
}
KMG_ABI_CATCH

extern "C" int kmg_palette(kmg_processor *p, const uint8_t *rgba, uint32_t w, uint32_t h, uint32_t color_count,
                           int algo, uint8_t *out_rgba, uint32_t *out_count)
try {
    KMG_TRY(check_image(p, rgba, w, h));
    KMG_TRY(check_k_nonzero(color_count));
    if (!out_rgba || !out_count) return fail(KMG_ERR_INVALID_ARGUMENT, "output pointer is NULL");
    KMG_TRY(check_algo(algo));
    if (algo == KMG_ALGO_KMEANS) KMG_TRY(check_k_limit(color_count));
    CallStart c;
    c.snapshot(p);
    KMG_TRY(check_fixed(c.fixed, color_count, algo, c.weighting));
    KMG_TRY(c.begin(p, rgba, w, h));
    if (algo == KMG_ALGO_OCTREE) {                                     // lib.rs:288-331
        std::vector<std::array<uint8_t, 4>> colors;
        KMG_TRY(octree_palette_of(p, c.d_rgba(), w, h, color_count, c.alpha_cutoff, c.sg.st, colors));
        for (size_t i = 0; i < colors.size(); ++i) memcpy(out_rgba + 4 * i, colors[i].data(), 4);
        *out_count = (uint32_t)colors.size();
        return KMG_OK;
    }
    std::vector<float> c4(4 * (size_t)color_count);
    KMG_TRY(extract_palette_kmeans(p, c.d_rgba(), w, h, color_count, c.alpha_cutoff, c.weighting, c.sg.st, c4.data(), c.fixed));
    sorted_palette_of(c4.data(), color_count, out_rgba);
    *out_count = color_count;
    return KMG_OK;
}
KMG_ABI_CATCH

// ---------------------------------------------------------------------------------------------
// batches (include/kmeans_hip.h at kmg_batch_report; the kernels and kmg_dev_palette_batch: kmg_batch.hip)
// ---------------------------------------------------------------------------------------------
namespace {

// The smallest sub-batch that goes through the batched kernels; a smaller one -- a single image -- runs the per-image palette step
// inside the call (the same results).  The batched initialisation is the single pick, k launches, where the per-image route picks
// several centroids per launch from k = 32 on (~ 0.3 k + 18 launches): one image alone would pay for that, two images already
// do not -- the `kernels` rows of profiles/r09_batch_time.txt (tools/batch_probe.py) at N = 1, i.e. two images: 0.89, 0.61 and
// 0.77 of the per-image calls at k = 8, 64 and 256.
constexpr uint32_t kBatchMinImages = 2;

// kmg_palette_batch, kmg_reduce_batch, kmg_reduce_indexed_batch, kmg_reduce_quality_batch
enum class BatchKind { kPalette, kReduce, kReduceIndexed, kQuality };

// kmg_reduce_quality from its working image on (defined with it, below): the search, the output, the results.  runs: ADDS the palette runs.
int quality_of_working(kmg_processor *p, const uint8_t *d_rgba, uint32_t w, uint32_t h, const WorkingImage &wi, uint32_t k_min, uint32_t k_max,
                       uint32_t target, int mode, int format, uint32_t alpha_cutoff, const FixedList &fixed, hipStream_t st,
                       uint8_t *out_palette_rgba, uint32_t *out_count, void *out, kmg_error_stats *achieved, int *reached, uint32_t *runs);

// One image of a sub-batch on the device: its source and its working image (the octree has the source only)
struct BatchStage { StreamBuf src; WorkingImage wi; };

// What image (w, h) keeps on the device while its sub-batch runs (include/kmeans_hip.h at max_resident_bytes): the source -- a palette
// call releases one that was shrunk --, the shrunk and the compacted copy, an indexed or quality call's output, a quality call's
// labels of the working image (2 bytes each).  The octree holds the source only.
uint64_t batch_resident_bytes(const kmg_processor *p, uint32_t w, uint32_t h, uint32_t alpha_cutoff, BatchKind kind, int algo, int format)
{
    const bool quality = kind == BatchKind::kQuality;
    const uint64_t n = (uint64_t)w * h, out = kind == BatchKind::kReduceIndexed || quality ? format_bytes(format) * n : 0ull;
    if (algo == KMG_ALGO_OCTREE) return 4 * n + out;
    uint32_t sw = w, sh = h;
    const uint32_t m = p->opt.shrink_max_dim;
    const bool shrunk = m && (w > m || h > m);
    if (shrunk) kmg_resized_dims(w, h, m, &sw, &sh);
    return (quality ? 2ull * sw * sh : 0ull) + (shrunk ? 4ull * sw * sh : 0ull) + (kind != BatchKind::kPalette || !shrunk ? 4 * n : 0ull) + (alpha_cutoff ? 4ull * sw * sh : 0ull) + out;
}

// One call of kmg_palette_batch / kmg_reduce_batch / kmg_reduce_indexed_batch by steps: run() is the refusals, the cuts, alpha
// mode's up-front pass, then per sub-batch a palette step (by algorithm) and an output step (by kind), and one drain at the end.
// First the arguments.  format: KMG_FORMAT_RGBA8 unless kReduceIndexed; out: per image the palette (kPalette) or the output;
// palettes: kReduceIndexed's and kQuality's palettes in index order, else NULL; out_counts: NULL for kReduce.  kQuality:
// color_count is k_max, and the call has k_min, target, achieved and reached (the last two may be NULL).
struct BatchCall {
    BatchKind kind; kmg_processor *p; uint32_t n_images;
    const uint8_t *const *rgba; const uint32_t *widths, *heights;
    uint32_t color_count; int algo, mode, format; uint64_t max_resident_bytes;
    uint8_t *const *out, *const *palettes; uint32_t *out_counts;
    uint32_t k_min = 0, target = 0; kmg_error_stats *achieved = nullptr; int *reached = nullptr;
    kmg_batch_quality_report qrep = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    CallStart c;
    hipStream_t st = nullptr;
    std::vector<uint32_t> cuts;      // sub-batch s: images [cuts[s], cuts[s + 1])
    std::vector<std::vector<std::array<uint8_t, 4>>> colors;   // the octree's palette of every image
    // what the palette step of a sub-batch leaves: the centroid table of its image q has ks[q] colours and starts at c4[at[q]]
    std::vector<float> c4; std::vector<uint32_t> ks; std::vector<size_t> at;
    kmg_batch_report rep = {0u, 0u, 0u, 0u}; kmg_batch_apply_report arep = {0u, 0u, 0u, 0u};
    bool octree() const { return algo == KMG_ALGO_OCTREE; }
    bool up_front() const { return c.alpha_cutoff && cuts.size() > 2; }   // alpha mode, several sub-batches: alpha_up_front runs
    const float *table(uint32_t q) const { return &c4[at[q]]; }

    // the refusals, for the whole batch, before any device work (the order is part of the contract: include/kmeans_hip.h)
    int refusals()
    {
        const bool quality = kind == BatchKind::kQuality, indexed = kind == BatchKind::kReduceIndexed;
        const bool array_null = !rgba || !widths || !heights || !out || (kind != BatchKind::kReduce && !out_counts) || ((indexed || quality) && !palettes);
        KMG_TRY(check_batch_prefix(p, n_images, array_null, "a batch array is NULL", rgba, widths, heights, out, palettes));
        if (quality) {                                                 // the list of kmg_reduce_quality, then the batches' two
            if (k_min < 1 || k_min > color_count || color_count > KMG_MAX_K)
                return fail(KMG_ERR_INVALID_ARGUMENT, "colour counts [%u, %u]: 1 <= k_min <= k_max <= %u", k_min, color_count, KMG_MAX_K);
            KMG_TRY(check_mode(mode));
            KMG_TRY(check_format(format));
            KMG_TRY(check_meld_format(mode, format));
            c.snapshot(p);
            KMG_TRY(check_index8_room(format == KMG_FORMAT_INDEX8, "k_max", color_count, c.alpha_cutoff != 0));
            if (const uint32_t f = fixed_count(c.fixed)) return fail(KMG_ERR_INVALID_ARGUMENT, "a batch has no fixed colours (%u are set on the processor)", f);
            if (c.weighting) return fail(KMG_ERR_INVALID_ARGUMENT, "a batch has no alpha weighting (it is on for the processor)");
            return KMG_OK;
        }
        KMG_TRY(check_k_nonzero(color_count));
        KMG_TRY(check_algo(algo));
        if (kind != BatchKind::kPalette) KMG_TRY(check_mode(mode));
        if (indexed) KMG_TRY(check_format(format));
        if (!octree()) KMG_TRY(check_k_limit(color_count));
        c.snapshot(p);
        if (format != KMG_FORMAT_RGBA8) {                              // (the centroids' box: once a sub-batch has its palettes)
            KMG_TRY(check_meld_format(mode, format));
            KMG_TRY(check_index8_room(format == KMG_FORMAT_INDEX8, "k", color_count, c.alpha_cutoff != 0));
        }
        if (const uint32_t f = fixed_count(c.fixed)) return fail(KMG_ERR_INVALID_ARGUMENT, "a batch has no fixed colours (%u are set on the processor)", f);
        if (c.weighting) return fail(KMG_ERR_INVALID_ARGUMENT, "a batch has no alpha weighting (it is on for the processor)");
        return KMG_OK;
    }
    // the cuts: batch_cuts over batch_resident_bytes
    void plan()
    {
        std::vector<uint64_t> bytes(n_images);
        for (uint32_t i = 0; i < n_images; ++i) bytes[i] = batch_resident_bytes(p, widths[i], heights[i], c.alpha_cutoff, kind, algo, format);
        cuts = batch_cuts(bytes.data(), n_images, max_resident_bytes);
        rep.sub_batches = arep.sub_batches = qrep.sub_batches = (uint32_t)cuts.size() - 1u;
        colors.resize(octree() ? n_images : 0);
    }
    // Uploads images [a, e) and makes their working images: working_enqueue for each, one read-back and one synchronisation for the
    // kept-pixel counts of all of them, working_resolve.  keep_source = false: a source that was shrunk is released at once.
    int stage_images(uint32_t a, uint32_t e, bool keep_source, BatchStage *stage)
    {
        const uint32_t cutoff = c.alpha_cutoff;
        StreamBuf counts;
        if (cutoff) HIP_TRY(counts.alloc(p, sizeof(uint64_t) * (e - a), st));
        for (uint32_t i = a; i < e; ++i) {
            BatchStage &s = stage[i - a];
            KMG_TRY(upload_image(p, rgba[i], widths[i], heights[i], st, s.src));
            KMG_TRY(working_enqueue(p, (const uint8_t *)s.src.ptr, widths[i], heights[i], cutoff, KMG_WEIGHT_NONE, st, s.wi,
                                    cutoff ? (uint64_t *)counts.ptr + (i - a) : nullptr, keep_source ? nullptr : &s.src));
        }
        if (!cutoff) return KMG_OK;
        std::vector<uint64_t> n_kept(e - a);
        HIP_TRY(hipMemcpyAsync(n_kept.data(), counts.ptr, sizeof(uint64_t) * (e - a), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        for (uint32_t i = a; i < e; ++i)
            if (!working_resolve(stage[i - a].wi, n_kept[i - a]))
                return fail(KMG_ERR_INVALID_ARGUMENT, "image %u: no pixel reaches alpha_cutoff = %u", i, cutoff);
        return KMG_OK;
    }
    // An image that keeps no pixel has to refuse the call before the first sub-batch writes its outputs -- everything is uploaded and
    // shrunk once up front for that alone.  The octree's palettes are kept, so it still runs once per image; the k-means route keeps
    // nothing and stages every image a second time in its sub-batch.
    int alpha_up_front()
    {
        for (size_t s = 0; s + 1 < cuts.size(); ++s) {
            const uint32_t a = cuts[s], e = cuts[s + 1];
            std::unique_ptr<BatchStage[]> stage(new BatchStage[octree() ? 0 : e - a]);
            if (!octree()) KMG_TRY(stage_images(a, e, false, stage.get()));
            for (uint32_t i = a; octree() && i < e; ++i) {
                StreamBuf src;
                KMG_TRY(upload_image(p, rgba[i], widths[i], heights[i], st, src));
                KMG_TRY(octree_palette_of(p, (const uint8_t *)src.ptr, widths[i], heights[i], color_count, c.alpha_cutoff, st, colors[i], i));
            }
        }
        return KMG_OK;
    }
    // The palette step of sub-batch [a, e), octree: per image the source on the device, the host algorithm (unless it ran up front)
    // and the centroid table.  (A palette call returns the octree's own bytes: no tables, none of octree_centroids' refusals.)
    int palettes_octree(uint32_t a, uint32_t e, BatchStage *stage)
    {
        std::vector<float> mine;
        for (uint32_t i = a; i < e; ++i) {
            StreamBuf &src = stage[i - a].src;
            KMG_TRY(upload_image(p, rgba[i], widths[i], heights[i], st, src));
            if (!up_front())
                KMG_TRY(octree_palette_of(p, (const uint8_t *)src.ptr, widths[i], heights[i], color_count, c.alpha_cutoff, st, colors[i], i));
            if (kind != BatchKind::kPalette) {
                KMG_TRY(octree_centroids(colors[i], mine));
                at.push_back(c4.size()); ks.push_back((uint32_t)(mine.size() / 4));
                c4.insert(c4.end(), mine.begin(), mine.end());
            }
        }
        return KMG_OK;
    }
    // The palette step of sub-batch [a, e), k-means: the working images, then the batched kernels -- or, below kBatchMinImages, the
    // per-image palette step, image after image.  Every table has color_count colours.
    int palettes_kmeans(uint32_t a, uint32_t e, BatchStage *stage)
    {
        const uint32_t count = e - a, k = color_count;
        KMG_TRY(stage_images(a, e, kind != BatchKind::kPalette, stage));
        c4.resize(4ull * k * count); ks.assign(count, k);
        std::vector<const uint8_t *> work(count); std::vector<uint32_t> sw(count), sh(count);
        for (uint32_t q = 0; q < count; ++q) {
            at.push_back(4ull * k * q);
            work[q] = stage[q].wi.src; sw[q] = stage[q].wi.sw; sh[q] = stage[q].wi.sh;
        }
        if (count < kBatchMinImages) {
            for (uint32_t q = 0; q < count; ++q) {                   // (no batched launch; the report's iterations cover the image all the same)
                uint32_t it = 0;
                KMG_TRY(kmg::palette_of_working(p, work[q], sw[q], sh[q], k, st, &c4[at[q]], nullptr, nullptr, 0, KMG_WEIGHT_NONE, &it));
                rep.iterations = std::max(rep.iterations, it);
            }
            return KMG_OK;
        }
        kmg_batch_report r;
        KMG_TRY_DRAIN(st, dev_palette_batch(p, count, work.data(), sw.data(), sh.data(), k, c4.data(), nullptr, &r, st));
        rep.launches += r.launches; rep.fallback += r.fallback;
        rep.iterations = std::max(rep.iterations, r.iterations);
        return KMG_OK;
    }
    // the output step of kmg_palette_batch: the octree's colours as they are, the k-means centroids as the sorted palette (lib.rs:255-286)
    void output_palette(uint32_t a, uint32_t e)
    {
        for (uint32_t i = a; i < e; ++i) {
            if (!octree()) sorted_palette_of(table(i - a), color_count, out[i]);
            for (size_t q = 0; octree() && q < colors[i].size(); ++q) memcpy(out[i] + 4 * q, colors[i][q].data(), 4);
            out_counts[i] = octree() ? (uint32_t)colors[i].size() : color_count;
        }
    }
    // kmg_reduce_indexed_batch: the palette of image a + q in index order, as the bytes the output pass writes (reduce_call)
    void palette_out(uint32_t a, uint32_t q)
    {
        for (uint32_t j = 0; j < ks[q]; ++j) shader_lab_to_rgba8(table(q) + 4 * j, palettes[a + q] + 4 * j);
        out_counts[a + q] = ks[q];
    }
    // the output step of kmg_reduce_batch, and of kmg_reduce_indexed_batch after the octree (palette sizes differ): the per-image output pass
    int output_each(uint32_t a, uint32_t e, const BatchStage *stage)
    {
        for (uint32_t q = 0; q < e - a; ++q) {
            KMG_TRY(apply_and_download(p, (const uint8_t *)stage[q].src.ptr, widths[a + q], heights[a + q], table(q), ks[q], mode, c.alpha_cutoff, st,
                                       out[a + q], format));
            if (kind == BatchKind::kReduceIndexed) palette_out(a, q);
        }
        if (kind == BatchKind::kReduceIndexed) arep.per_image += e - a;
        return KMG_OK;
    }
    // the output step of kmg_reduce_indexed_batch after k-means: one launch for the images that join it, one download each (kmg_batch_apply.hip)
    int output_joined(uint32_t a, uint32_t e, const BatchStage *stage)
    {
        const uint32_t count = e - a, k = color_count;
        std::vector<const uint8_t *> src(count);
        for (uint32_t q = 0; q < count; ++q) src[q] = (const uint8_t *)stage[q].src.ptr;
        if (format != KMG_FORMAT_RGBA8)
            for (uint32_t q = 0; q < count; ++q) KMG_TRY(check_index_format(table(q), k, mode, format, c.alpha_cutoff));
        KMG_TRY(apply_batch_download(p, count, src.data(), widths + a, heights + a, c4.data(), count, k, mode, format, c.alpha_cutoff, out + a, &arep,
                                     st));
        for (uint32_t q = 0; q < count; ++q) palette_out(a, q);
        return KMG_OK;
    }
    // kmg_reduce_quality's own search for image a + q of a sub-batch, from its staged working image on
    int quality_each(uint32_t a, uint32_t q, const BatchStage *stage)
    {
        const uint32_t i = a + q;
        ++qrep.per_image;
        return quality_of_working(p, (const uint8_t *)stage[q].src.ptr, widths[i], heights[i], stage[q].wi, k_min, color_count, target, mode, format,
                                  c.alpha_cutoff, c.fixed, st, palettes[i], &out_counts[i], out[i], achieved ? &achieved[i] : nullptr,
                                  reached ? &reached[i] : nullptr, &qrep.palette_runs);
    }
    // Sub-batch [a, e) of kmg_reduce_quality_batch: the working images; the per-image search for a working image of kBatchMaxWorking
    // pixels or more and for fewer than kBatchMinImages smaller ones; for the others the search in lock step (kmg_quality_search.h)
    // -- per round one palette chain, one label pass, one record, each with the images' own counts -- and the output at every k*.
    int quality_batch(uint32_t a, uint32_t e, BatchStage *stage)
    {
        constexpr uint64_t kBatchMaxWorking = 1ull << 19;              // (what kmg_dev_palette_batch takes through the batched kernels)
        KMG_TRY(stage_images(a, e, true, stage));
        std::vector<uint32_t> small;
        for (uint32_t q = 0; q < e - a; ++q) {
            if ((uint64_t)stage[q].wi.sw * stage[q].wi.sh < kBatchMaxWorking) { small.push_back(q); continue; }
            ++qrep.fallback;
            KMG_TRY(quality_each(a, q, stage));
        }
        if (small.size() < kBatchMinImages) {
            for (const uint32_t q : small) KMG_TRY(quality_each(a, q, stage));
            return KMG_OK;
        }
        const uint32_t m = (uint32_t)small.size();
        // W and its labels (one block, kmg_batch_layout.h), the records
        std::vector<const uint8_t *> work(m); std::vector<uint32_t> sw(m), sh(m); std::vector<uint64_t> nw(m), offset;
        for (uint32_t j = 0; j < m; ++j) {
            const WorkingImage &wi = stage[small[j]].wi;
            work[j] = wi.src; sw[j] = wi.sw; sh[j] = wi.sh; nw[j] = (uint64_t)wi.sw * wi.sh;
        }
        uint64_t total = 0;
        if (!batch_offsets(nw.data(), m, 2u, offset, &total, (uint64_t)SIZE_MAX / 2))
            return fail(KMG_ERR_OUT_OF_MEMORY, "the labels of the sub-batch do not fit one block");
        StreamBuf labels, records;
        HIP_TRY(labels.alloc(p, (size_t)total, st));
        HIP_TRY(records.alloc(p, sizeof(kmg_error_stats) * m, st));
        std::vector<QualitySearch> search(m, QualitySearch(k_min, color_count));
        std::vector<std::vector<float>> best_c4(m);
        std::vector<kmg_error_stats> best(m), cur(m);
        // the rounds: the images that still search, each at its own count
        std::vector<uint32_t> act, ks_r, sw_r, sh_r; std::vector<const uint8_t *> work_r; std::vector<void *> lab_r; std::vector<uint64_t> nw_r;
        std::vector<size_t> at_r; std::vector<float> c4_r; std::vector<uint8_t> pal_r;
        for (uint32_t round = 0;; ++round) {
            act.clear(); ks_r.clear(); sw_r.clear(); sh_r.clear(); work_r.clear(); lab_r.clear(); nw_r.clear(); at_r.clear();
            size_t k_sum = 0;
            for (uint32_t j = 0; j < m; ++j) {
                if (search[j].done()) continue;
                act.push_back(j); ks_r.push_back(search[j].next()); sw_r.push_back(sw[j]); sh_r.push_back(sh[j]); work_r.push_back(work[j]);
                lab_r.push_back((uint8_t *)labels.ptr + offset[j]); nw_r.push_back(nw[j]); at_r.push_back(4 * k_sum);
                k_sum += ks_r.back();
            }
            if (act.empty()) break;
            qrep.rounds = std::max(qrep.rounds, round + 1u);
            const uint32_t r = (uint32_t)act.size();
            c4_r.resize(4 * k_sum); pal_r.resize(4 * k_sum);
            kmg_batch_report prep;
            KMG_TRY_DRAIN(st, dev_palette_batch_counts(p, r, work_r.data(), sw_r.data(), sh_r.data(), ks_r.data(), c4_r.data(), nullptr, &prep, st));
            qrep.launches += prep.launches; qrep.palette_runs += r;
            kmg_batch_apply_report lrep = {0u, 0u, 0u, 0u};
            KMG_TRY_DRAIN(st, apply_batch_counts(p, r, work_r.data(), sw_r.data(), sh_r.data(), c4_r.data(), at_r.data(), ks_r.data(), false,
                                                 KMG_MODE_REPLACE, KMG_FORMAT_INDEX16, 0u, lab_r.data(), &lrep, st));
            for (size_t t = 0; t < k_sum; ++t) shader_lab_to_rgba8(&c4_r[4 * t], &pal_r[4 * t]);
            HIP_TRY_DRAIN(st, hipMemsetAsync(records.ptr, 0, sizeof(kmg_error_stats) * r, st));
            KMG_TRY_DRAIN(st, dev_compare_batch(p, r, work_r.data(), lab_r.data(), nw_r.data(), KMG_FORMAT_INDEX16, pal_r.data(), ks_r.data(), 0u,
                                                KMG_ERROR_RGB | KMG_ERROR_LAB, (kmg_error_stats *)records.ptr, st, &qrep.measure_launches));
            HIP_TRY_DRAIN(st, hipMemcpyAsync(cur.data(), records.ptr, sizeof(kmg_error_stats) * r, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            for (uint32_t t = 0; t < r; ++t) {
                const uint32_t j = act[t];
                const bool accepted = cur[t].lab_sse <= (uint64_t)target * nw[j];
                if (log_debug())
                    fprintf(stderr, "[kmeans_hip] reduce_quality_batch: image %u, k = %u, E = %llu, limit %llu: %s\n", a + small[j], ks_r[t],
                            (unsigned long long)cur[t].lab_sse, (unsigned long long)((uint64_t)target * nw[j]), accepted ? "accepted" : "not accepted");
                if (search[j].take(accepted)) {
                    best[j] = cur[t];
                    best_c4[j].assign(c4_r.begin() + at_r[t], c4_r.begin() + at_r[t] + 4 * (size_t)ks_r[t]);
                }
            }
        }
        // the output: every image at its own k*, on the full-size sources
        std::vector<const uint8_t *> src(m); std::vector<uint32_t> w_o(m), h_o(m), ks_o(m); std::vector<size_t> at_o(m); std::vector<uint8_t *> out_o(m);
        std::vector<float> c4_o;
        for (uint32_t j = 0; j < m; ++j) {
            const uint32_t i = a + small[j];
            src[j] = (const uint8_t *)stage[small[j]].src.ptr; w_o[j] = widths[i]; h_o[j] = heights[i]; out_o[j] = out[i];
            ks_o[j] = search[j].k_star(); at_o[j] = c4_o.size();
            c4_o.insert(c4_o.end(), best_c4[j].begin(), best_c4[j].end());
        }
        if (format != KMG_FORMAT_RGBA8)
            for (uint32_t j = 0; j < m; ++j) KMG_TRY(check_index_format(&c4_o[at_o[j]], ks_o[j], mode, format, c.alpha_cutoff));
        kmg_batch_apply_report orep = {0u, 0u, 0u, 0u};
        KMG_TRY(apply_batch_counts_download(p, m, src.data(), w_o.data(), h_o.data(), c4_o.data(), at_o.data(), ks_o.data(), mode, format, c.alpha_cutoff,
                                            out_o.data(), &orep, st));
        qrep.batched += orep.batched; qrep.per_image += orep.per_image;
        for (uint32_t j = 0; j < m; ++j) {
            const uint32_t i = a + small[j];
            for (uint32_t t = 0; t < ks_o[j]; ++t) shader_lab_to_rgba8(&c4_o[at_o[j] + 4 * t], palettes[i] + 4 * t);
            out_counts[i] = ks_o[j];
            if (achieved) achieved[i] = best[j];
            if (reached) reached[i] = search[j].reached ? 1 : 0;
        }
        return KMG_OK;
    }
    int run(kmg_batch_report *report, kmg_batch_apply_report *apply_report = nullptr)
    {
        KMG_TRY(refusals());
        HIP_TRY(hipSetDevice(p->device));
        HIP_TRY(c.sg.acquire(p));
        st = c.sg.st;
        plan();
        if (up_front()) KMG_TRY(alpha_up_front());
        for (size_t s = 0; s + 1 < cuts.size(); ++s) {
            const uint32_t a = cuts[s], e = cuts[s + 1];
            std::unique_ptr<BatchStage[]> stage(new BatchStage[e - a]);
            c4.clear(); ks.clear(); at.clear();
            if (kind == BatchKind::kQuality) { KMG_TRY(quality_batch(a, e, stage.get())); continue; }
            KMG_TRY(octree() ? palettes_octree(a, e, stage.get()) : palettes_kmeans(a, e, stage.get()));
            if (kind == BatchKind::kPalette) output_palette(a, e);
            else if (kind == BatchKind::kReduce || octree()) KMG_TRY(output_each(a, e, stage.get()));
            else KMG_TRY(output_joined(a, e, stage.get()));
        }
        HIP_TRY(hipStreamSynchronize(st));
        if (report) *report = rep;
        if (apply_report) *apply_report = arep;
        return KMG_OK;
    }
};

}  // namespace

extern "C" int kmg_palette_batch(kmg_processor *p, uint32_t n_images, const uint8_t *const *rgba, const uint32_t *widths,
                                 const uint32_t *heights, uint32_t color_count, int algo, uint64_t max_resident_bytes,
                                 uint8_t *const *out_rgba, uint32_t *out_counts, kmg_batch_report *report)
try {
    return BatchCall{BatchKind::kPalette, p, n_images, rgba, widths, heights, color_count, algo, KMG_MODE_REPLACE, KMG_FORMAT_RGBA8,
                     max_resident_bytes, out_rgba, nullptr, out_counts}.run(report);
}
KMG_ABI_CATCH

extern "C" int kmg_reduce_batch(kmg_processor *p, uint32_t n_images, const uint8_t *const *rgba, const uint32_t *widths,
                                const uint32_t *heights, uint32_t color_count, int algo, int mode, uint64_t max_resident_bytes,
                                uint8_t *const *out_rgba, kmg_batch_report *report)
try {
    return BatchCall{BatchKind::kReduce, p, n_images, rgba, widths, heights, color_count, algo, mode, KMG_FORMAT_RGBA8,
                     max_resident_bytes, out_rgba, nullptr, nullptr}.run(report);
}
KMG_ABI_CATCH

extern "C" int kmg_reduce_indexed_batch(kmg_processor *p, uint32_t n_images, const uint8_t *const *rgba, const uint32_t *widths,
                                        const uint32_t *heights, uint32_t color_count, int algo, int mode, int format,
                                        uint64_t max_resident_bytes, uint8_t *const *out_palette_rgba, uint32_t *out_counts,
                                        void *const *out_index, kmg_batch_report *batch_report, kmg_batch_apply_report *apply_report)
try {
    return BatchCall{BatchKind::kReduceIndexed, p, n_images, rgba, widths, heights, color_count, algo, mode, format,
                     max_resident_bytes, (uint8_t *const *)out_index, out_palette_rgba, out_counts}.run(batch_report, apply_report);
}
KMG_ABI_CATCH

namespace {

// kmg_find_batch: kmg_find_indexed of every image with one palette; the sources of a sub-batch in one stream-ordered block
// (kmg_batch_layout.h), its output step in one launch (apply_batch_download)
int find_batch_call(kmg_processor *p, uint32_t n_images, const uint8_t *const *rgba, const uint32_t *widths, const uint32_t *heights,
                    const uint8_t *palette_rgba, uint32_t n_colors, int mode, int format, uint64_t max_resident_bytes, uint8_t *const *out,
                    kmg_batch_apply_report *report)
{
    // the refusals, for the whole batch, before any device work (the order is part of the contract: include/kmeans_hip.h)
    KMG_TRY(check_batch_prefix(p, n_images, !rgba || !widths || !heights || !out, "a batch array is NULL", rgba, widths, heights, out));
    if (!palette_rgba || n_colors == 0) return fail(KMG_ERR_INVALID_ARGUMENT, "palette is empty");
    KMG_TRY(check_mode(mode));
    KMG_TRY(check_format(format));
    KMG_TRY(check_k_limit(n_colors));
    CallStart c;
    c.snapshot(p);
    const uint32_t cutoff = c.alpha_cutoff, bpp = format_bytes(format);
    std::vector<float> c4(4 * (size_t)n_colors);
    KMG_TRY(kmg_palette_to_centroids(palette_rgba, n_colors, c4.data()));   // lib.rs:86-87
    if (format != KMG_FORMAT_RGBA8) KMG_TRY(check_index_format(c4.data(), n_colors, mode, format, cutoff));
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(c.sg.acquire(p));
    hipStream_t st = c.sg.st;

    // consecutive sub-batches whose resident bytes (source and output) fit the bound: images [a, a + count)
    kmg_batch_apply_report rep = {0u, 0u, 0u, 0u};
    std::vector<uint64_t> pixels(n_images), bytes(n_images), offset;
    for (uint32_t i = 0; i < n_images; ++i) { pixels[i] = (uint64_t)widths[i] * heights[i]; bytes[i] = (4ull + bpp) * pixels[i]; }
    const std::vector<uint32_t> cuts = batch_cuts(bytes.data(), n_images, max_resident_bytes);
    for (size_t s = 0; s + 1 < cuts.size(); ++s) {
        const uint32_t a = cuts[s], count = cuts[s + 1] - a;
        uint64_t total = 0;
        if (!batch_offsets(&pixels[a], count, 4u, offset, &total, (uint64_t)SIZE_MAX / 2))
            return fail(KMG_ERR_OUT_OF_MEMORY, "the sources of the sub-batch do not fit one block");
        StreamBuf block;
        HIP_TRY(block.alloc(p, (size_t)total, st));
        std::vector<const uint8_t *> src(count);
        for (uint32_t q = 0; q < count; ++q) {
            src[q] = (const uint8_t *)block.ptr + offset[q];
            HIP_TRY_DRAIN(st, copy_host_image(p, (void *)src[q], rgba[a + q], (size_t)pixels[a + q] * 4, hipMemcpyHostToDevice, st));   // structures.rs:31-65
        }
        KMG_TRY_DRAIN(st, apply_batch_download(p, count, src.data(), widths + a, heights + a, c4.data(), 1u, n_colors, mode, format, cutoff,
                                               out + a, &rep, st));
        ++rep.sub_batches;
    }
    if (report) *report = rep;
    return KMG_OK;
}

}  // namespace

extern "C" int kmg_find_batch(kmg_processor *p, uint32_t n_images, const uint8_t *const *rgba, const uint32_t *widths,
                              const uint32_t *heights, const uint8_t *palette_rgba, uint32_t n_colors, int mode, int format,
                              uint64_t max_resident_bytes, void *const *out, kmg_batch_apply_report *report)
try {
    return find_batch_call(p, n_images, rgba, widths, heights, palette_rgba, n_colors, mode, format, max_resident_bytes, (uint8_t *const *)out,
                           report);
}
KMG_ABI_CATCH

// ---------------------------------------------------------------------------------------------
// error statistics and the quality-targeted colour count (include/kmeans_hip.h at kmg_error_stats; kernels: kmg_error.hip)
// ---------------------------------------------------------------------------------------------
namespace {

// kmg_dev_compare with the output's form given (kmg_kernels.h kErrorRgba8 .. kErrorLabel32).  Enqueues on st: for the index forms
// the palette's upload from a heap copy of the caller's bytes (released by the stream once the copy has run), the launch that
// makes its q triples, and the statistics launch; the device scratch goes back to the pool in stream order.
int dev_compare_form(kmg_processor *p, const uint8_t *d_src, const void *d_out, uint64_t n, int form, const uint8_t *palette_rgba,
                     uint32_t k, uint32_t alpha_cutoff, uint32_t what, kmg_error_stats *d_stats, hipStream_t st)
{
    static_assert(sizeof(kmg_error_stats) == 14 * sizeof(uint64_t), "kmg_error_stats is 14 x uint64_t");
    // (the refusals that need no device come first)
    if (what == 0 || (what & ~(KMG_ERROR_RGB | KMG_ERROR_LAB))) return fail(KMG_ERR_INVALID_ARGUMENT, "what = %u: KMG_ERROR_RGB | KMG_ERROR_LAB", what);
    if (alpha_cutoff > 255u) return fail(KMG_ERR_INVALID_ARGUMENT, "alpha cutoff %u is above 255", alpha_cutoff);
    if (form != kErrorRgba8) {
        if (!palette_rgba || k == 0 || k > KMG_MAX_K) return fail(KMG_ERR_INVALID_ARGUMENT, "an index format needs a palette of 1 .. %u colours", KMG_MAX_K);
        KMG_TRY(check_index8_room(form == kErrorIndex8, "k", k, alpha_cutoff != 0));
        if (form == kErrorIndex16 && (reinterpret_cast<uintptr_t>(d_out) & 1u)) return fail(KMG_ERR_INVALID_ARGUMENT, "INDEX16 output is not 2-byte aligned");
    }
    if (!p || !d_src || !d_out || !d_stats || n == 0) return fail(KMG_ERR_INVALID_ARGUMENT, "bad compare arguments");
    if (n > 0xFFFFFFFFull) return fail(KMG_ERR_UNSUPPORTED, "more than 2^32-1 pixels");
    if (reinterpret_cast<uintptr_t>(d_stats) & 7u) return fail(KMG_ERR_INVALID_ARGUMENT, "the statistics record is not 8-byte aligned");
    HIP_TRY(hipSetDevice(p->device));
    unsigned long long *stats = reinterpret_cast<unsigned long long *>(d_stats);
    if (form == kErrorRgba8) {
        HIP_TRY(launch_error_stats(form, what, (const uint32_t *)d_src, d_out, n, nullptr, nullptr, 0, alpha_cutoff, p->d_lut, stats, st));
        return KMG_OK;
    }
    StreamBuf tab;                                                     // k (word, qL, qa, qb) entries, then the k palette words
    const size_t ent_bytes = pad256(error_palette_bytes(k));
    HIP_TRY(tab.alloc(p, ent_bytes + (size_t)k * 4, st));
    uint32_t *d_pal = (uint32_t *)((uint8_t *)tab.ptr + ent_bytes);
    HIP_TRY(upload_host_copy(d_pal, palette_rgba, (size_t)k * 4, st));
    if (what & KMG_ERROR_LAB) HIP_TRY(launch_error_palette(d_pal, k, p->d_lut, tab.ptr, st));
    HIP_TRY(launch_error_stats(form, what, (const uint32_t *)d_src, d_out, n, d_pal, tab.ptr, k, alpha_cutoff, p->d_lut, stats, st));
    return KMG_OK;
}

int format_form(int format)
{
    return format == KMG_FORMAT_RGBA8 ? kErrorRgba8 : format == KMG_FORMAT_INDEX8 ? kErrorIndex8 : format == KMG_FORMAT_INDEX16 ? kErrorIndex16 : -1;
}

}  // namespace

extern "C" int kmg_dev_compare(kmg_processor *p, const uint8_t *d_src_rgba, const void *d_out, uint64_t n_pixels, int format,
                               const uint8_t *palette_rgba, uint32_t k, uint32_t alpha_cutoff, uint32_t what, kmg_error_stats *d_stats,
                               void *stream)
try {
    KMG_TRY(check_format(format));
    return dev_compare_form(p, d_src_rgba, d_out, n_pixels, format_form(format), palette_rgba, k, alpha_cutoff, what, d_stats, S(stream));
}
KMG_ABI_CATCH

extern "C" int kmg_compare(kmg_processor *p, const uint8_t *src_rgba, const void *out, uint32_t w, uint32_t h, int format,
                           const uint8_t *palette_rgba, uint32_t k, uint32_t what, kmg_error_stats *stats)
try {
    // (the refusals that need no device come first)
    KMG_TRY(check_format(format));
    const int form = format_form(format);
    if (what == 0 || (what & ~(KMG_ERROR_RGB | KMG_ERROR_LAB))) return fail(KMG_ERR_INVALID_ARGUMENT, "what = %u: KMG_ERROR_RGB | KMG_ERROR_LAB", what);
    if (form != kErrorRgba8 && (!palette_rgba || k == 0 || k > KMG_MAX_K))
        return fail(KMG_ERR_INVALID_ARGUMENT, "an index format needs a palette of 1 .. %u colours", KMG_MAX_K);
    KMG_TRY(check_index8_room(form == kErrorIndex8, "k", k, false));
    KMG_TRY(check_image(p, src_rgba, w, h));
    if (!out || !stats) return fail(KMG_ERR_INVALID_ARGUMENT, "output or statistics pointer is NULL");
    CallStart c;
    c.snapshot(p);
    KMG_TRY(check_index8_room(form == kErrorIndex8, "k", k, c.alpha_cutoff != 0));
    KMG_TRY(c.begin(p, src_rgba, w, h));
    hipStream_t st = c.sg.st;
    const size_t n = (size_t)w * h, out_bytes = n * format_bytes(format);
    StreamBuf res, rec;
    HIP_TRY(res.alloc(p, out_bytes, st));
    HIP_TRY(copy_host_image(p, res.ptr, out, out_bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(rec.alloc(p, sizeof(kmg_error_stats), st));
    HIP_TRY(hipMemsetAsync(rec.ptr, 0, sizeof(kmg_error_stats), st));
    KMG_TRY_DRAIN(st, dev_compare_form(p, c.d_rgba(), res.ptr, n, form, palette_rgba, k, c.alpha_cutoff, what, (kmg_error_stats *)rec.ptr, st));
    HIP_TRY(hipMemcpyAsync(stats, rec.ptr, sizeof(kmg_error_stats), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return KMG_OK;
}
KMG_ABI_CATCH

namespace {

int quality_of_working(kmg_processor *p, const uint8_t *d_rgba, uint32_t w, uint32_t h, const WorkingImage &wi, uint32_t k_min, uint32_t k_max,
                       uint32_t target, int mode, int format, uint32_t alpha_cutoff, const FixedList &fixed, hipStream_t st,
                       uint8_t *out_palette_rgba, uint32_t *out_count, void *out, kmg_error_stats *achieved, int *reached, uint32_t *total_runs)
{
    const uint64_t nw = (uint64_t)wi.sw * wi.sh;
    StreamBuf labels, rec;
    HIP_TRY(labels.alloc(p, (size_t)nw * 4, st));
    HIP_TRY(rec.alloc(p, sizeof(kmg_error_stats), st));

    // one candidate: the palette pipeline on W at k (a new Lloyd problem), the labels of W, the palette bytes, the statistics
    std::vector<float> c4(4 * (size_t)k_max), best_c4;
    std::vector<uint8_t> pal(4 * (size_t)k_max);
    kmg_error_stats cur, best;
    uint32_t runs = 0;
    auto evaluate = [&](uint32_t k, bool *accepted) -> int {
        KMG_TRY(palette_of_working(p, wi, k, st, c4.data(), fixed, (uint32_t *)labels.ptr));
        for (uint32_t i = 0; i < k; ++i) shader_lab_to_rgba8(&c4[4 * i], &pal[4 * i]);
        HIP_TRY(hipMemsetAsync(rec.ptr, 0, sizeof(kmg_error_stats), st));
        KMG_TRY(dev_compare_form(p, wi.src, labels.ptr, nw, kErrorLabel32, pal.data(), k, 0, KMG_ERROR_RGB | KMG_ERROR_LAB,
                                 (kmg_error_stats *)rec.ptr, st));
        HIP_TRY(hipMemcpyAsync(&cur, rec.ptr, sizeof cur, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        ++runs;
        *accepted = cur.lab_sse <= (uint64_t)target * nw;
        if (log_debug())
            fprintf(stderr, "[kmeans_hip] reduce_quality: k = %u, E = %llu, limit %llu: %s\n", k, (unsigned long long)cur.lab_sse,
                    (unsigned long long)((uint64_t)target * nw), *accepted ? "accepted" : "not accepted");
        return KMG_OK;
    };
    auto keep = [&](uint32_t k) { best = cur; best_c4.assign(c4.begin(), c4.begin() + 4 * (size_t)k); };

    bool ok = false;
    uint32_t k_star = k_max;
    KMG_TRY(evaluate(k_max, &ok));
    keep(k_max);
    const int did_reach = ok ? 1 : 0;
    if (ok) {
        uint32_t lo = k_min, hi = k_max;
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo) / 2;
            KMG_TRY(evaluate(mid, &ok));
            if (ok) { hi = mid; keep(mid); }
            else lo = mid + 1;
        }
        k_star = hi;
    }
    KMG_TRY(apply_and_download(p, d_rgba, w, h, best_c4.data(), k_star, mode, alpha_cutoff, st, (uint8_t *)out, format));
    for (uint32_t i = 0; i < k_star; ++i) shader_lab_to_rgba8(&best_c4[4 * i], out_palette_rgba + 4 * i);
    *out_count = k_star;
    if (achieved) *achieved = best;
    if (reached) *reached = did_reach;
    if (total_runs) *total_runs += runs;
    if (log_debug()) fprintf(stderr, "[kmeans_hip] reduce_quality: k* = %u after %u palette runs\n", k_star, runs);
    return KMG_OK;
}

}  // namespace

extern "C" int kmg_reduce_quality(kmg_processor *p, const uint8_t *rgba, uint32_t w, uint32_t h, uint32_t k_min, uint32_t k_max,
                                  uint32_t target, int mode, int format, uint8_t *out_palette_rgba, uint32_t *out_count, void *out,
                                  kmg_error_stats *achieved, int *reached)
try {
    // (the refusals that need no device come first)
    if (k_min < 1 || k_min > k_max || k_max > KMG_MAX_K)
        return fail(KMG_ERR_INVALID_ARGUMENT, "colour counts [%u, %u]: 1 <= k_min <= k_max <= %u", k_min, k_max, KMG_MAX_K);
    KMG_TRY(check_mode(mode));
    KMG_TRY(check_format(format));
    KMG_TRY(check_meld_format(mode, format));
    KMG_TRY(check_index8_room(format == KMG_FORMAT_INDEX8, "k_max", k_max, false));
    KMG_TRY(check_image(p, rgba, w, h));
    if (!out || !out_palette_rgba || !out_count) return fail(KMG_ERR_INVALID_ARGUMENT, "output pointer is NULL");
    CallStart c;
    c.snapshot(p);
    KMG_TRY(check_fixed(c.fixed, k_min, KMG_ALGO_KMEANS, c.weighting));
    KMG_TRY(check_index8_room(format == KMG_FORMAT_INDEX8, "k_max", k_max, c.alpha_cutoff != 0));
    KMG_TRY(c.begin(p, rgba, w, h));
    hipStream_t st = c.sg.st;
    WorkingImage wi;                                                   // uploaded, shrunk and compacted once
    KMG_TRY(working_image(p, c.d_rgba(), w, h, c.alpha_cutoff, c.weighting, st, wi));
    return quality_of_working(p, c.d_rgba(), w, h, wi, k_min, k_max, target, mode, format, c.alpha_cutoff, c.fixed, st, out_palette_rgba, out_count,
                              out, achieved, reached, nullptr);
}
KMG_ABI_CATCH

extern "C" int kmg_reduce_quality_batch(kmg_processor *p, uint32_t n_images, const uint8_t *const *rgba, const uint32_t *widths,
                                        const uint32_t *heights, uint32_t k_min, uint32_t k_max, uint32_t target, int mode, int format,
                                        uint64_t max_resident_bytes, uint8_t *const *out_palette_rgba, uint32_t *out_counts,
                                        void *const *out, kmg_error_stats *achieved, int *reached, kmg_batch_quality_report *report)
try {
    BatchCall call{BatchKind::kQuality, p, n_images, rgba, widths, heights, k_max, KMG_ALGO_KMEANS, mode, format, max_resident_bytes,
                   (uint8_t *const *)out, out_palette_rgba, out_counts, k_min, target, achieved, reached};
    KMG_TRY(call.run(nullptr));
    if (report) *report = call.qrep;
    return KMG_OK;
}
KMG_ABI_CATCH
