// kmg_internal.h -- what the translation units of libkmeans_hip share besides the kernels' launchers: the error
// channel of the C ABI and the few host helpers of kmg_api.hip / kmg_processor.hip that the multi-device layer (kmg_group.hip) reuses.
// Nothing here is exported (-fvisibility=hidden).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <array>
#include <vector>

#include "../../include/kmeans_hip.h"
#include "kmg_dither_map.h"

// Tuning switches and knock-outs (kernel variants that skip work and return WRONG results, for measurements) exist only in the
// tools build (make tools: -DKMG_TOOLS, lib/libkmeans_hip_tools.so, loaded by tools/ through KMG_LIBRARY).  In the product
// library the environment is not even consulted for them: KMG_TOOLS_ENV is a macro so that the variable's name is not in the
// binary, and KMG_KNOCK(flags, bit) is a constant so that the knocked-out paths are not compiled.
#ifdef KMG_TOOLS
#include <stdlib.h>
#define KMG_TOOLS_ENV(name) getenv(name)
#define KMG_KNOCK(flags, bit) (((flags) & (bit)) != 0u)
#else
#define KMG_TOOLS_ENV(name) (static_cast<const char *>(nullptr))
#define KMG_KNOCK(flags, bit) (false)
#endif

#include <stdlib.h>
static inline int tools_env_int(const char *e, int dflt) { return e ? atoi(e) : dflt; }

namespace kmg {

// sets the calling thread's kmg_last_error() message and returns `code`
int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
bool log_debug();
// a HIP call that failed where HIP_TRY does not fit (the caller has something to release first): "<what> failed: <HIP's words>",
// out of memory told apart from every other error
static inline int fail_hip(hipError_t e, const char *what)
{
    return fail(e == hipErrorOutOfMemory ? KMG_ERR_OUT_OF_MEMORY : KMG_ERR_HIP, "%s failed: %s", what, hipGetErrorString(e));
}

// No C++ exception leaves the library: the callers of this ABI are C, Rust (rust-shim/) and ctypes, for which an exception that
// unwinds through an extern "C" frame is undefined behaviour, where the reference returns anyhow::Result (core/src/lib.rs:38).
// Every extern "C" definition is a function-try-block closed by one of the macros below; abi_trap() names what was caught:
// std::bad_alloc -> KMG_ERR_OUT_OF_MEMORY, any other std::exception -> KMG_ERR_HIP with what() in kmg_last_error(), anything
// else -> KMG_ERR_HIP.  (tests/test_abi.py checks that no definition is left out.)
int abi_trap() noexcept;
#define KMG_ABI_CATCH      catch (...) { return kmg::abi_trap(); }
#define KMG_ABI_CATCH_VOID catch (...) { (void)kmg::abi_trap(); }
#define KMG_ABI_CATCH_NULL catch (...) { (void)kmg::abi_trap(); return nullptr; }

// early return from a function that returns a status: a HIP call that failed (the message names it), a library call that failed
// (it has set the message itself)
#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return fail(e_ == hipErrorOutOfMemory ? KMG_ERR_OUT_OF_MEMORY : KMG_ERR_HIP,       \
                        "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

#define KMG_TRY(expr)                                                                          \
    do {                                                                                       \
        const int rc_ = (expr);                                                                \
        if (rc_ != KMG_OK) return rc_;                                                         \
    } while (0)

// lib.rs:255-286 kmeans_palette: CentroidsBuffer::pull_values (palette-crate Lab -> sRGB8) of a k-means centroid table, then
// sorted ascending by the palette-crate Lab L of the 8-bit colour.  out_rgba: k x 4 bytes.
void sorted_palette_of(const float *centroids4, uint32_t k, uint8_t *out_rgba);
// lib.rs:288-331 octree_palette on a host image already shrunk to <= 128: the reference's CPU octree, sorted by L
std::vector<std::array<uint8_t, 4>> octree_sorted_palette(const uint8_t *host_rgba, uint64_t n_pixels, uint32_t color_count);
// an octree's colour list -> centroid table, 4 floats per colour (kmg_api.hip): refuses an empty list and one of more than KMG_MAX_K
int octree_centroids(const std::vector<std::array<uint8_t, 4>> &colors, std::vector<float> &centroids4);

// kmg_dev_apply with the alpha cutoff given (kmg_apply.hip): the host-buffer calls read the processor's once per call
// filter: the kmg_diffusion of KMG_MODE_DIFFUSE, or -1 = the processor's switch as it is now (an open sequence output hands on its own)
// dither: the map and strength of KMG_MODE_DITHER (*dither null: the default), or NULL = the processor's choice as it is now
int dev_apply(kmg_processor *p, const uint8_t *d_rgba, uint32_t w, uint32_t rows, uint32_t row0, const float *centroids4, uint32_t k,
              int mode, uint8_t *d_out, void *stream, uint32_t alpha_cutoff, int format = KMG_FORMAT_RGBA8, int filter = -1,
              const DitherPtr *dither = nullptr);
// the dither choice set on a processor right now (kmg_processor.hip; kmg_processor_set_dither[_custom]), null = the default
DitherPtr dither_snapshot(kmg_processor *p);
// the box of the index formats (include/kmeans_hip.h at kmg_output_format)
constexpr float kIndexBoxLmin = -100.0f, kIndexBoxLmax = 200.0f, kIndexBoxAB = 300.0f;
// the rules of the index formats for a centroid table (kmg_apply.hip): the mode has an index, k fits the format, every centroid lies
// in the box
int check_index_format(const float *centroids4, uint32_t k, int mode, int format, uint32_t alpha_cutoff);
// The output pass of many images in device memory (kmg_batch_apply.hip; include/kmeans_hip.h at kmg_batch_apply_report), arguments
// already checked: the images that join (batch_apply_joins, kmg_apply_route.h) through the batched launch, the others through
// dev_apply one by one.  centroids4: n_tables (1 or n_images) tables of k.  ADDS to report's launches, batched and per_image.
// Synchronises `st`.
int apply_batch(kmg_processor *p, uint32_t n_images, const uint8_t *const *d_src, const uint32_t *widths, const uint32_t *heights,
                const float *centroids4, uint32_t n_tables, uint32_t k, int mode, int format, uint32_t alpha_cutoff, void *const *d_out,
                kmg_batch_apply_report *report, hipStream_t st, int filter = -1, const DitherPtr *dither = nullptr);
// apply_batch into one stream-ordered block (kmg_batch_layout.h: every image at a 16-byte aligned offset), then the images'
// outputs to the host buffers out[i].  Synchronises `st`.
int apply_batch_download(kmg_processor *p, uint32_t n_images, const uint8_t *const *d_src, const uint32_t *widths, const uint32_t *heights,
                         const float *centroids4, uint32_t n_tables, uint32_t k, int mode, int format, uint32_t alpha_cutoff,
                         uint8_t *const *out, kmg_batch_apply_report *report, hipStream_t st);

// The k-means palette step on a working image (kmg_api.hip): sw x sh pixels in device memory -> host centroid table, a new Lloyd
// problem of k centroids (initialisation + loop with the processor's options).  Synchronises `st`.  d_labels: optional label map.
// fixed4 / n_fixed (kmg_processor_set_fixed_colors; n_fixed <= k): the Lab of the pinned entries -- centroids 0 .. n_fixed - 1 start
// there and stay, the rest is initialised and moves around them.  weighting (KMG_WEIGHT_*): the loop's sums weigh each pixel by its
// alpha byte; the initialisation does not.  iterations (may be NULL): where kmg_lloyd_run stopped.
int palette_of_working(kmg_processor *p, const uint8_t *d_src, uint32_t sw, uint32_t sh, uint32_t k, hipStream_t st, float *centroids4,
                       uint32_t *d_labels = nullptr, const float *fixed4 = nullptr, uint32_t n_fixed = 0, int weighting = KMG_WEIGHT_NONE,
                       uint32_t *iterations = nullptr);
// kmg_dev_palette_batch on a hipStream_t (kmg_batch.hip): the k-means palette step of many working images in device memory, the
// small ones through the batched kernels.  Synchronises `st`.
int dev_palette_batch(kmg_processor *p, uint32_t n_images, const uint8_t *const *d_rgba, const uint32_t *widths, const uint32_t *heights,
                      uint32_t k, float *centroids4, uint32_t *iterations, kmg_batch_report *report, hipStream_t st);
// kmg_dev_palette_batch_counts, arguments already checked: image i has ks[i] colours, its table starts at centroids4[4 * (ks[0] + ... +
// ks[i - 1])].  launches: the largest count + 2 + the most iterations, per piece.
int dev_palette_batch_counts(kmg_processor *p, uint32_t n_images, const uint8_t *const *d_rgba, const uint32_t *widths, const uint32_t *heights,
                             const uint32_t *ks, float *centroids4, uint32_t *iterations, kmg_batch_report *report, hipStream_t st);
// apply_batch with a count per image: image i has ks[i] colours and the table at centroids4[at[i]] (shared: every image the table
// of the first, all ks equal).  The joined images go out as at most two chains of launches, those below k = 32 and the others.
int apply_batch_counts(kmg_processor *p, uint32_t n_images, const uint8_t *const *d_src, const uint32_t *widths, const uint32_t *heights,
                       const float *centroids4, const size_t *at, const uint32_t *ks, bool shared, int mode, int format, uint32_t alpha_cutoff,
                       void *const *d_out, kmg_batch_apply_report *report, hipStream_t st, int filter = -1, const DitherPtr *dither = nullptr);
int apply_batch_counts_download(kmg_processor *p, uint32_t n_images, const uint8_t *const *d_src, const uint32_t *widths, const uint32_t *heights,
                                const float *centroids4, const size_t *at, const uint32_t *ks, int mode, int format, uint32_t alpha_cutoff,
                                uint8_t *const *out, kmg_batch_apply_report *report, hipStream_t st);
// kmg_dev_compare_batch on a hipStream_t, arguments already checked (kmg_batch_error.hip): COMBINES into the n_images records at
// d_stats.  Only enqueues; its scratch goes back to the pool in stream order.  launches (may be NULL): ADDS the statistics launches.
int dev_compare_batch(kmg_processor *p, uint32_t n_images, const uint8_t *const *d_src, const void *const *d_out, const uint64_t *n_pixels,
                      int format, const uint8_t *palettes_rgba, const uint32_t *ks, uint32_t alpha_cutoff, uint32_t what,
                      kmg_error_stats *d_stats, hipStream_t st, uint32_t *launches);
// the weighting set on a processor right now (kmg_processor.hip; kmg_processor_set_weighting)
int processor_weighting(kmg_processor *p);
// the number of fixed colours set on a processor right now (kmg_processor.hip; kmg_processor_set_fixed_colors)
uint32_t processor_fixed_count(kmg_processor *p);
// KMG_MODE_DIFFUSE: the plan's next run starts a new image (row0 = 0, zero error above it) instead of continuing the last one
// (kmg_apply.hip).  The caller has every earlier run of the plan behind it on the stream of the next one.  Other modes: nothing.
void apply_plan_restart(kmg_apply_plan *plan);

// The argument checks of the two delta passes, in one order (kmg_sequence.hip): `name` prefixes the messages; lossy: the call has
// the two RGBA8 buffers d_src / d_held and a hold record (exact: both NULL, a delta record).
int check_index_band(const char *name, bool lossy, const kmg_processor *p, const void *d_index, const void *d_canvas, const void *d_delta,
                     const void *d_src, const void *d_held, const void *d_info, uint32_t width, uint32_t rows, uint32_t row0, int format,
                     uint32_t k);
// kmg_dev_frame_delta_lossy on a hipStream_t (kmg_hold.hip): the sequence layer's lossy frames
int frame_hold_impl(kmg_processor *p, const uint8_t *d_src_rgba, const void *d_index, void *d_canvas, uint8_t *d_held_rgba, uint32_t width,
                    uint32_t rows, uint32_t row0, int format, uint32_t k, uint32_t tolerance, void *d_delta, kmg_frame_hold *d_info,
                    hipStream_t st);
// kmg_dev_frame_delta_clip on a hipStream_t (kmg_clip.hip): every frame of a clip through the delta passes in one launch chain.
// launches (may be NULL): ADDS the launches of the two clip kernels.  Only enqueues.
int frame_clip_impl(kmg_processor *p, uint32_t n_frames, const uint8_t *const *d_src_rgba, const void *const *d_index, void *d_canvas,
                    uint8_t *d_held_rgba, uint32_t width, uint32_t height, int format, uint32_t k, const uint32_t *tolerances, uint32_t flags,
                    void *const *d_out, kmg_frame_hold *d_info, uint32_t *d_full, uint32_t *launches, hipStream_t st);
// the alpha cutoff a plan was made with (kmg_apply.hip)
uint32_t apply_plan_cutoff(const kmg_apply_plan *plan);
// the diffusion filter a plan was made with (kmg_apply.hip)
int apply_plan_filter(const kmg_apply_plan *plan);
// the dither choice a plan was made with (kmg_apply.hip), null = the default
const DitherPtr &apply_plan_dither(const kmg_apply_plan *plan);

// kmg_dev_frame_delta_colour / _colour_lossy on a hipStream_t (kmg_local.hip): the frames of an output with per-frame palettes.
// lossy: d_src_rgba, d_held_rgba and a hold record; exact: both NULL and a delta record
int frame_local_impl(kmg_processor *p, const uint8_t *d_src_rgba, const void *d_index, const uint8_t *d_palette_rgba, uint8_t *d_shown_rgba,
                     uint8_t *d_held_rgba, uint32_t width, uint32_t rows, uint32_t row0, int format, uint32_t k, bool lossy, uint32_t tolerance,
                     void *d_delta, void *d_info, hipStream_t st);
// The centroids of one frame of such an output (kmg_api.hip): the working image of kmg_reduce_indexed's k-means step for the frame in
// device memory, then -- warm4 == NULL -- that step itself with the fixed colours given, or -- warm4: k x 4 -- the Lloyd loop from
// those k centroids (a seeded initialisation with every centroid given: no pick).  Synchronises `st`.  weighting: KMG_WEIGHT_* (the
// working image is then cut at max(alpha_cutoff, 1) and both loops are weighted).
int local_frame_centroids(kmg_processor *p, const uint8_t *d_rgba, uint32_t w, uint32_t h, uint32_t k, uint32_t alpha_cutoff, hipStream_t st,
                          float *centroids4, const float *fixed4, uint32_t n_fixed, const float *warm4, int weighting = KMG_WEIGHT_NONE);

// An image between a caller's (pageable) buffer and the device, ordered on `st` (kmg_api.hip): small images asynchronously,
// large ones as synchronous row-range copies on several streams of the processor.
hipError_t copy_host_image(kmg_processor *p, void *dst, const void *src, size_t bytes, hipMemcpyKind kind, hipStream_t st);

}  // namespace kmg
