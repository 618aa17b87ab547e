// kmg_apply.hip -- the output passes of the C ABI (find_colors / dither_colors / meld_colors, core/src/operations.rs:99-155,
// 215-271): kmg_apply_plan_*, kmg_dev_apply and the exhaustive checks of their candidate masks / lists.  Which route a plan takes
// is decided by apply_route (kmg_apply_route.h, with the cost models); here a route is named in three places only: the list of its
// scratch parts, the switch that builds them and the switch that runs a band.

#include "kmg_state.h"
#include "kmg_apply_route.h"

static_assert(kRouteListMaxK == kLabListMaxK && kRouteModeDither == KMG_MODE_DITHER && kRouteModeMeld == KMG_MODE_MELD &&
              kRouteModeDiffuse == KMG_MODE_DIFFUSE, "kmg_apply_route.h repeats these constants");

// a HIP call inside a function that returns hipError_t
#define HIP_PASS(expr)                                                                         \
    do {                                                                                       \
        const hipError_t e_ = (expr);                                                          \
        if (e_ != hipSuccess) return e_;                                                       \
    } while (0)

// the (L, a, b, chroma) table of a caller's k x 4 floats
static std::vector<Centroid> centroids_of(const float *c4, uint32_t k)
{
    std::vector<Centroid> hc(k);
    for (uint32_t i = 0; i < k; ++i) hc[i] = {c4[4 * i], c4[4 * i + 1], c4[4 * i + 2], chroma(c4[4 * i + 1], c4[4 * i + 2])};
    return hc;
}

// test support: exhaustive validation of the candidate masks (kmg_table.hip) and, for k <= kLabListMaxK, of the byte lists over Lab
// cells (kmg_lists.hip, same counter) for a centroid table.  *violations must come back 0.
//   dither: over all 2^24 colours x 16 Bayer offsets, the arg-min over the candidates must equal the brute-force arg-min;
//   meld (k >= 2): over all 2^24 colours the two closest centroids found among the cell's candidates must be those of the full scan.
static int check_candidates(kmg_processor *p, const float *c4, uint32_t k, bool dither, uint64_t *violations, hipStream_t st)
{
    HIP_TRY(hipSetDevice(p->device));
    KMG_TRY(ensure_bounds(p, st));
    const std::vector<Centroid> hc = centroids_of(c4, k);
    const float thr = dither ? dither_threshold(c4, k) : 0.0f;
    DevBuf cent, masks, viol, lists;
    HIP_TRY(cent.alloc(sizeof(Centroid) * k));
    HIP_TRY(masks.alloc(sizeof(uint64_t) * (size_t)kCells * (dither ? 16u : 1u) * mask_words(k)));
    HIP_TRY(viol.alloc(sizeof(unsigned long long)));
    HIP_TRY(hipMemcpyAsync(cent.ptr, hc.data(), sizeof(Centroid) * k, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(viol.ptr, 0, sizeof(unsigned long long), st));
    const Centroid *d_cent = (const Centroid *)cent.ptr;
    uint64_t *d_masks = (uint64_t *)masks.ptr;
    unsigned long long *d_viol = (unsigned long long *)viol.ptr;
    if (dither) {
        HIP_TRY(launch_offset_candidates(p->d_bounds, d_cent, k, thr, d_masks, st));
        HIP_TRY(launch_check_offset_masks(d_cent, k, d_masks, p->d_lut, thr, d_viol, st));
    } else {
        HIP_TRY(launch_meld_candidates(p->d_bounds, d_cent, k, d_masks, st));
        HIP_TRY(launch_check_meld_masks(d_cent, k, d_masks, p->d_lut, d_viol, st));
    }
    if (k <= kLabListMaxK) {
        HIP_TRY(lists.alloc(lab_list_bytes(k)));
        HIP_TRY(launch_lab_candidates(d_cent, k, thr, !dither, (uint8_t *)lists.ptr, st));
        HIP_TRY(dither ? launch_check_lab_lists(d_cent, k, (const uint8_t *)lists.ptr, p->d_lut, thr, d_viol, st)
                       : launch_check_lab_lists_two(d_cent, k, (const uint8_t *)lists.ptr, p->d_lut, d_viol, st));
    }
    unsigned long long h = 0;
    HIP_TRY(hipMemcpyAsync(&h, viol.ptr, sizeof h, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *violations = h;
    if (dither && KMG_TOOLS_ENV("KMG_DITHER_STATS")) {
        // distribution of the candidate counts: per (cell, Bayer index) slot, and per cell over its 16 slots together
        const uint32_t words = mask_words(k);
        std::vector<uint64_t> hm((size_t)kCells * 16u * words);
        HIP_TRY(hipMemcpy(hm.data(), masks.ptr, hm.size() * 8, hipMemcpyDeviceToHost));
        uint64_t hs[34] = {0}, hu[34] = {0};
        for (uint32_t c = 0; c < kCells; ++c) {
            std::vector<uint64_t> u(words, 0);
            for (uint32_t b = 0; b < 16; ++b) {
                uint32_t n = 0;
                for (uint32_t w = 0; w < words; ++w) { const uint64_t m = hm[((size_t)c * 16 + b) * words + w]; u[w] |= m; n += (uint32_t)__builtin_popcountll(m); }
                hs[n < 33 ? n : 33]++;
            }
            uint32_t n = 0;
            for (uint32_t w = 0; w < words; ++w) n += (uint32_t)__builtin_popcountll(u[w]);
            hu[n < 33 ? n : 33]++;
        }
        fprintf(stderr, "dither candidates per slot :");
        for (int i = 0; i < 34; ++i) fprintf(stderr, " %.4f", (double)hs[i] / (kCells * 16.0));
        fprintf(stderr, "\ndither candidates per cell (union of 16 slots):");
        for (int i = 0; i < 34; ++i) fprintf(stderr, " %.4f", (double)hu[i] / kCells);
        fprintf(stderr, "\n");
    }
    return KMG_OK;
}

extern "C" int kmg_debug_check_dither_masks(kmg_processor *p, const float *c4, uint32_t k, uint64_t *violations, void *stream)
try {
    if (!p || !c4 || !violations || k < 2 || k > KMG_MAX_K) return fail(KMG_ERR_INVALID_ARGUMENT, "bad check_dither_masks arguments");
    return check_candidates(p, c4, k, true, violations, S(stream));
}
KMG_ABI_CATCH

extern "C" int kmg_debug_check_meld_masks(kmg_processor *p, const float *c4, uint32_t k, uint64_t *violations, void *stream)
try {
    if (!p || !c4 || !violations || k < 2 || k > KMG_MAX_K) return fail(KMG_ERR_INVALID_ARGUMENT, "bad check_meld_masks arguments");
    return check_candidates(p, c4, k, false, violations, S(stream));
}
KMG_ABI_CATCH

#ifdef KMG_TOOLS
namespace kmg {
hipError_t launch_dither_list_stats(const uint32_t *rgba, uint32_t w, uint32_t rows, uint32_t row0, const float *lut, float threshold,
                                    const uint8_t *lists, unsigned long long *out68, hipStream_t st);
}
// tools build: list lengths of the dither pass over an image (k <= 256): out[68] as k_dither_list_stats leaves them
extern "C" KMG_API int kmg_tools_dither_list_stats(kmg_processor *p, const uint8_t *d_rgba, uint32_t w, uint32_t rows, const float *c4, uint32_t k,
                                                  unsigned long long *out68)
try {
    if (!p || !d_rgba || !c4 || !out68 || k < 2 || k > 256) return fail(KMG_ERR_INVALID_ARGUMENT, "bad dither_list_stats arguments");
    HIP_TRY(hipSetDevice(p->device));
    const std::vector<Centroid> hc = centroids_of(c4, k);
    const float thr = dither_threshold(c4, k);
    DevBuf cent, lists, acc;
    HIP_TRY(cent.alloc(sizeof(Centroid) * k));
    HIP_TRY(lists.alloc(lab_list_bytes(k)));
    HIP_TRY(acc.alloc(sizeof(unsigned long long) * 68));
    HIP_TRY(hipMemcpy(cent.ptr, hc.data(), sizeof(Centroid) * k, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(acc.ptr, 0, sizeof(unsigned long long) * 68));
    HIP_TRY(launch_lab_candidates((const Centroid *)cent.ptr, k, thr, false, (uint8_t *)lists.ptr, nullptr));
    HIP_TRY(launch_dither_list_stats((const uint32_t *)d_rgba, w, rows, 0u, p->d_lut, thr, (const uint8_t *)lists.ptr, (unsigned long long *)acc.ptr, nullptr));
    HIP_TRY(hipMemcpy(out68, acc.ptr, sizeof(unsigned long long) * 68, hipMemcpyDeviceToHost));
    return KMG_OK;
}
KMG_ABI_CATCH
#endif

// ---- the output pass as a PLAN: everything that depends on the centroid table only -- the device copy of centroids and palette,
// the threshold, the candidate lists / masks or the label tables of the colour cube -- is built once (asynchronously on the
// creating call's stream); kmg_apply_plan_run then launches the per-pixel kernel for any band of rows on any stream, without a
// host synchronisation, so a caller that streams an image in bands (or runs bands on several streams) overlaps copies and
// kernels.  kmg_dev_apply = create + run + synchronise + destroy.
struct kmg_apply_plan {
    kmg_processor *p = nullptr;
    uint32_t k = 0;
    int mode = 0;
    int format = KMG_FORMAT_RGBA8;      // kmg_output_format of what _run writes
    uint32_t alpha_cutoff = 0;          // kmg_options.alpha_cutoff when the plan was made (0: alpha ignored)
    int filter = KMG_DIFFUSION_FLOYD_STEINBERG;   // kmg_processor_set_diffusion when the plan was made (KMG_MODE_DIFFUSE reads it)
    bool dither = false;
    float thr = 0.0f;
    // kmg_processor_set_dither[_custom] when the plan was made (KMG_MODE_DITHER reads it): null = the default, the kernels that carry
    // the reference's matrix; else the plan's copy of the map, its v in the scratch block (d_v) and t = thr * strength
    DitherPtr choice;
    float *d_v = nullptr;
    float t = 0.0f;
    Route route = Route::kScan;
    ArenaGuard arena;
    std::vector<uint8_t> staged;        // host copy of the tables: lives as long as the asynchronous upload may
    Centroid *d_cent = nullptr;
    uint32_t *d_pal = nullptr;
    uint32_t *d_ident = nullptr;        // index formats, kDitherMasks: the identity table (entry i = i) its kernels take as palette
    void *aux = nullptr;                // candidate lists / masks, or the per-colour labels (kReplaceTable)
    uint16_t *sub = nullptr;            // kReplaceTable: the label pass's first-level tables
    hipEvent_t ready = nullptr;         // the tables are built (recorded on the creating stream)
    hipStream_t built_on = nullptr;
    // KMG_MODE_DIFFUSE: the diffusion continues across the bands of consecutive runs
    // dstate: 4 x width packed error rows (Floyd-Steinberg uses the first 2 x width), the sticky timeout word (zeroed once), the per-call control block (kmg_diffuse.hip);
    // stream-ordered from the processor's pool on the first run's stream, given back on `built_on` (every stream is idle by then)
    void *dstate = nullptr;
    uint32_t dwidth = 0, drows = 0, dparity = 0;
    hipEvent_t ddone = nullptr;         // the previous run's pass has completed (the next one waits on it, on any stream)
    void *h_slot = nullptr;             // page-locked slot of the processor (host_slot_take) for the sticky word's read-back
    uint32_t h_word = 0;                // (the same in pageable memory when no slot is left)
    volatile uint32_t *h_timeout = &h_word;
    ~kmg_apply_plan()
    {
        if (dstate) (void)hipFreeAsync(dstate, built_on);
        if (ddone) (void)hipEventDestroy(ddone);
        if (h_slot) host_slot_give(p, h_slot);
    }
};

// The index formats (include/kmeans_hip.h at kmg_output_format): the mode has an index, k fits the format (with the transparent
// slot in alpha mode), and every centroid lies in the box inside which the dither scan's sentinel never wins.
int kmg::check_index_format(const float *c4, uint32_t k, int mode, int format, uint32_t alpha_cutoff)
{
    KMG_TRY(check_format(format));                                     // (the caller has dealt with KMG_FORMAT_RGBA8)
    KMG_TRY(check_meld_format(mode, format));
    KMG_TRY(check_index8_room(format == KMG_FORMAT_INDEX8, "k", k, alpha_cutoff != 0));
    for (uint32_t i = 0; i < k; ++i) {
        const float L = c4[4 * i], a = c4[4 * i + 1], b = c4[4 * i + 2];
        if (!(L >= kIndexBoxLmin && L <= kIndexBoxLmax && a >= -kIndexBoxAB && a <= kIndexBoxAB && b >= -kIndexBoxAB && b <= kIndexBoxAB))
            return fail(KMG_ERR_INVALID_ARGUMENT, "centroid %u (%g, %g, %g) is outside L in [-100, 200], a, b in [-300, 300] (index formats)",
                        i, (double)L, (double)a, (double)b);
    }
    return KMG_OK;
}

// What a route keeps in the plan's scratch block behind the centroid table and the palette: the parts in the order the build (the
// switch of plan_create) takes them, and whether the identity table rides behind the palette.  Sizing and building both read this.
struct RouteScratch {
    bool ident = false;
    std::vector<size_t> parts;
};

static RouteScratch route_scratch(Route route, uint32_t k, bool index_format)
{
    const size_t masks_bytes = sizeof(uint64_t) * (size_t)kCells * mask_words(k);
    switch (route) {
    case Route::kScan:
    case Route::kMeldScan:
    case Route::kDiffuseScan:
        return {};
    case Route::kMeldLists:
    case Route::kDitherLists:
        return {false, {lab_list_bytes(k)}};
    case Route::kMeldMasks:
        return {false, {masks_bytes}};
    case Route::kDitherMasks:                                          // (index output: its kernel writes pal[label] with pal = the identity)
        return {index_format, {16u * masks_bytes}};
    case Route::kReplaceTable:
    case Route::kDiffuseTable:                                         // per-colour labels, first-level tables, the cube pass's scratch
        return {false, {(size_t)(k <= 256 ? 1 : 2) << 24, sub_table_bytes(), cube_masks_bytes(k), cube_work_bytes()}};
    }
    return {};
}

static int plan_create(kmg_processor *p, const float *c4, uint32_t k, int mode, uint64_t n_pixels_hint, void *stream,
                       uint32_t alpha_cutoff, kmg_apply_plan **out, int format = KMG_FORMAT_RGBA8, int filter = -1,
                       const DitherPtr *dither = nullptr)
{
    if (!p || !c4 || !out || k == 0) return fail(KMG_ERR_INVALID_ARGUMENT, "bad apply_plan arguments");
    *out = nullptr;
    KMG_TRY(check_k_limit(k));
    KMG_TRY(check_mode(mode));
    if (format != KMG_FORMAT_RGBA8) KMG_TRY(check_index_format(c4, k, mode, format, alpha_cutoff));
    HIP_TRY(hipSetDevice(p->device));
    const hipStream_t st = S(stream);
    kmg_apply_plan *pl = new (std::nothrow) kmg_apply_plan();
    if (!pl) return fail(KMG_ERR_OUT_OF_MEMORY, "host allocation failed");
    struct Undo { kmg_apply_plan *pl; ~Undo() { if (pl) { if (pl->ready) (void)hipEventDestroy(pl->ready); (void)hipStreamSynchronize(pl->built_on); delete pl; } } } undo{pl};
    pl->p = p; pl->k = k; pl->mode = mode; pl->format = format; pl->alpha_cutoff = alpha_cutoff; pl->built_on = st;
    pl->filter = filter >= 0 ? filter : p->diffusion.load(std::memory_order_relaxed);

    // per-centroid work on the host: (L,a,b,C) table, RGBA8 palette (lab_to_rgb.wgsl) with the sentinel's entry behind it
    // (mix_colors.wgsl:73), threshold
    const std::vector<Centroid> hc = centroids_of(c4, k);
    std::vector<uint32_t> pal(k + 1);
    const float sentinel[3] = {10000.0f, 10000.0f, 10000.0f};
    for (uint32_t i = 0; i <= k; ++i) {
        uint8_t px[4];
        shader_lab_to_rgba8(i < k ? c4 + 4 * i : sentinel, px);
        memcpy(&pal[i], px, 4);
    }
    pl->dither = (mode == KMG_MODE_DITHER) && k > 1;                   // mix_colors.wgsl:104-108
    pl->thr = pl->dither ? dither_threshold(c4, k) : 0.0f;
    if (pl->dither) pl->choice = dither ? *dither : dither_snapshot(p);
    const DitherChoice *map = pl->choice.get();
    const size_t map_bytes = map ? sizeof(float) * map->v.size() : 0u;
    if (map) {
        volatile float t = pl->thr * map->strength;                   // fp32, one rounding
        pl->t = t;
        if (apply_map_lds_bytes(k, (uint32_t)map->v.size()) > device_info().lds_max)
            return fail(KMG_ERR_UNSUPPORTED, "k = %u centroids and a %u x %u dither map need %zu bytes of LDS, the device gives a workgroup %zu", k,
                        map->mw, map->mh, apply_map_lds_bytes(k, (uint32_t)map->v.size()), device_info().lds_max);
    }

    // which route (by the number of pixels the plan is made for), and the scratch it needs: one block per plan
    const bool mask_words_only = (p->strategy.load(std::memory_order_relaxed) & KMG_STRATEGY_MASK_WORDS) != 0;
    pl->route = apply_route_mapped(map != nullptr, mode, k, n_pixels_hint, forced_strategy(p), mask_words_only);
    const RouteScratch scratch = route_scratch(pl->route, k, format != KMG_FORMAT_RGBA8);
    const size_t cent_bytes = sizeof(Centroid) * k, pal_bytes = sizeof(uint32_t) * (k + 1);
    const size_t ident_bytes = scratch.ident ? pal_bytes : 0u;
    const size_t tables_bytes = cent_bytes + pal_bytes + ident_bytes + map_bytes;   // (the map's v last: 4-byte aligned like the palette)
    size_t need = ArenaGuard::padded(tables_bytes);
    for (const size_t bytes : scratch.parts) need += ArenaGuard::padded(bytes);
    ArenaGuard &arena = pl->arena;
    HIP_TRY(arena.acquire(p, need));
    // centroid table and palette travel in one block (one copy)
    pl->staged.resize(tables_bytes);
    memcpy(pl->staged.data(), hc.data(), cent_bytes);
    memcpy(pl->staged.data() + cent_bytes, pal.data(), pal_bytes);
    if (scratch.ident) {
        uint32_t *id = (uint32_t *)(pl->staged.data() + cent_bytes + pal_bytes);
        for (uint32_t i = 0; i <= k; ++i) id[i] = i;
    }
    Centroid *d_cent = pl->d_cent = (Centroid *)arena.take(tables_bytes);
    pl->d_pal = (uint32_t *)((uint8_t *)d_cent + cent_bytes);
    if (scratch.ident) pl->d_ident = pl->d_pal + (k + 1);
    if (map) {
        memcpy(pl->staged.data() + cent_bytes + pal_bytes + ident_bytes, map->v.data(), map_bytes);
        pl->d_v = (float *)((uint8_t *)d_cent + cent_bytes + pal_bytes + ident_bytes);
    }
    void *part[4] = {nullptr, nullptr, nullptr, nullptr};
    for (size_t i = 0; i < scratch.parts.size(); ++i) part[i] = arena.take(scratch.parts[i]);
    pl->aux = part[0];
    HIP_TRY(hipMemcpyAsync(d_cent, pl->staged.data(), pl->staged.size(), hipMemcpyHostToDevice, st));

    switch (pl->route) {
    case Route::kScan:
    case Route::kMeldScan:
    case Route::kDiffuseScan:                                          // every pixel scans all centroids: nothing to build
        break;
    case Route::kMeldLists:
    case Route::kDitherLists:
        // candidate lists per cell of a grid over Lab, then a scan of the pixel's candidates only (meld: whatever can be one of the
        // two closest; its threshold is 0)
        // (a map: the reach of its own offsets t v, for speed only)
        if (map) HIP_TRY(launch_lab_candidates_range(d_cent, k, fminf(pl->t * map->vmin, pl->t * map->vmax), fmaxf(pl->t * map->vmin, pl->t * map->vmax),
                                                     false, (uint8_t *)part[0], st));
        else HIP_TRY(launch_lab_candidates(d_cent, k, pl->thr, mode == KMG_MODE_MELD, (uint8_t *)part[0], st));
        break;
    case Route::kMeldMasks:
        // large image: per colour cell, the centroids that can be one of a pixel's two closest
        KMG_TRY(ensure_bounds(p, st));
        HIP_TRY(launch_meld_candidates(p->d_bounds, d_cent, k, (uint64_t *)part[0], st));
        break;
    case Route::kDitherMasks:
        // dither on a large image above k = 512: mask words per (colour cell, Bayer index)
        KMG_TRY(ensure_bounds(p, st));
        HIP_TRY(launch_offset_candidates(p->d_bounds, d_cent, k, pl->thr, (uint64_t *)part[0], st));
        break;
    case Route::kReplaceTable:
    case Route::kDiffuseTable:
        // replace mode on a large image: the label of a pixel depends on its colour only, so label the
        // colour cube once (candidate masks + cube pass without sums) and emit pal[label] through the
        // label tables -- the same bit-exact machinery as the Lloyd label pass
        KMG_TRY(ensure_bounds(p, st));
        pl->sub = (uint16_t *)part[1];
        HIP_TRY(launch_cube(labels_only_pass(p, d_cent, k, st, (uint64_t *)part[2], part[3], part[0], pl->sub), st));
        break;
    }
    if (mode == KMG_MODE_DIFFUSE) {
        HIP_TRY(hipEventCreateWithFlags(&pl->ddone, hipEventDisableTiming));
        if ((pl->h_slot = host_slot_take(p)) != nullptr) pl->h_timeout = static_cast<uint32_t *>(pl->h_slot);
        *pl->h_timeout = 0;
    }
    HIP_TRY(hipEventCreateWithFlags(&pl->ready, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(pl->ready, st));
    undo.pl = nullptr;
    *out = pl;
    return KMG_OK;
}

extern "C" int kmg_apply_plan_create(kmg_processor *p, const float *c4, uint32_t k, int mode, uint64_t n_pixels_hint, void *stream,
                                     kmg_apply_plan **out)
try {
    if (!p) return fail(KMG_ERR_INVALID_ARGUMENT, "bad apply_plan arguments");
    return plan_create(p, c4, k, mode, n_pixels_hint, stream, p->alpha_cutoff.load(std::memory_order_relaxed), out);
}
KMG_ABI_CATCH

extern "C" int kmg_apply_plan_create_format(kmg_processor *p, const float *c4, uint32_t k, int mode, int format, uint64_t n_pixels_hint,
                                            void *stream, kmg_apply_plan **out)
try {
    if (!p) return fail(KMG_ERR_INVALID_ARGUMENT, "bad apply_plan arguments");
    return plan_create(p, c4, k, mode, n_pixels_hint, stream, p->alpha_cutoff.load(std::memory_order_relaxed), out, format);
}
KMG_ABI_CATCH

// KMG_MODE_DIFFUSE: one band of the diffusion.  The bands of one plan are consecutive rows of one image (row0 = the rows done
// so far, the width unchanged); each run waits on the previous run's completion event, so bands issued on several streams still
// execute in order, and each continues from the error row the previous one left in the plan's scratch.
static int check_diffuse_band(kmg_apply_plan *pl, uint32_t w, uint32_t row0)
{
    if (w > 0x7FFFFF00u) return fail(KMG_ERR_UNSUPPORTED, "diffusion needs a width below 2^31 - 256");
    if (row0 != pl->drows) return fail(KMG_ERR_INVALID_ARGUMENT, "diffusion band starts at row %u, the plan has done %u rows", row0, pl->drows);
    if (pl->drows && w != pl->dwidth) return fail(KMG_ERR_INVALID_ARGUMENT, "diffusion band has width %u, the image has %u", w, pl->dwidth);
    // an earlier band that timed out (the sticky word; known once a run after it has completed) fails every later run
    if (pl->drows && hipEventQuery(pl->ddone) == hipSuccess && *pl->h_timeout)
        return fail(KMG_ERR_HIP, "diffusion pass timed out");
    return KMG_OK;
}

static hipError_t run_diffuse(kmg_apply_plan *pl, const uint32_t *src, uint32_t w, uint32_t rows, void *d_out, hipStream_t st)
{
    kmg_processor *p = pl->p;
    const size_t sticky_off = pad256(diffuse_erow_bytes(w)), ctl_off = sticky_off + 16;
    const size_t ctl_bytes = (diffuse_ctl_bytes() + 15) & ~(size_t)15;
    if (!pl->dstate) {
        HIP_PASS(pool_alloc(p, &pl->dstate, ctl_off + ctl_bytes, st));
        HIP_PASS(hipMemsetAsync((uint8_t *)pl->dstate + sticky_off, 0, 16, st));
    }
    uint8_t *erow = (uint8_t *)pl->dstate, *ctl = erow + ctl_off;
    uint32_t *sticky = (uint32_t *)(erow + sticky_off);
    if (pl->drows) HIP_PASS(hipStreamWaitEvent(st, pl->ddone, 0));
    else {                                                             // no row above the image
        const size_t slot = diffuse_slot_bytes(pl->filter, w);
        HIP_PASS(hipMemsetAsync(erow + (size_t)pl->dparity * slot, 0, slot, st));
    }
    HIP_PASS(hipMemsetAsync(ctl, 0, ctl_bytes, st));
    const int route = pl->route != Route::kDiffuseTable ? kDiffuseScan : (pl->k <= 256 ? kDiffusePairs : kDiffuseCells);
    HIP_PASS(launch_diffuse(route, pl->filter, src, w, rows, d_out, pl->format, erow, pl->dparity, ctl, sticky, pl->d_cent, pl->k, p->d_lut,
                            pl->d_pal, pl->aux, pl->sub, st, pl->alpha_cutoff));
    HIP_PASS(hipMemcpyAsync((void *)pl->h_timeout, sticky, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_PASS(hipEventRecord(pl->ddone, st));
    pl->dwidth = w;
    pl->drows += rows;
    pl->dparity = (pl->dparity + (rows + 63u) / 64u) & 1u;
    return hipSuccess;
}

void kmg::apply_plan_restart(kmg_apply_plan *pl)
{
    if (pl) pl->drows = 0;
}

uint32_t kmg::apply_plan_cutoff(const kmg_apply_plan *pl) { return pl->alpha_cutoff; }

int kmg::apply_plan_filter(const kmg_apply_plan *pl) { return pl->filter; }

const DitherPtr &kmg::apply_plan_dither(const kmg_apply_plan *pl) { return pl->choice; }

// the plan's dither offsets as the launchers take them: the default choice is the reference's matrix at the plan's threshold
static MapOffsets plan_offsets(const kmg_apply_plan *pl)
{
    if (!pl->choice) return {pl->thr, {}};
    const DitherChoice &c = *pl->choice;
    return {pl->t, {pl->d_v, c.mw - 1u, c.mh - 1u, (uint32_t)__builtin_ctz(c.mw)}};
}

// kmg_dev_apply and kmg_apply_plan_status: did any diffusion run of the plan time out?  (Read after the last run has completed.)
static int diffuse_status(kmg_apply_plan *pl)
{
    if (pl->mode == KMG_MODE_DIFFUSE && *pl->h_timeout) return fail(KMG_ERR_HIP, "diffusion pass timed out");
    return KMG_OK;
}

extern "C" int kmg_apply_plan_status(kmg_apply_plan *pl)
try {
    if (!pl) return fail(KMG_ERR_INVALID_ARGUMENT, "bad apply_plan_status arguments");
    if (pl->mode != KMG_MODE_DIFFUSE || !pl->drows) return KMG_OK;
    HIP_TRY(hipSetDevice(pl->p->device));
    HIP_TRY(hipEventSynchronize(pl->ddone));                          // (the last run, and with it the read-back of the sticky word)
    return diffuse_status(pl);
}
KMG_ABI_CATCH

// The mask-word dither route.  RGBA8: its kernel lives in kmg_table.hip and knows no alpha, so k_alpha_merge follows in alpha mode
// (DESIGN.md 4.6).  Index output: the unchanged kernel with the identity palette into stream-ordered u32 scratch, then narrowed
// (k_narrow_index).
static hipError_t run_dither_masks(kmg_apply_plan *pl, const uint32_t *src, uint32_t w, uint32_t rows, uint32_t row0, void *d_out, hipStream_t st)
{
    kmg_processor *p = pl->p;
    const uint64_t n_px = (uint64_t)w * rows;
    const uint64_t *masks = (const uint64_t *)pl->aux;
    if (pl->format == KMG_FORMAT_RGBA8) {
        HIP_PASS(launch_dither_pruned(src, w, rows, row0, pl->d_cent, pl->k, p->d_lut, pl->d_pal, pl->thr, masks, (uint32_t *)d_out, st));
        return pl->alpha_cutoff ? launch_alpha_merge(src, (uint32_t *)d_out, n_px, st) : hipSuccess;
    }
    StreamBuf lab;                                                    // (freed in stream order when this returns)
    HIP_PASS(lab.alloc(p, sizeof(uint32_t) * n_px, st));
    HIP_PASS(launch_dither_pruned(src, w, rows, row0, pl->d_cent, pl->k, p->d_lut, pl->d_ident, pl->thr, masks, (uint32_t *)lab.ptr, st));
    return launch_narrow_index(src, (const uint32_t *)lab.ptr, n_px, pl->k, d_out, pl->format, st, pl->alpha_cutoff);
}

// One band by the plan's route.  RGBA8 in alpha mode: the source's alpha byte over the output's -- inside the kernel (its ALPHA
// instantiation), or by k_alpha_merge after the two routes whose kernels live in kmg_table.hip.  Index output
// (kmg_output_format INDEX8 / INDEX16): the index instantiations of the scan and list kernels and the label-table kernel of
// kmg_index.hip write the label directly.
static int run_band(kmg_apply_plan *pl, const uint32_t *src, uint32_t w, uint32_t rows, uint32_t row0, void *d_out, hipStream_t st)
{
    kmg_processor *p = pl->p;
    const uint64_t n_px = (uint64_t)w * rows;
    const uint32_t k = pl->k, cutoff = pl->alpha_cutoff;
    const bool index = pl->format != KMG_FORMAT_RGBA8, alpha = cutoff != 0;
    uint32_t *out = (uint32_t *)d_out;                                // (RGBA8)
    hipError_t e = hipSuccess;
    switch (pl->route) {
    case Route::kScan:
        e = launch_apply(src, w, rows, row0, pl->d_cent, k, p->d_lut, pl->d_pal, pl->dither, plan_offsets(pl), d_out, pl->format, st, cutoff);
        break;
    case Route::kReplaceTable:
        if (index) e = launch_labels_index(src, n_px, pl->aux, pl->sub, k, d_out, pl->format, st, cutoff);
        else if ((e = launch_labels(src, n_px, pl->aux, pl->sub, k, pl->d_pal, out, st)) == hipSuccess && alpha)
            e = launch_alpha_merge(src, out, n_px, st);
        break;
    case Route::kDitherLists:
        e = launch_dither_lists(src, w, rows, row0, pl->d_cent, k, p->d_lut, pl->d_pal, plan_offsets(pl), (const uint8_t *)pl->aux, d_out, pl->format, st, cutoff);
        break;
    case Route::kDitherMasks:
        e = run_dither_masks(pl, src, w, rows, row0, d_out, st);
        break;
    case Route::kMeldLists:
    case Route::kMeldMasks:
    case Route::kMeldScan:
        if (index) return fail(KMG_ERR_INVALID_ARGUMENT, "the plan's route has no index output");   // (meld: refused at create)
        e = pl->route == Route::kMeldLists ? launch_meld_lists(src, n_px, pl->d_cent, k, p->d_lut, (const uint8_t *)pl->aux, out, st, alpha)
                                           : launch_meld(src, n_px, pl->d_cent, k, p->d_lut, (const uint64_t *)pl->aux, out, st, alpha);
        break;
    case Route::kDiffuseTable:
    case Route::kDiffuseScan:
        e = run_diffuse(pl, src, w, rows, d_out, st);
        break;
    }
    return e == hipSuccess ? KMG_OK : fail_hip(e, "apply");
}

extern "C" int kmg_apply_plan_run(kmg_apply_plan *pl, const uint8_t *d_rgba, uint32_t w, uint32_t rows, uint32_t row0, uint8_t *d_out,
                                  void *stream)
try {
    if (!pl || !d_rgba || !d_out || !w || !rows) return fail(KMG_ERR_INVALID_ARGUMENT, "bad apply_plan_run arguments");
    // the output kernels keep the pixel index (and from it the Bayer coordinates) in 32 bits
    if ((uint64_t)w * rows > 0xFFFFFFFFull) return fail(KMG_ERR_UNSUPPORTED, "band has more than 2^32-1 pixels");
    if (pl->format == KMG_FORMAT_INDEX16 && (reinterpret_cast<uintptr_t>(d_out) & 1u))
        return fail(KMG_ERR_INVALID_ARGUMENT, "INDEX16 output must be 2-byte aligned");
    HIP_TRY(hipSetDevice(pl->p->device));
    const bool diffuse = pl->mode == KMG_MODE_DIFFUSE;
    if (diffuse) KMG_TRY(check_diffuse_band(pl, w, row0));
    // after the tables: diffusion always waits, the others only on another stream than the one that builds them
    if (diffuse || S(stream) != pl->built_on) HIP_TRY(hipStreamWaitEvent(S(stream), pl->ready, 0));
    return run_band(pl, (const uint32_t *)d_rgba, w, rows, row0, d_out, S(stream));
}
KMG_ABI_CATCH

// The plan's scratch block goes back to the processor: every stream that ran the plan must have been synchronised by the caller,
// or `synchronise` != 0 makes this call wait for the whole device first.
extern "C" void kmg_apply_plan_destroy(kmg_apply_plan *pl, int synchronise)
try {
    if (!pl) return;
    (void)hipSetDevice(pl->p->device);
    if (synchronise) (void)hipDeviceSynchronize();
    if (pl->ready) (void)hipEventDestroy(pl->ready);
    delete pl;                                                        // (~ArenaGuard returns the block)
}
KMG_ABI_CATCH_VOID

int kmg::dev_apply(kmg_processor *p, const uint8_t *d_rgba, uint32_t w, uint32_t rows, uint32_t row0, const float *c4, uint32_t k, int mode,
                   uint8_t *d_out, void *stream, uint32_t alpha_cutoff, int format, int filter, const DitherPtr *dither)
{
    if (!p || !d_rgba || !d_out || !c4 || !w || !rows || k == 0)
        return fail(KMG_ERR_INVALID_ARGUMENT, "bad apply arguments");
    if ((uint64_t)w * rows > 0xFFFFFFFFull) return fail(KMG_ERR_UNSUPPORTED, "band has more than 2^32-1 pixels");
    kmg_apply_plan *pl = nullptr;
    KMG_TRY(plan_create(p, c4, k, mode, (uint64_t)w * rows, stream, alpha_cutoff, &pl, format, filter, dither));
    // (diffusion: the band is an image of its own -- the plan is new, so its first run starts from a zero error row)
    int rc = kmg_apply_plan_run(pl, d_rgba, w, rows, mode == KMG_MODE_DIFFUSE ? 0u : row0, d_out, stream);
    const hipError_t e2 = hipStreamSynchronize(S(stream));            // the call returns when the band is written; the block is idle again
    if (rc == KMG_OK && e2 == hipSuccess) rc = diffuse_status(pl);
    kmg_apply_plan_destroy(pl, 0);
    if (rc != KMG_OK) return rc;
    return e2 == hipSuccess ? KMG_OK : fail_hip(e2, "apply");
}

extern "C" int kmg_dev_apply(kmg_processor *p, const uint8_t *d_rgba, uint32_t w, uint32_t rows, uint32_t row0,
                             const float *c4, uint32_t k, int mode, uint8_t *d_out, void *stream)
try {
    if (!p) return fail(KMG_ERR_INVALID_ARGUMENT, "bad apply arguments");
    return dev_apply(p, d_rgba, w, rows, row0, c4, k, mode, d_out, stream, p->alpha_cutoff.load(std::memory_order_relaxed));
}
KMG_ABI_CATCH

extern "C" int kmg_dev_apply_format(kmg_processor *p, const uint8_t *d_rgba, uint32_t w, uint32_t rows, uint32_t row0, const float *c4,
                                    uint32_t k, int mode, int format, void *d_out, void *stream)
try {
    if (!p) return fail(KMG_ERR_INVALID_ARGUMENT, "bad apply arguments");
    return dev_apply(p, d_rgba, w, rows, row0, c4, k, mode, (uint8_t *)d_out, stream, p->alpha_cutoff.load(std::memory_order_relaxed), format);
}
KMG_ABI_CATCH
