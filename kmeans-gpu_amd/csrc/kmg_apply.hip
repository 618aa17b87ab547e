// kmg_apply.hip -- the output passes of the C ABI (find_colors / dither_colors / meld_colors, core/src/operations.rs:99-155,
// 215-271): kmg_apply_plan_*, kmg_dev_apply, their cost models and the exhaustive checks of their candidate masks / lists.

#include "kmg_state.h"

#include <cmath>

// Same model for the replace-mode output pass (no histogram: every cell is labelled; scratch from the processor's
// blocks).
static bool replace_table_pays(const kmg_processor *p, uint64_t n, uint32_t k)
{
    if (const int f = forced_strategy(p)) return f > 0;
    const double N = (double)n;
    const double brute = N * (8.1e-12 + 2.45e-13 * k);
    const double table = 9.0e-5 + 1.85e-7 * k + N * (k <= 256 ? 1.8e-12 + 2.0e-15 * k : 6.6e-12);
    return table < brute;
}

// Error-diffusion output pass (kmg_diffuse.hip): the colour table costs its build (the replace route's model above) and then a
// few LDS reads per step; the per-lane scan costs ~k key evaluations per step on the critical path, which for a W x H image is
// W + 2 (H - 1) steps -- about 3 sqrt(n) for the shapes of photographs (an estimate from the step counts; not fitted).
static bool diffuse_table_pays(const kmg_processor *p, uint64_t n, uint32_t k)
{
    if (k < 2) return false;                                // one colour: nothing to look up
    if (const int f = forced_strategy(p)) return f > 0;
    const double steps = 3.0 * std::sqrt((double)n);
    const double table = 9.0e-5 + 1.85e-7 * k;
    return steps * 6.0e-9 * k > table;
}

// Dither output pass: per-pixel scan of all k centroids, or of the candidates of the pixel's cell only (k <= 256: byte lists per
// cell of a grid over Lab, kmg_lists.hip; above: mask words per (RGB cell, Bayer index)).  Measured on MI355X, noise images,
// random palettes (tools/dither_crossover.py -> profiles/r03_dither_crossover.txt): the scan costs 6.5 + 0.275 k ps per pixel,
// the list pass 6.8 + 0.02 k ps per pixel after ~45 us for the lists and their launch; with k >= 128 the scan's own latency
// (one wave walks all k) makes the lists win on any image.
static bool dither_pruning_pays(const kmg_processor *p, uint64_t n, uint32_t k)
{
    if (const int f = forced_strategy(p)) return f > 0;
    if (k > kLabListMaxK) return n >= 4000000ull;          // mask words: 0.55 ms of masks at k = 512
    if (k >= 128u) return n >= 16384ull;
    return (double)n * (0.255 * k - 0.3) > 45.0e6;          // ps saved per pixel x pixels > 45 us
}

// Meld output pass: ordered scan of all k centroids per pixel, or of the candidates of the pixel's colour
// cell only (k_meld_candidates: ~0.03 ms per 64 centroids; tools/dither_probe.py).
static bool meld_pruning_pays(const kmg_processor *p, uint64_t n, uint32_t k)
{
    if (const int f = forced_strategy(p)) return f > 0;
    return k >= 16 && n >= (1ull << 20);
}

// test support: exhaustive validation of the dither candidate masks (kmg_table.hip) for a centroid
// table: over all 2^24 colours x 16 Bayer offsets, the arg-min over the candidates must equal the
// brute-force arg-min.  *violations must come back 0.
// Which pruned dither / meld pass?  k <= 512: byte lists per cell of a grid over Lab (kmg_lists.hip); larger k: mask words per (RGB
// cell, Bayer index) (kmg_table.hip).  KMG_STRATEGY_MASK_WORDS (kmg_options.strategy) sends every k to the mask words.
static bool dither_takes_lists(const kmg_processor *p, uint32_t k)
{
    return !(p->strategy.load(std::memory_order_relaxed) & KMG_STRATEGY_MASK_WORDS) && k <= kLabListMaxK;
}

extern "C" int kmg_debug_check_dither_masks(kmg_processor *p, const float *c4, uint32_t k, uint64_t *violations, void *stream)
try {
    if (!p || !c4 || !violations || k < 2 || k > KMG_MAX_K) return fail(KMG_ERR_INVALID_ARGUMENT, "bad check_dither_masks arguments");
    HIP_TRY(hipSetDevice(p->device));
    int rc;
    if ((rc = ensure_bounds(p, S(stream))) != KMG_OK) return rc;
    std::vector<Centroid> hc(k);
    for (uint32_t i = 0; i < k; ++i) {
        hc[i].L = c4[4 * i]; hc[i].a = c4[4 * i + 1]; hc[i].b = c4[4 * i + 2];
        hc[i].C = chroma(hc[i].a, hc[i].b);
    }
    const float thr = dither_threshold(c4, k);
    DevBuf cent, masks, viol;
    HIP_TRY(cent.alloc(sizeof(Centroid) * k));
    HIP_TRY(masks.alloc(sizeof(uint64_t) * (size_t)kCells * 16u * mask_words(k)));
    HIP_TRY(viol.alloc(sizeof(unsigned long long)));
    HIP_TRY(hipMemcpyAsync(cent.ptr, hc.data(), sizeof(Centroid) * k, hipMemcpyHostToDevice, S(stream)));
    HIP_TRY(hipMemsetAsync(viol.ptr, 0, sizeof(unsigned long long), S(stream)));
    HIP_TRY(launch_offset_candidates(p->d_bounds, (const Centroid *)cent.ptr, k, thr, (uint64_t *)masks.ptr, S(stream)));
    HIP_TRY(launch_check_offset_masks((const Centroid *)cent.ptr, k, (const uint64_t *)masks.ptr, p->d_lut, thr,
                                      (unsigned long long *)viol.ptr, S(stream)));
    if (k <= kLabListMaxK) {                                // the byte lists over Lab cells (kmg_lists.hip), same counter
        DevBuf lists;
        HIP_TRY(lists.alloc(lab_list_bytes(k)));
        HIP_TRY(launch_lab_candidates((const Centroid *)cent.ptr, k, thr, false, (uint8_t *)lists.ptr, S(stream)));
        HIP_TRY(launch_check_lab_lists((const Centroid *)cent.ptr, k, (const uint8_t *)lists.ptr, p->d_lut, thr,
                                       (unsigned long long *)viol.ptr, S(stream)));
        HIP_TRY(hipStreamSynchronize(S(stream)));
    }
    unsigned long long h = 0;
    HIP_TRY(hipMemcpyAsync(&h, viol.ptr, sizeof h, hipMemcpyDeviceToHost, S(stream)));
    HIP_TRY(hipStreamSynchronize(S(stream)));
    *violations = h;
    if (KMG_TOOLS_ENV("KMG_DITHER_STATS")) {
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
    std::vector<Centroid> hc(k);
    for (uint32_t i = 0; i < k; ++i) hc[i] = {c4[4 * i], c4[4 * i + 1], c4[4 * i + 2], chroma(c4[4 * i + 1], c4[4 * i + 2])};
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

// test support: exhaustive validation of the meld candidate masks for a centroid table (k >= 2): over all
// 2^24 colours the two closest centroids found among the cell's candidates must be those of the full scan.
extern "C" int kmg_debug_check_meld_masks(kmg_processor *p, const float *c4, uint32_t k, uint64_t *violations, void *stream)
try {
    if (!p || !c4 || !violations || k < 2 || k > KMG_MAX_K) return fail(KMG_ERR_INVALID_ARGUMENT, "bad check_meld_masks arguments");
    HIP_TRY(hipSetDevice(p->device));
    int rc;
    if ((rc = ensure_bounds(p, S(stream))) != KMG_OK) return rc;
    std::vector<Centroid> hc(k);
    for (uint32_t i = 0; i < k; ++i) {
        hc[i].L = c4[4 * i]; hc[i].a = c4[4 * i + 1]; hc[i].b = c4[4 * i + 2];
        hc[i].C = chroma(hc[i].a, hc[i].b);
    }
    DevBuf cent, masks, viol;
    HIP_TRY(cent.alloc(sizeof(Centroid) * k));
    HIP_TRY(masks.alloc(sizeof(uint64_t) * (size_t)kCells * mask_words(k)));
    HIP_TRY(viol.alloc(sizeof(unsigned long long)));
    HIP_TRY(hipMemcpyAsync(cent.ptr, hc.data(), sizeof(Centroid) * k, hipMemcpyHostToDevice, S(stream)));
    HIP_TRY(hipMemsetAsync(viol.ptr, 0, sizeof(unsigned long long), S(stream)));
    HIP_TRY(launch_meld_candidates(p->d_bounds, (const Centroid *)cent.ptr, k, (uint64_t *)masks.ptr, S(stream)));
    HIP_TRY(launch_check_meld_masks((const Centroid *)cent.ptr, k, (const uint64_t *)masks.ptr, p->d_lut,
                                    (unsigned long long *)viol.ptr, S(stream)));
    DevBuf lists;
    if (k <= kLabListMaxK) {                                // the byte lists over Lab cells (kmg_lists.hip), same counter
        HIP_TRY(lists.alloc(lab_list_bytes(k)));
        HIP_TRY(launch_lab_candidates((const Centroid *)cent.ptr, k, 0.0f, true, (uint8_t *)lists.ptr, S(stream)));
        HIP_TRY(launch_check_lab_lists_two((const Centroid *)cent.ptr, k, (const uint8_t *)lists.ptr, p->d_lut,
                                           (unsigned long long *)viol.ptr, S(stream)));
    }
    unsigned long long h = 0;
    HIP_TRY(hipMemcpyAsync(&h, viol.ptr, sizeof h, hipMemcpyDeviceToHost, S(stream)));
    HIP_TRY(hipStreamSynchronize(S(stream)));
    *violations = h;
    return KMG_OK;
}
KMG_ABI_CATCH

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
    bool dither = false;
    float thr = 0.0f;
    enum Route { kScan, kMeldScan, kMeldMasks, kMeldLists, kReplaceTable, kDitherLists, kDitherMasks, kDiffuseTable, kDiffuseScan } route = kScan;
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
    // dstate: 2 x width packed error rows, the sticky timeout word (zeroed once), the per-call control block (kmg_diffuse.hip);
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
static int check_index_format(const float *c4, uint32_t k, int mode, int format, uint32_t alpha_cutoff)
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

static int plan_create(kmg_processor *p, const float *c4, uint32_t k, int mode, uint64_t n_pixels_hint, void *stream,
                       uint32_t alpha_cutoff, kmg_apply_plan **out, int format = KMG_FORMAT_RGBA8)
{
    if (!p || !c4 || !out || k == 0) return fail(KMG_ERR_INVALID_ARGUMENT, "bad apply_plan arguments");
    *out = nullptr;
    KMG_TRY(check_k_limit(k));
    KMG_TRY(check_mode(mode));
    int rc0;
    if (format != KMG_FORMAT_RGBA8 && (rc0 = check_index_format(c4, k, mode, format, alpha_cutoff)) != KMG_OK) return rc0;
    HIP_TRY(hipSetDevice(p->device));
    kmg_apply_plan *pl = new (std::nothrow) kmg_apply_plan();
    if (!pl) return fail(KMG_ERR_OUT_OF_MEMORY, "host allocation failed");
    struct Undo { kmg_apply_plan *pl; ~Undo() { if (pl) { if (pl->ready) (void)hipEventDestroy(pl->ready); (void)hipStreamSynchronize(pl->built_on); delete pl; } } } undo{pl};
    pl->p = p; pl->k = k; pl->mode = mode; pl->format = format; pl->alpha_cutoff = alpha_cutoff; pl->built_on = S(stream);

    // per-centroid work on the host: (L,a,b,C) table, RGBA8 palette (lab_to_rgb.wgsl), threshold
    std::vector<Centroid> hc(k);
    std::vector<uint32_t> pal(k + 1);
    for (uint32_t i = 0; i < k; ++i) {
        hc[i].L = c4[4 * i]; hc[i].a = c4[4 * i + 1]; hc[i].b = c4[4 * i + 2];
        hc[i].C = chroma(hc[i].a, hc[i].b);
        uint8_t px[4];
        shader_lab_to_rgba8(c4 + 4 * i, px);
        memcpy(&pal[i], px, 4);
    }
    {
        const float sentinel[3] = {10000.0f, 10000.0f, 10000.0f};     // mix_colors.wgsl:73
        uint8_t px[4];
        shader_lab_to_rgba8(sentinel, px);
        memcpy(&pal[k], px, 4);
    }
    const bool dither = (mode == KMG_MODE_DITHER) && k > 1;           // mix_colors.wgsl:104-108
    const float thr = dither ? dither_threshold(c4, k) : 0.0f;
    pl->dither = dither; pl->thr = thr;

    // which route (by the number of pixels the plan is made for), and how much scratch it needs: one block per plan
    const uint64_t n_px = n_pixels_hint;
    const bool meld_masks_pay = mode == KMG_MODE_MELD && k >= 2 && meld_pruning_pays(p, n_px, k);
    const bool diffuse = mode == KMG_MODE_DIFFUSE;
    const bool replace_table = diffuse ? diffuse_table_pays(p, n_px, k) : (mode != KMG_MODE_MELD && !dither && replace_table_pays(p, n_px, k));
    const bool dither_pruned = mode != KMG_MODE_MELD && !diffuse && dither && dither_pruning_pays(p, n_px, k);
    const bool ident = format != KMG_FORMAT_RGBA8 && dither_pruned && !dither_takes_lists(p, k);   // index output of kDitherMasks
    const size_t tables_bytes = sizeof(Centroid) * k + sizeof(uint32_t) * (k + 1) * (ident ? 2u : 1u);
    const size_t sub_bytes = sizeof(uint16_t) * (kSubCells + kCells) + sizeof(uint32_t) * kCells;
    const size_t labels_bytes = (size_t)(k <= 256 ? 1 : 2) << 24;
    const size_t masks_bytes = sizeof(uint64_t) * (size_t)kCells * mask_words(k) * (dither_pruned ? 16u : 1u);
    size_t need = ArenaGuard::padded(tables_bytes);
    const bool dither_lists = dither_pruned && dither_takes_lists(p, k);      // byte lists over Lab cells instead of mask words
    const bool meld_lists = meld_masks_pay && dither_takes_lists(p, k);       // the same for the meld pass's two closest
    if ((meld_masks_pay && !meld_lists) || (dither_pruned && !dither_lists)) need += ArenaGuard::padded(masks_bytes);
    if (dither_lists || meld_lists) need += ArenaGuard::padded(lab_list_bytes(k));
    if (replace_table) need += ArenaGuard::padded(labels_bytes) + ArenaGuard::padded(sub_bytes) + ArenaGuard::padded(cube_masks_bytes(k)) +
                               ArenaGuard::padded(cube_work_bytes());
    ArenaGuard &arena = pl->arena;
    hipError_t e = arena.acquire(p, need);
    // centroid table and palette travel in one block (one copy)
    pl->staged.resize(tables_bytes);
    memcpy(pl->staged.data(), hc.data(), sizeof(Centroid) * k);
    memcpy(pl->staged.data() + sizeof(Centroid) * k, pal.data(), sizeof(uint32_t) * (k + 1));
    if (ident) {
        uint32_t *id = (uint32_t *)(pl->staged.data() + sizeof(Centroid) * k + sizeof(uint32_t) * (k + 1));
        for (uint32_t i = 0; i <= k; ++i) id[i] = i;
    }
    Centroid *d_cent = nullptr;
    if (e == hipSuccess) {
        d_cent = (Centroid *)arena.take(tables_bytes);
        pl->d_cent = d_cent;
        pl->d_pal = (uint32_t *)((uint8_t *)d_cent + sizeof(Centroid) * k);
        if (ident) pl->d_ident = pl->d_pal + (k + 1);
        e = hipMemcpyAsync(d_cent, pl->staged.data(), pl->staged.size(), hipMemcpyHostToDevice, S(stream));
    }
    int rc = KMG_OK;
    if (e != hipSuccess) {
        // fall through to the error report
    } else if (mode == KMG_MODE_MELD) {
        pl->route = kmg_apply_plan::kMeldScan;
        if (meld_lists) {
            uint8_t *lst = (uint8_t *)arena.take(lab_list_bytes(k));
            e = launch_lab_candidates(d_cent, k, 0.0f, true, lst, S(stream));
            pl->aux = lst; pl->route = kmg_apply_plan::kMeldLists;
        } else if (meld_masks_pay) {
            // large image: per colour cell, the centroids that can be one of a pixel's two closest
            if ((rc = ensure_bounds(p, S(stream))) == KMG_OK) {
                uint64_t *m = (uint64_t *)arena.take(masks_bytes);
                e = launch_meld_candidates(p->d_bounds, d_cent, k, m, S(stream));
                pl->aux = m; pl->route = kmg_apply_plan::kMeldMasks;
            }
        }
    } else if (replace_table) {
        // replace mode on a large image: the label of a pixel depends on its colour only, so label the
        // colour cube once (candidate masks + cube pass without sums) and emit pal[label] through the
        // label tables -- the same bit-exact machinery as the Lloyd label pass
        if ((rc = ensure_bounds(p, S(stream))) == KMG_OK) {
            void *colour_labels = arena.take(labels_bytes);
            uint16_t *sub = (uint16_t *)arena.take(sub_bytes);
            uint64_t *m = (uint64_t *)arena.take(cube_masks_bytes(k));
            void *cwork = arena.take(cube_work_bytes());
            e = launch_cube(nullptr, nullptr, nullptr, nullptr, nullptr, p->d_bounds, p->d_sub_bounds, d_cent, k, p->d_lab_table,
                            m, cwork, colour_labels, sub, nullptr, 0, 0u, nullptr, S(stream), nullptr, affine_for(p, k, S(stream)));
            pl->aux = colour_labels; pl->sub = sub; pl->route = diffuse ? kmg_apply_plan::kDiffuseTable : kmg_apply_plan::kReplaceTable;
        }
    } else if (diffuse) {
        pl->route = kmg_apply_plan::kDiffuseScan;
    } else if (dither_pruned) {
        // dither on a large image: candidate lists per cell of a grid over Lab (mask words per (colour cell, Bayer index)
        // above k = 512), then a scan of the pixel's candidates only
        if (dither_lists) {
            uint8_t *lst = (uint8_t *)arena.take(lab_list_bytes(k));
            e = launch_lab_candidates(d_cent, k, thr, false, lst, S(stream));
            pl->aux = lst; pl->route = kmg_apply_plan::kDitherLists;
        } else if ((rc = ensure_bounds(p, S(stream))) == KMG_OK) {
            uint64_t *m = (uint64_t *)arena.take(masks_bytes);
            e = launch_offset_candidates(p->d_bounds, d_cent, k, thr, m, S(stream));
            pl->aux = m; pl->route = kmg_apply_plan::kDitherMasks;
        }
    }
    if (rc != KMG_OK) return rc;
    if (e == hipSuccess && diffuse) e = hipEventCreateWithFlags(&pl->ddone, hipEventDisableTiming);
    if (e == hipSuccess && diffuse && (pl->h_slot = host_slot_take(p)) != nullptr) pl->h_timeout = static_cast<uint32_t *>(pl->h_slot);
    if (e == hipSuccess && diffuse) *pl->h_timeout = 0;
    if (e == hipSuccess) e = hipEventCreateWithFlags(&pl->ready, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventRecord(pl->ready, S(stream));
    if (e != hipSuccess) return fail_hip(e, "apply plan");
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
static int run_diffuse(kmg_apply_plan *pl, const uint8_t *d_rgba, uint32_t w, uint32_t rows, uint32_t row0, void *d_out, hipStream_t st)
{
    kmg_processor *p = pl->p;
    if (w > 0x7FFFFF00u) return fail(KMG_ERR_UNSUPPORTED, "diffusion needs a width below 2^31 - 256");
    if (row0 != pl->drows) return fail(KMG_ERR_INVALID_ARGUMENT, "diffusion band starts at row %u, the plan has done %u rows", row0, pl->drows);
    if (pl->drows && w != pl->dwidth) return fail(KMG_ERR_INVALID_ARGUMENT, "diffusion band has width %u, the image has %u", w, pl->dwidth);
    // an earlier band that timed out (the sticky word; known once a run after it has completed) fails every later run
    if (pl->drows && hipEventQuery(pl->ddone) == hipSuccess && *pl->h_timeout)
        return fail(KMG_ERR_HIP, "diffusion pass timed out");
    const size_t erow_bytes = sizeof(uint32_t) * 2 * 2 * (size_t)w;
    const size_t sticky_off = (erow_bytes + 255) & ~(size_t)255, ctl_off = sticky_off + 16;
    const size_t ctl_bytes = (diffuse_ctl_bytes() + 15) & ~(size_t)15;
    if (!pl->dstate) {
        HIP_TRY(pool_alloc(p, &pl->dstate, ctl_off + ctl_bytes, st));
        HIP_TRY(hipMemsetAsync((uint8_t *)pl->dstate + sticky_off, 0, 16, st));
    }
    uint8_t *erow = (uint8_t *)pl->dstate, *ctl = erow + ctl_off;
    uint32_t *sticky = (uint32_t *)(erow + sticky_off);
    HIP_TRY(hipStreamWaitEvent(st, pl->ready, 0));
    if (pl->drows) HIP_TRY(hipStreamWaitEvent(st, pl->ddone, 0));
    else HIP_TRY(hipMemsetAsync(erow + (size_t)pl->dparity * 8u * w, 0, 8u * (size_t)w, st));    // no row above the image
    HIP_TRY(hipMemsetAsync(ctl, 0, ctl_bytes, st));
    const bool table = pl->route == kmg_apply_plan::kDiffuseTable;
    const int route = !table ? kDiffuseScan : (pl->k <= 256 ? kDiffusePairs : kDiffuseCells);
    hipError_t e = launch_diffuse(route, (const uint32_t *)d_rgba, w, rows, d_out, erow, pl->dparity, ctl, sticky, pl->d_cent,
                                  pl->k, p->d_lut, pl->d_pal, pl->aux, pl->sub, st, pl->alpha_cutoff, pl->format);
    if (e == hipSuccess) e = hipMemcpyAsync((void *)pl->h_timeout, sticky, sizeof(uint32_t), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipEventRecord(pl->ddone, st);
    if (e != hipSuccess) return fail(KMG_ERR_HIP, "diffusion failed: %s", hipGetErrorString(e));
    pl->dwidth = w;
    pl->drows += rows;
    pl->dparity = (pl->dparity + (rows + 63u) / 64u) & 1u;
    return KMG_OK;
}

void kmg::apply_plan_restart(kmg_apply_plan *pl)
{
    if (pl) pl->drows = 0;
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

// Index output (kmg_output_format INDEX8 / INDEX16) of the routes other than diffusion: the index instantiations of the scan and
// list kernels and the label-table kernel of kmg_index.hip write the label directly; the mask-word dither route runs its
// unchanged kernel with the identity palette into stream-ordered u32 scratch, then narrows it (k_narrow_index).
static int run_index(kmg_apply_plan *pl, const uint8_t *d_rgba, uint32_t w, uint32_t rows, uint32_t row0, void *d_out, hipStream_t st)
{
    kmg_processor *p = pl->p;
    if (st != pl->built_on) HIP_TRY(hipStreamWaitEvent(st, pl->ready, 0));
    const uint64_t n_px = (uint64_t)w * rows;
    const uint32_t k = pl->k;
    const bool wide = pl->format == KMG_FORMAT_INDEX16;
    const uint32_t *src = (const uint32_t *)d_rgba;
    hipError_t e = hipSuccess;
    switch (pl->route) {
    case kmg_apply_plan::kReplaceTable:
        e = launch_labels_index(src, n_px, pl->aux, pl->sub, k, d_out, wide, st, pl->alpha_cutoff);
        break;
    case kmg_apply_plan::kDitherLists:
        e = launch_dither_lists_index(src, w, rows, row0, pl->d_cent, k, p->d_lut, pl->thr, (const uint8_t *)pl->aux, d_out, wide, st,
                                      pl->alpha_cutoff);
        break;
    case kmg_apply_plan::kDitherMasks: {
        void *lab = nullptr;
        HIP_TRY(pool_alloc(p, &lab, sizeof(uint32_t) * n_px, st));
        e = launch_dither_pruned(src, w, rows, row0, pl->d_cent, k, p->d_lut, pl->d_ident, pl->thr, (const uint64_t *)pl->aux, (uint32_t *)lab, st);
        if (e == hipSuccess) e = launch_narrow_index(src, (const uint32_t *)lab, n_px, k, d_out, wide, st, pl->alpha_cutoff);
        const hipError_t e2 = hipFreeAsync(lab, st);
        if (e == hipSuccess) e = e2;
        break;
    }
    case kmg_apply_plan::kScan:
        e = launch_apply_index(src, w, rows, row0, pl->d_cent, k, p->d_lut, pl->dither, pl->thr, d_out, wide, st, pl->alpha_cutoff);
        break;
    default:
        return fail(KMG_ERR_INVALID_ARGUMENT, "the plan's route has no index output");
    }
    if (e != hipSuccess) return fail(KMG_ERR_HIP, "apply failed: %s", hipGetErrorString(e));
    return KMG_OK;
}

extern "C" int kmg_apply_plan_run(kmg_apply_plan *pl, const uint8_t *d_rgba, uint32_t w, uint32_t rows, uint32_t row0, uint8_t *d_out,
                                  void *stream)
try {
    if (!pl || !d_rgba || !d_out || !w || !rows) return fail(KMG_ERR_INVALID_ARGUMENT, "bad apply_plan_run arguments");
    // the output kernels keep the pixel index (and from it the Bayer coordinates) in 32 bits
    if ((uint64_t)w * rows > 0xFFFFFFFFull) return fail(KMG_ERR_UNSUPPORTED, "band has more than 2^32-1 pixels");
    if (pl->format == KMG_FORMAT_INDEX16 && (reinterpret_cast<uintptr_t>(d_out) & 1u))
        return fail(KMG_ERR_INVALID_ARGUMENT, "INDEX16 output must be 2-byte aligned");
    kmg_processor *p = pl->p;
    HIP_TRY(hipSetDevice(p->device));
    if (pl->mode == KMG_MODE_DIFFUSE) return run_diffuse(pl, d_rgba, w, rows, row0, d_out, S(stream));
    if (pl->format != KMG_FORMAT_RGBA8) return run_index(pl, d_rgba, w, rows, row0, d_out, S(stream));
    if (S(stream) != pl->built_on) HIP_TRY(hipStreamWaitEvent(S(stream), pl->ready, 0));      // (another stream: after the tables)
    const uint64_t n_px = (uint64_t)w * rows;
    const uint32_t k = pl->k;
    // alpha mode: the source's alpha byte over the output's -- inside the kernel (its ALPHA instantiation), or by k_alpha_merge after
    // the two routes whose kernels live in kmg_table.hip
    const bool alpha = pl->alpha_cutoff != 0;
    hipError_t e = hipSuccess;
    switch (pl->route) {
    case kmg_apply_plan::kMeldLists:
        e = launch_meld_lists((const uint32_t *)d_rgba, n_px, pl->d_cent, k, p->d_lut, (const uint8_t *)pl->aux, (uint32_t *)d_out, S(stream),
                              alpha);
        break;
    case kmg_apply_plan::kMeldMasks:
    case kmg_apply_plan::kMeldScan:
        e = launch_meld((const uint32_t *)d_rgba, n_px, pl->d_cent, k, p->d_lut, (const uint64_t *)pl->aux, (uint32_t *)d_out, S(stream),
                        alpha);
        break;
    case kmg_apply_plan::kReplaceTable:
        e = launch_labels((const uint32_t *)d_rgba, n_px, pl->aux, pl->sub, k, pl->d_pal, (uint32_t *)d_out, S(stream));
        if (e == hipSuccess && alpha) e = launch_alpha_merge((const uint32_t *)d_rgba, (uint32_t *)d_out, n_px, S(stream));
        break;
    case kmg_apply_plan::kDitherLists:
        e = launch_dither_lists((const uint32_t *)d_rgba, w, rows, row0, pl->d_cent, k, p->d_lut, pl->d_pal, pl->thr, (const uint8_t *)pl->aux,
                                (uint32_t *)d_out, S(stream), alpha);
        break;
    case kmg_apply_plan::kDitherMasks:
        e = launch_dither_pruned((const uint32_t *)d_rgba, w, rows, row0, pl->d_cent, k, p->d_lut, pl->d_pal, pl->thr, (const uint64_t *)pl->aux,
                                 (uint32_t *)d_out, S(stream));
        if (e == hipSuccess && alpha) e = launch_alpha_merge((const uint32_t *)d_rgba, (uint32_t *)d_out, n_px, S(stream));
        break;
    default:
        e = launch_apply((const uint32_t *)d_rgba, w, rows, row0, pl->d_cent, k, p->d_lut, pl->d_pal, pl->dither, pl->thr, (uint32_t *)d_out,
                         S(stream), alpha);
    }
    if (e != hipSuccess) return fail(KMG_ERR_HIP, "apply failed: %s", hipGetErrorString(e));
    return KMG_OK;
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
                   uint8_t *d_out, void *stream, uint32_t alpha_cutoff, int format)
{
    if (!p || !d_rgba || !d_out || !c4 || !w || !rows || k == 0)
        return fail(KMG_ERR_INVALID_ARGUMENT, "bad apply arguments");
    if ((uint64_t)w * rows > 0xFFFFFFFFull) return fail(KMG_ERR_UNSUPPORTED, "band has more than 2^32-1 pixels");
    kmg_apply_plan *pl = nullptr;
    int rc = plan_create(p, c4, k, mode, (uint64_t)w * rows, stream, alpha_cutoff, &pl, format);
    if (rc != KMG_OK) return rc;
    // (diffusion: the band is an image of its own -- the plan is new, so its first run starts from a zero error row)
    rc = kmg_apply_plan_run(pl, d_rgba, w, rows, mode == KMG_MODE_DIFFUSE ? 0u : row0, d_out, stream);
    const hipError_t e2 = hipStreamSynchronize(S(stream));            // the call returns when the band is written; the block is idle again
    if (rc == KMG_OK && e2 == hipSuccess) rc = diffuse_status(pl);
    kmg_apply_plan_destroy(pl, 0);
    if (rc != KMG_OK) return rc;
    if (e2 != hipSuccess) return fail(KMG_ERR_HIP, "apply failed: %s", hipGetErrorString(e2));
    return KMG_OK;
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
