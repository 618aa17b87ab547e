// kmg_apply_route.h -- which route an apply plan takes (csrc/kmg_apply.hip): the cost models of the output passes and
// the one rule that reads them.  Host only, no device, no processor: plain C++ that a host test can include
// (tests/native/check_apply_route.cpp walks a table recorded from the rule as it stood inside plan_create).  `forced` is what a
// model's decision is overridden with (forced_strategy of kmg_state.h): +1 = colour table / candidate lists, -1 = per-pixel scan,
// 0 = the model decides; `mask_words` is KMG_STRATEGY_MASK_WORDS of the processor's strategy.
#pragma once

#include <stdint.h>

#include <cmath>

namespace kmg {

enum class Route { kScan, kMeldScan, kMeldMasks, kMeldLists, kReplaceTable, kDitherLists, kDitherMasks, kDiffuseTable, kDiffuseScan };

constexpr int kRouteModeDither = 1, kRouteModeMeld = 2, kRouteModeDiffuse = 3;   // kmg_reduce_mode of include/kmeans_hip.h
constexpr uint32_t kRouteListMaxK = 512;                                           // kLabListMaxK of kmg_table.h

// Same model for the replace-mode output pass (no histogram: every cell is labelled; scratch from the processor's
// blocks).
inline bool replace_table_pays(int forced, uint64_t n, uint32_t k)
{
    if (forced) return forced > 0;
    const double N = (double)n;
    const double brute = N * (8.1e-12 + 2.45e-13 * k);
    const double table = 9.0e-5 + 1.85e-7 * k + N * (k <= 256 ? 1.8e-12 + 2.0e-15 * k : 6.6e-12);
    return table < brute;
}

// Error-diffusion output pass (kmg_diffuse.hip): the colour table costs its build (the replace route's model above) and then a
// few LDS reads per step; the per-lane scan costs ~k key evaluations per step on the critical path, which for a W x H image is
// W + 2 (H - 1) steps -- about 3 sqrt(n) for the shapes of photographs (an estimate from the step counts; not fitted).
inline bool diffuse_table_pays(int forced, uint64_t n, uint32_t k)
{
    if (k < 2) return false;                                // one colour: nothing to look up
    if (forced) return forced > 0;
    const double steps = 3.0 * std::sqrt((double)n);
    const double table = 9.0e-5 + 1.85e-7 * k;
    return steps * 6.0e-9 * k > table;
}

// Dither output pass: per-pixel scan of all k centroids, or of the candidates of the pixel's cell only (k <= 256: byte lists per
// cell of a grid over Lab, kmg_lists.hip; above: mask words per (RGB cell, Bayer index)).  Measured on MI355X, noise images,
// random palettes (tools/dither_crossover.py -> profiles/r03_dither_crossover.txt): the scan costs 6.5 + 0.275 k ps per pixel,
// the list pass 6.8 + 0.02 k ps per pixel after ~45 us for the lists and their launch; with k >= 128 the scan's own latency
// (one wave walks all k) makes the lists win on any image.
inline bool dither_pruning_pays(int forced, uint64_t n, uint32_t k)
{
    if (forced) return forced > 0;
    if (k > kRouteListMaxK) return n >= 4000000ull;        // mask words: 0.55 ms of masks at k = 512
    if (k >= 128u) return n >= 16384ull;
    return (double)n * (0.255 * k - 0.3) > 45.0e6;          // ps saved per pixel x pixels > 45 us
}

// Meld output pass: ordered scan of all k centroids per pixel, or of the candidates of the pixel's colour
// cell only (k_meld_candidates: ~0.03 ms per 64 centroids; tools/dither_probe.py).
inline bool meld_pruning_pays(int forced, uint64_t n, uint32_t k)
{
    if (forced) return forced > 0;
    return k >= 16 && n >= (1ull << 20);
}

// Which pruned dither / meld pass?  k <= 512: byte lists per cell of a grid over Lab (kmg_lists.hip); larger k: mask words per (RGB
// cell, Bayer index) (kmg_table.hip).  KMG_STRATEGY_MASK_WORDS (kmg_options.strategy) sends every k to the mask words.
inline bool dither_takes_lists(bool mask_words, uint32_t k)
{
    return !mask_words && k <= kRouteListMaxK;
}

// The route of a plan for k centroids in `mode`, made for n_pixels_hint pixels: meld first; then the colour table, which replace
// mode and diffusion share (dither is replace when k = 1: mix_colors.wgsl:104-108); then the diffusion scan; then the pruned
// dither; else the scan of all centroids.
inline Route apply_route(int mode, uint32_t k, uint64_t n_pixels_hint, int forced, bool mask_words)
{
    const uint64_t n = n_pixels_hint;
    if (mode == kRouteModeMeld) {
        if (k < 2 || !meld_pruning_pays(forced, n, k)) return Route::kMeldScan;
        return dither_takes_lists(mask_words, k) ? Route::kMeldLists : Route::kMeldMasks;
    }
    const bool diffuse = mode == kRouteModeDiffuse, dither = mode == kRouteModeDither && k > 1;
    if (diffuse ? diffuse_table_pays(forced, n, k) : (!dither && replace_table_pays(forced, n, k)))
        return diffuse ? Route::kDiffuseTable : Route::kReplaceTable;
    if (diffuse) return Route::kDiffuseScan;
    if (dither && dither_pruning_pays(forced, n, k)) return dither_takes_lists(mask_words, k) ? Route::kDitherLists : Route::kDitherMasks;
    return Route::kScan;
}

// A plan whose dither choice is not the default (kmg_processor_set_dither[_custom]) never takes the mask words --
// their records are per (cell, index of the reference's 4 x 4 matrix) --: it scans instead, above k = 512 as under
// KMG_STRATEGY_MASK_WORDS.  The candidate lists are over Lab itself and serve any map.
inline Route apply_route_mapped(bool map_choice, int mode, uint32_t k, uint64_t n_pixels_hint, int forced, bool mask_words)
{
    const Route route = apply_route(mode, k, n_pixels_hint, forced, mask_words);
    return map_choice && route == Route::kDitherMasks ? Route::kScan : route;
}

// Which images of a batch join the batched output launch (kmg_batch_apply.hip): replace or dither, and the image's
// own plan would scan all centroids per pixel -- the batched launch then does the same work with one launch and no plan build.
// Every other image (meld, diffusion, a table, lists or mask-word route, a forced KMG_STRATEGY_TABLE) keeps its per-image pass.
// All routes write identical bytes: the rule changes time only.
// Widened by one case (profiles/r10_batch_apply_time.txt, the `pruned` rows): with 128 <= k <= 512 a plan takes the candidate
// lists from 16384 pixels on because ONE image's scan is bound by the latency of a wave that walks all k, not by throughput
// (dither_pruning_pays).  In a batched launch that latency is paid once for all images, so in a batch of two images or more such
// an image joins while the throughput model alone -- the line dither_pruning_pays applies below k = 128 -- says that the lists do
// not pay for it: at k = 256 the joined launch takes 0.23 - 0.37 of the images' own passes from 7 such images on; one such image
// alone takes 1.30 of its own pass and keeps it.
inline bool batch_apply_joins(int mode, uint32_t k, uint64_t n_pixels, int forced, bool mask_words, uint32_t n_images)
{
    if (mode == kRouteModeMeld || mode == kRouteModeDiffuse) return false;
    const Route route = apply_route(mode, k, n_pixels, forced, mask_words);
    if (route == Route::kScan) return true;
    if (n_images >= 2u && forced == 0 && (route == Route::kDitherLists || route == Route::kDitherMasks) && k >= 128u && k <= kRouteListMaxK)
        return !((double)n_pixels * (0.255 * k - 0.3) > 45.0e6);
    return false;
}

}  // namespace kmg
