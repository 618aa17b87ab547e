// kmg_checks.h -- the argument checks that the entry points of the C ABI share (host only).  Each refusal's condition and message
// stand here once; an entry point calls the checks it needs in the order it refuses.  Every check returns KMG_OK or the status
// of fail().  (kmg_usage.hip keeps its own checks: their messages carry the call's name.)
#pragma once

#include "kmg_internal.h"

namespace kmg {

static inline int check_pixel_count(uint64_t n)
{
    if (n > 0xFFFFFFFFull) return fail(KMG_ERR_UNSUPPORTED, "image has more than 2^32-1 pixels");
    return KMG_OK;
}

static inline int check_image_size(uint32_t w, uint32_t h)
{
    if (w == 0 || h == 0) return fail(KMG_ERR_INVALID_ARGUMENT, "image has zero width or height");
    return check_pixel_count((uint64_t)w * h);
}

// the image triple: pointer, zero side, 2^32-1 pixels -- the first thing a call does with an image
static inline int check_image_buffer(const void *rgba, uint32_t w, uint32_t h)
{
    if (!rgba) return fail(KMG_ERR_INVALID_ARGUMENT, "image pointer is NULL");
    return check_image_size(w, h);
}

// The refusals every batch call starts with, in the order that is part of the contract (include/kmeans_hip.h at kmg_batch_report):
// processor, empty batch, the call's arrays (array_null: one of them is NULL; array_message: how the call words that), then image by
// image a NULL image, a NULL entry of a per-image output array (out_a, out_b: NULL = the call has none), a zero side, 2^32-1 pixels.
template <typename Image, typename OutA = void, typename OutB = void>
static inline int check_batch_prefix(const void *p, uint32_t n_images, bool array_null, const char *array_message, Image *const *images,
                                     const uint32_t *widths, const uint32_t *heights, OutA *const *out_a = nullptr, OutB *const *out_b = nullptr)
{
    if (!p) return fail(KMG_ERR_INVALID_ARGUMENT, "processor is NULL");
    if (n_images == 0) return fail(KMG_ERR_INVALID_ARGUMENT, "the batch is empty");
    if (array_null) return fail(KMG_ERR_INVALID_ARGUMENT, "%s", array_message);
    for (uint32_t i = 0; i < n_images; ++i) {
        if (!images[i]) return fail(KMG_ERR_INVALID_ARGUMENT, "image %u: image pointer is NULL", i);
        if ((out_a && !out_a[i]) || (out_b && !out_b[i])) return fail(KMG_ERR_INVALID_ARGUMENT, "image %u: output pointer is NULL", i);
        if (!widths[i] || !heights[i]) return fail(KMG_ERR_INVALID_ARGUMENT, "image %u has zero width or height", i);
        KMG_TRY(check_pixel_count((uint64_t)widths[i] * heights[i]));
    }
    return KMG_OK;
}

// the colour count (args.rs:160-171), its two halves for the calls that refuse something else in between
static inline int check_k_nonzero(uint32_t k)
{
    if (k == 0) return fail(KMG_ERR_INVALID_ARGUMENT, "k must be an integer higher than 0");
    return KMG_OK;
}

static inline int check_k_limit(uint32_t k)
{
    if (k > KMG_MAX_K) return fail(KMG_ERR_UNSUPPORTED, "k = %u exceeds KMG_MAX_K = %u", k, KMG_MAX_K);
    return KMG_OK;
}

static inline int check_k(uint32_t k)
{
    const int rc = check_k_nonzero(k);
    return rc != KMG_OK ? rc : check_k_limit(k);
}

static inline int check_algo(int algo)
{
    if (algo != KMG_ALGO_KMEANS && algo != KMG_ALGO_OCTREE) return fail(KMG_ERR_INVALID_ARGUMENT, "unknown algorithm %d", algo);
    return KMG_OK;
}

// last: KMG_MODE_DIFFUSE, or KMG_MODE_MELD for the group calls, which have no diffusion
static inline int check_mode(int mode, int last = KMG_MODE_DIFFUSE)
{
    if (mode < KMG_MODE_REPLACE || mode > last) return fail(KMG_ERR_INVALID_ARGUMENT, "unknown mode %d", mode);
    return KMG_OK;
}

// (a call that takes index formats only refuses KMG_FORMAT_RGBA8 with a sentence of its own first)
static inline int check_format(int format)
{
    if (format < KMG_FORMAT_RGBA8 || format > KMG_FORMAT_INDEX16) return fail(KMG_ERR_INVALID_ARGUMENT, "unknown output format %d", format);
    return KMG_OK;
}

static inline int check_meld_format(int mode, int format)
{
    if (format != KMG_FORMAT_RGBA8 && mode == KMG_MODE_MELD)
        return fail(KMG_ERR_INVALID_ARGUMENT, "meld blends two colours: it has no index output");
    return KMG_OK;
}

// index8 (the output is KMG_FORMAT_INDEX8): it holds k colours, and the transparent slot where the call has one.  label: what the
// call names its count (k, k_max)
static inline int check_index8_room(bool index8, const char *label, uint32_t k, bool transparent_slot)
{
    if (index8 && k + (transparent_slot ? 1u : 0u) > 256u)
        return fail(KMG_ERR_INVALID_ARGUMENT, "INDEX8 holds 256 indices; %s = %u%s needs INDEX16", label, k,
                    transparent_slot ? " plus the transparent slot" : "");
    return KMG_OK;
}

}  // namespace kmg
