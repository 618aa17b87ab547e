/*
 * kmeans_hip.h -- C ABI of libkmeans_hip.so: the MI355X (gfx950) implementation of the
 * Lloyd-iteration hot path of redwarp/kmeans-gpu (per-pixel CIE94 assignment, per-cluster
 * sum/count reduction + centroid update, ordered-dither / replace output pass).
 *
 * Every entry point names the reference interface it replaces (paths relative to the
 * reference repository).  The high-level calls take HOST buffers exactly like the reference
 * crate's `ImageProcessor` (core/src/lib.rs:24-165); the `kmg_dev_*` / `kmg_lloyd_*` calls take
 * DEVICE pointers and an explicit hipStream_t so a host runtime (one process per GPU) can
 * shard an image, run the exchange step of the update itself (RCCL all-reduce of the k
 * accumulators) and keep everything resident in HBM.
 *
 * Conventions
 *  - images: tightly packed row-major RGBA8, 4 bytes per pixel, no row padding
 *    (core/src/image.rs:20-48); alpha is ignored on input and 255 on output, unless
 *    kmg_options.alpha_cutoff turns on alpha mode (see there).
 *  - centroid tables: k x 4 floats (L, a, b, 1.0) -- the `vec4<f32>` array of the reference's
 *    CentroidsBuffer (core/src/structures.rs:501-521) without its 16-byte count header.
 *  - accumulators: k x 4 int64 = (sum qL, sum qa, sum qb, count), q = rint(Lab * 2^20).
 *    Integer sums are order independent, so results are identical for any tiling or GPU count.
 *  - all functions return KMG_OK (0) or a negative kmg_status; kmg_last_error() gives the
 *    thread-local message of the last failure.
 *  - every entry point is re-entrant on one kmg_processor (per-call workspace + stream), like
 *    the reference's Send+Sync ImageProcessor (core/examples/parallel.rs:36-50).
 *  - there is NO CPU fallback: without a usable HIP device kmg_processor_create fails.
 *  - no C++ exception leaves the library (every entry point is a function-try-block): host allocation failures come back
 *    as KMG_ERR_OUT_OF_MEMORY, any other internal exception as KMG_ERR_HIP -- the reference's anyhow::Result (lib.rs:38).
 */
#ifndef KMEANS_HIP_H
#define KMEANS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KMG_API __attribute__((visibility("default")))

typedef enum kmg_status {
    KMG_OK = 0,
    KMG_ERR_INVALID_ARGUMENT = -1, /* null pointer, zero-sized image, color_count == 0 ... */
    KMG_ERR_NO_DEVICE = -2,        /* no HIP device / device init failed                    */
    KMG_ERR_HIP = -3,              /* a HIP runtime call failed (message has the detail)    */
    KMG_ERR_OUT_OF_MEMORY = -4,
    KMG_ERR_UNSUPPORTED = -5       /* e.g. k > KMG_MAX_K, more than 2^32-1 pixels            */
} kmg_status;

/* core/src/lib.rs:215-219 `enum Algorithm` */
typedef enum kmg_algorithm { KMG_ALGO_KMEANS = 0, KMG_ALGO_OCTREE = 1 } kmg_algorithm;
/* core/src/lib.rs:234-239 `enum ReduceMode`, and one mode of this library's own:
 *
 * KMG_MODE_DIFFUSE -- Floyd-Steinberg error diffusion onto the palette.  Pixels are visited in raster order (rows top to
 * bottom, each row left to right; no serpentine).  For each pixel (x, y) and each channel ch in {R, G, B}, in int32:
 *   S   = 7 e(x-1, y) + 3 e(x+1, y-1) + 5 e(x, y-1) + 1 e(x-1, y-1)     (a neighbour outside the image contributes 0)
 *   v   = 16 src(x, y) + floor((S + 8) / 16)                             (units of 1/16 LSB; floor = arithmetic >> 4)
 *   t   = clamp(v, 0, 4080)
 *   c   = (t + 8) >> 4                                                   (0 .. 255)
 *   lbl = the label KMG_MODE_REPLACE gives an opaque pixel of colour (c_R, c_G, c_B)
 *   o   = the bytes KMG_MODE_REPLACE writes for lbl
 *   out(x, y) = (o_R, o_G, o_B, 255)
 *   e(x, y)   = t - 16 o                                                 (|e| <= 4080, so |S| <= 65 280)
 * Input alpha is ignored (alpha mode: see kmg_options.alpha_cutoff).  kmg_dev_apply diffuses the given rows as an image of their own (zero error above the band);
 * kmg_apply_plan_run continues the diffusion across consecutive bands (row0 = the rows done so far, 0 first; the width
 * unchanged; anything else is KMG_ERR_INVALID_ARGUMENT), each band after the previous one whatever its stream.  A pass in
 * which nothing moves for about half a second gives up and is reported as KMG_ERR_HIP ("diffusion pass timed out"): by
 * kmg_dev_apply, by later runs of the plan, and by kmg_apply_plan_status.
 * The kmg_group_* calls reject this mode (KMG_ERR_INVALID_ARGUMENT): diffusion across row-band ranks is serial by nature. */
typedef enum kmg_reduce_mode {
    KMG_MODE_REPLACE = 0,
    KMG_MODE_DITHER = 1,
    KMG_MODE_MELD = 2,
    KMG_MODE_DIFFUSE = 3
} kmg_reduce_mode;

/* The filter of KMG_MODE_DIFFUSE (kmg_processor_set_diffusion; the other modes ignore it).  A filter is a divisor D and weights
 * W[dy][dx]: W[dy][dx] / D is the share of pixel (x, y)'s error that goes to (x + dx, y + dy).  Row 0 has dx = +1, +2, rows 1 and
 * 2 have dx = -2 .. +2; absent entries are 0.  The contract is the one above with its first two lines generalised:
 *   S   = sum over dy, dx of W[dy][dx] e(x - dx, y - dy)                 (a neighbour outside the image contributes 0)
 *   v   = 16 src(x, y) + floor((S + D/2) / D)                            (mathematical floor, S may be negative; every D is even)
 *   t, c, lbl, o, out, e: as above                                       (|e| <= 4080, |S| <= 4080 D <= 195 840: int32)
 * For D = 16 the v line is (S + 8) >> 4: filter 0 is the contract above word for word.  Alpha mode, the index formats, the bands
 * of a plan and kmg_dev_apply on a band behave as for Floyd-Steinberg.
 *                                    D    row 0 (dx +1, +2)   row 1 (dx -2 .. +2)   row 2 (dx -2 .. +2)
 *   KMG_DIFFUSION_FLOYD_STEINBERG   16    7, 0                0, 3, 5, 1, 0         -
 *   KMG_DIFFUSION_SIERRA_LITE        4    2, 0                0, 1, 1, 0, 0         -
 *   KMG_DIFFUSION_ATKINSON           8    1, 1                0, 1, 1, 1, 0         0, 0, 1, 0, 0     (passes on 6/8 of the error)
 *   KMG_DIFFUSION_BURKES            32    8, 4                2, 4, 8, 4, 2         -
 *   KMG_DIFFUSION_SIERRA2           16    4, 3                1, 2, 3, 2, 1         -
 *   KMG_DIFFUSION_SIERRA3           32    5, 3                2, 4, 5, 4, 2         0, 2, 3, 2, 0
 *   KMG_DIFFUSION_JARVIS            48    7, 5                3, 5, 7, 5, 3         1, 3, 5, 3, 1
 *   KMG_DIFFUSION_STUCKI            42    8, 4                2, 4, 8, 4, 2         1, 2, 4, 2, 1
 * kmg_diffusion_weights returns this table. */
typedef enum kmg_diffusion {
    KMG_DIFFUSION_FLOYD_STEINBERG = 0,
    KMG_DIFFUSION_SIERRA_LITE = 1,
    KMG_DIFFUSION_ATKINSON = 2,
    KMG_DIFFUSION_BURKES = 3,
    KMG_DIFFUSION_SIERRA2 = 4,
    KMG_DIFFUSION_SIERRA3 = 5,
    KMG_DIFFUSION_JARVIS = 6,
    KMG_DIFFUSION_STUCKI = 7,
    KMG_DIFFUSION_COUNT = 8
} kmg_diffusion;

/* The threshold map and the strength of KMG_MODE_DITHER (kmg_processor_set_dither[_custom]; the other modes ignore them).  A map is
 * mw x mh levels l(x, y), each a uint16_t below n_levels; mw and mh are powers of two in 1 .. 64, independent of each other, and
 * 1 <= n_levels <= 65536.  For the image pixel (x, y) -- y the image row, so a band starting at row0 reads row row0 + its own --
 *   v   = (float)l(x mod mw, y mod mh) / (float)n_levels - 0.5f     (on the host, once per map, IEEE fp32: one correctly rounded
 *                                                                     division, then one subtraction)
 *   t   = threshold * strength                                       (threshold = palette diameter / sqrt(k) as before; fp32, one
 *                                                                     rounding)
 *   off = t * v                                                      (fp32, no contraction)
 *   adjusted = (L + off, a + off, b + off)
 * and then mix_colors.wgsl:73-80 as before: the scan starts at the sentinel (10000, 10000, 10000), whose index is k, and k = 1
 * behaves as KMG_MODE_REPLACE.  With the reference's matrix, n_levels = 16 and strength 1.0f this is the reference's arithmetic
 * operation for operation (threshold * 1.0f is exact, M / 16 - 0.5 is what it computes): KMG_DITHER_BAYER4 at strength 1, the
 * default, writes the bytes this library wrote before it had maps.
 *   KMG_DITHER_BAYER4    the reference's 4 x 4 matrix (mix_colors.wgsl:14-17), n_levels = 16
 *   KMG_DITHER_BAYER2 / BAYER8 / BAYER16   the Bayer recursion M2 = [[0, 2], [3, 1]], M2n = [[4M, 4M + 2], [4M + 3, 4M + 1]]
 *                        (which also gives the reference's matrix), n_levels = side^2
 *   KMG_DITHER_BLUE64    a 64 x 64 void-and-cluster (blue-noise) map, a permutation of 0 .. 4095, n_levels = 4096
 *   KMG_DITHER_CUSTOM    the caller's own map (kmg_processor_set_dither_custom)
 * kmg_dither_map_values returns the table of a built-in map.  strength is finite and in [0, 4].
 * The kmg_group_* calls in KMG_MODE_DITHER refuse a member processor whose choice is not the default (KMG_ERR_INVALID_ARGUMENT),
 * as they refuse alpha weighting. */
typedef enum kmg_dither_map {
    KMG_DITHER_BAYER4 = 0,
    KMG_DITHER_BAYER2 = 1,
    KMG_DITHER_BAYER8 = 2,
    KMG_DITHER_BAYER16 = 3,
    KMG_DITHER_BLUE64 = 4,
    KMG_DITHER_CUSTOM = 5,
    KMG_DITHER_COUNT = 6
} kmg_dither_map;

/* Output format of the output passes (kmg_apply_plan_create_format, kmg_dev_apply_format, kmg_find_indexed, kmg_reduce_indexed).
 * KMG_FORMAT_RGBA8 is the RGBA8 image every other call writes: the same bytes.  The index formats write one uint8_t / uint16_t
 * per pixel, tightly packed, row-major: the label i the mode picks for the pixel -- the very label whose palette bytes the RGBA8
 * call of the same arguments writes, so out_rgba8 = (P[i].rgb, a) with P = the palette of the output pass (lab_to_rgb.wgsl of
 * centroid i; kmg_reduce_indexed returns it; kmg_centroids_to_palette converts with the palette crate instead and can differ
 * from it by one LSB where a channel rounds at .5).  For kmg_find_indexed, i is entry i of the caller's palette; the RGBA8
 * output holds its re-encoded bytes (kmg_palette_to_centroids, then lab_to_rgb.wgsl).
 *  - Modes: replace, dither and diffuse, each with its per-pixel decision unchanged bit for bit (the Bayer coordinates from
 *    row0, the diffusion carried across the bands of a plan).  KMG_MODE_MELD blends two colours and has no index:
 *    KMG_ERR_INVALID_ARGUMENT.
 *  - Every index is < k.  The dither scan starts from the reference's sentinel (label k, mix_colors.wgsl:73); it cannot win for
 *    an sRGB8 pixel when every centroid lies in the box L in [-100, 200], a, b in [-300, 300], so the index
 *    formats refuse (KMG_ERR_INVALID_ARGUMENT) a table with a non-finite component or one outside that box.  Every table
 *    kmg_palette, kmg_palette_to_centroids or kmg_reduce produces lies inside it.  (KMG_FORMAT_RGBA8 accepts any table, as before.)
 *  - Alpha mode (kmg_options.alpha_cutoff = t > 0): a pixel with alpha < t is written as index k, the transparent slot; kept
 *    pixels get their normal index (their partial alpha is not represented).  Diffusion: unchanged, excluded pixels pass no
 *    error on.
 *  - Limits: KMG_FORMAT_INDEX8 needs k <= 256 (k <= 255 in alpha mode), KMG_FORMAT_INDEX16 takes any k <= KMG_MAX_K; device
 *    outputs of KMG_FORMAT_INDEX16 are 2-byte aligned.  Otherwise KMG_ERR_INVALID_ARGUMENT.  The kmg_group_* calls have no
 *    index output. */
typedef enum kmg_output_format { KMG_FORMAT_RGBA8 = 0, KMG_FORMAT_INDEX8 = 1, KMG_FORMAT_INDEX16 = 2 } kmg_output_format;

#define KMG_FIX_SHIFT 20
/* largest k: the kernels keep 48 bytes of LDS per cluster (centroid + int64 sums), 160 KiB per CU */
#define KMG_MAX_K 3072u

/* Compile-time constants of the reference exposed as options (defaults = reference values). */
typedef struct kmg_options {
    uint32_t struct_size;     /* sizeof(kmg_options)                                           */
    int32_t  device;          /* HIP device ordinal, -1 = current device                       */
    uint32_t shrink_max_dim;  /* MAX_IMAGE_DIMENSION = 256 (core/src/structures.rs:23); 0 = off */
    uint32_t max_iterations;  /* MAX_ITERATION = 128 (core/src/modules.rs:765)                  */
    uint32_t check_period;    /* MAX_ITERATION_BEFORE_CONVERGENCE_CHECK = 8 (modules.rs:766)    */
    float    convergence;     /* ColorSpace::Lab.convergence() = 1.0 (core/src/lib.rs:189-194)  */
    int32_t  strategy;        /* KMG_STRATEGY_*: 0 = the library's cost models pick per call (default)                     */
    uint32_t alpha_cutoff;    /* 0 = alpha ignored (default); 1..255 = alpha mode, see below                                   */
} kmg_options;

/* kmg_options.alpha_cutoff / kmg_processor_set_alpha_cutoff -- alpha-aware quantisation.  0 keeps the behaviour described
 * everywhere else in this header, bit for bit; a value above 255 is KMG_ERR_INVALID_ARGUMENT.  t = 1..255 turns alpha mode on:
 * a pixel is KEPT if and only if its alpha byte is >= t (t = 1 drops the fully transparent pixels only).
 *  - Palette (kmg_palette, the palette step of kmg_reduce), KMG_ALGO_KMEANS.  S = the image after the shrink (unchanged: it
 *    filters alpha with the same bilinear weights as RGB, so colour of transparent neighbours bleeds into edge pixels -- there
 *    is no premultiplied shrink), K = the kept pixels of S in raster order, n_kept = |K|.  n_kept = |S|: the default call, byte
 *    for byte.  n_kept = 0: KMG_ERR_INVALID_ARGUMENT ("no pixel reaches alpha_cutoff"), nothing written.  Otherwise the
 *    centroids are those the default pipeline (initialisation + Lloyd loop, max_iterations / check_period / convergence) gives
 *    for an image of n_kept x 1 pixels made of K: c_0 = K[floor(n_kept * 0.5625f)], the farthest-point tie rule runs over K's
 *    indices, the sums run over K only.  Every kept pixel weighs 1, whatever its alpha (kmg_processor_set_weighting changes that).
 *  - Palette, KMG_ALGO_OCTREE: the octree receives the kept pixels of its <= 128 shrink, in raster order.  All kept: the
 *    default call; none kept: the error above.
 *  - Output (kmg_find, kmg_reduce, kmg_dev_apply, apply plans), all four modes: out.rgb = what the mode writes for the pixel
 *    without alpha mode, out.a = the input's alpha byte -- for excluded pixels too (their RGB is invisible anyway).  Exception,
 *    KMG_MODE_DIFFUSE: a pixel that is not kept takes no part in the diffusion -- its out.rgb is the replace bytes of its own
 *    unmodified colour and e(x, y) = 0 (it passes no error on; the error that would reach it is dropped).  Kept pixels use the
 *    formulas of KMG_MODE_DIFFUSE unchanged (excluded neighbours contribute 0); bands of an apply plan continue as without it.
 *  - Palette entries keep alpha 255.  The kmg_lloyd_* calls count every pixel they are given (callers compact first:
 *    kmg_dev_alpha_compact); kmg_group_create refuses alpha_cutoff != 0 (KMG_ERR_INVALID_ARGUMENT).
 * (Options structs of the two previous sizes -- without this field, and without `strategy` -- are accepted and mean 0.)        */

/* kmg_processor_set_weighting -- alpha-weighted k-means: a pixel shapes the palette by how much of it is seen.  No counterpart in the
 * reference.  KMG_WEIGHT_NONE, the default, keeps the behaviour described everywhere else in this header, byte for byte;
 * KMG_WEIGHT_ALPHA turns weighting on; any other value is KMG_ERR_INVALID_ARGUMENT.  The setter is sticky, like
 * kmg_processor_set_fixed_colors (kmg_options has no field for it); calls that are already running keep the value they started
 * with.  With KMG_WEIGHT_ALPHA on a processor whose alpha_cutoff is t:
 *  - Weight.  The weight of a pixel of the working image is its alpha byte a, 0 .. 255 -- the alpha after the shrink, which filters
 *    alpha with the bilinear weights of RGB.  (An importance map for an opaque image is therefore an alpha channel, at t = 0.)
 *  - Kept pixels.  A pixel is kept iff a >= max(t, 1).  The working image W is alpha mode's compaction at that cutoff (the whole
 *    pixel is copied, alpha included); when every pixel is kept the image itself is W; when none is, the KMG_ERR_INVALID_ARGUMENT
 *    of alpha mode comes back.
 *  - Initialisation: unweighted and unchanged -- the farthest-point loop over the kept pixels, the fixed colours first when set,
 *    exactly what alpha mode at cutoff max(t, 1) runs.
 *  - Lloyd loop: the accumulators are (sum a qL, sum a qa, sum a qb, sum a) instead of (sum qL, sum qa, sum qb, count) --
 *    equivalently, the default loop on the pixel list in which pixel i appears a_i times.  Update, convergence count,
 *    check_period, max_iterations and the fixed colours are unchanged and read those sums; a cluster whose members all weigh 0 is
 *    an empty cluster.  Labels do not depend on the weights.  Integer sums: every route returns identical bits, as ever.
 *  - NO identity with the unweighted result is promised, not even for uniform weights: (double)(255 S) / (double)(255 n) can
 *    round differently from (double)S / (double)n once a sum passes 2^53.
 *  - Outputs (kmg_find, the output step of kmg_reduce, apply plans, index maps, delta frames, error records) are unchanged: with
 *    t = 0 the output alpha is 255 as ever, in alpha mode the input's alpha is kept (and the cutoff of the OUTPUT stays t).
 *  - Bound: |q| < 2^27 and a < 2^8, so a working image of up to 2^28 pixels cannot overflow the int64 sums; a larger one is
 *    KMG_ERR_UNSUPPORTED, found on the host before any pass of the loop is enqueued.
 *  - Applies to kmg_palette, kmg_reduce, kmg_reduce_indexed; every palette run of kmg_reduce_quality (whose error measure stays
 *    the UNWEIGHTED record it is without weighting: a pixel of alpha 1 counts as much as one of 255 there); kmg_sequence_* -- the
 *    weighting in force at an add decides that frame's cutoff, as alpha_cutoff is read there, and the weighting in force at
 *    _centroids, _palette, _output_begin or _output_begin_local decides whether the loop is weighted (pixels of weight 0 already
 *    in W add nothing); the cold and warm per-frame palettes of _output_frame_local.
 *  - The sums are always those of the per-pixel passes, whatever kmg_options.strategy says: the colour table's histogram counts
 *    pixels.  (The initialisation may still run over the colour table.)
 *  - KMG_ERR_INVALID_ARGUMENT, nothing written: KMG_ALGO_OCTREE while weighting is on; kmg_group_palette / _reduce /
 *    _reduce_batch when a member processor has it on.
 * kmg_lloyd_set_weighting(s, KMG_WEIGHT_ALPHA) is the device building block: every later sum of that object -- _assign_accumulate,
 * _assign_partials + _reduce_partials, _assign_update, _iterate, _run -- weighs each pixel it is given by its alpha byte (at most
 * 2^28 pixels per pass: KMG_ERR_UNSUPPORTED above); kmg_lloyd_prepare answers strategy 0, and kmg_lloyd_run drops a binding the
 * initialisation left instead of inheriting it.  Refused with KMG_ERR_INVALID_ARGUMENT on such an object: kmg_lloyd_bind_image,
 * _set_cell_share, _accumulate_into, _labels_from_tables_update; and kmg_lloyd_set_weighting itself while the caller holds a
 * binding (kmg_lloyd_bind_image / _prepare).  The kmg_lloyd_* calls still count every pixel they are given: callers compact.     */
#define KMG_WEIGHT_NONE  0
#define KMG_WEIGHT_ALPHA 1

/* kmg_processor_set_fixed_colors -- fixed palette colours: entries the k-means keeps, exactly, and builds the rest around.  No
 * counterpart in the reference.  F = a list of f RGBA8 colours set on a processor (alpha ignored, duplicates allowed,
 * f <= KMG_MAX_K); f = 0, the default, keeps the behaviour described everywhere else in this header, byte for byte.
 * P_j = kmg_palette_to_centroids(F_j): a pinned entry behaves exactly like an entry of a kmg_find palette.
 *  - Palette step (kmg_palette, kmg_reduce, kmg_reduce_indexed, every palette run of kmg_reduce_quality, kmg_sequence_centroids /
 *    _palette / _output_begin), k >= f, on the working image W = the n pixels the default pipeline sees, in its order: after the
 *    shrink, after alpha mode's compaction, after the concatenation of a sequence.
 *    Initialisation (the reference's farthest-point loop with the first f picks replaced):  c_j = P_j for j < f;
 *    dist[i] = 1000000.0f;  for j = 1 .. k - 1:  dist[i] = fminf(dist[i], cie94(pixel_i, c_(j-1)))  (pixel first: CIE94 is
 *    asymmetric), and, when j >= f, c_j = the pixel the arg-max of dist names under the reference's tie rule (inside each block of
 *    16 consecutive pixels the earliest maximum, folded from Candidate(0, 0.0); across blocks the last block that attains it).
 *    With f >= 1 no pixel index derived from width and height enters, so (sw, sh) and |W| x 1 give the same centroids.
 *    Lloyd loop: the reference's, except that for c < f the update leaves the centroid exactly as it is, whatever its count, and
 *    counts it as converged: the convergence count is f + the count over c >= f (an empty free cluster: not converged, as ever).
 *    The check at it > 0 && it % check_period == 0 and max_iterations are unchanged.
 *  - Outputs take the resulting centroid table and are unchanged.  In index order (kmg_reduce_indexed, kmg_sequence_centroids,
 *    the index maps) the pinned entries are indices 0 .. f - 1, in the order given; kmg_palette sorts by L as always.  The
 *    palette bytes of a pinned entry are what the output pass writes for P_j (lab_to_rgb.wgsl) -- the "re-encoded bytes" of
 *    kmg_find_indexed.  That re-encoding is the identity for every one of the 2^24 colours (counted: DESIGN.md 4.10), so
 *    pinned colours come back byte-exact: palette entry j of the index-order outputs has the R, G, B of F_j and alpha 255.
 *  - Alpha mode composes: the pins come first, then the kept pixels as ever.
 *  - KMG_ERR_INVALID_ARGUMENT, nothing written: color_count < f (kmg_reduce_quality: k_min < f); KMG_ALGO_OCTREE while f > 0;
 *    n > KMG_MAX_K, or a NULL list with n > 0; kmg_group_palette / _reduce / _reduce_batch when a member processor has fixed
 *    colours set (the group layer has no pinned path).
 * The call copies the list; n = 0 clears it.  Calls that are already running keep the list they started with.                   */

/* kmg_options.strategy / kmg_processor_set_strategy: which of the library's interchangeable strategies a call takes.  Results are
 * IDENTICAL either way (that is what the tests use the switch for); only the time differs.  The low two bits choose between the
 * per-pixel scans and the colour-table / candidate-list passes for every decision the cost models otherwise make (Lloyd
 * iteration, initialisation, output passes); KMG_STRATEGY_MASK_WORDS sends the pruned dither / meld passes of every k through
 * the mask words per (RGB cell, Bayer index) instead of the byte lists over Lab cells (the path of k > 512).  (An options
 * struct of the previous size -- without this field -- is accepted and means KMG_STRATEGY_AUTO.)                                */
#define KMG_STRATEGY_AUTO       0
#define KMG_STRATEGY_SCAN       1
#define KMG_STRATEGY_TABLE      2
#define KMG_STRATEGY_MASK_WORDS 4

typedef struct kmg_processor kmg_processor;
typedef struct kmg_lloyd kmg_lloyd;
typedef struct kmg_apply_plan kmg_apply_plan;

KMG_API const char *kmg_last_error(void);
KMG_API const char *kmg_version(void);
KMG_API void kmg_default_options(kmg_options *opt);

/* ---- ImageProcessor::new  (core/src/lib.rs:38-65) ------------------------------------- */
KMG_API int kmg_processor_create(kmg_processor **out);
KMG_API int kmg_processor_create_ex(const kmg_options *opt, kmg_processor **out);
KMG_API void kmg_processor_destroy(kmg_processor *p);
/* changes kmg_options.strategy of a live processor (tests and tuning: one processor, both strategies); calls that are
 * already running keep the strategy they started with                                                                        */
KMG_API int kmg_processor_set_strategy(kmg_processor *p, int strategy);
/* changes kmg_options.alpha_cutoff of a live processor (0 .. 255); calls that are already running keep the value they started
 * with                                                                                                                         */
KMG_API int kmg_processor_set_alpha_cutoff(kmg_processor *p, uint32_t alpha_cutoff);
/* kmg_diffusion of a live processor: the filter of the KMG_MODE_DIFFUSE output from now on.  It is read where alpha_cutoff is
 * read, when an apply plan is made: a plan keeps its filter over all its bands, every call that diffuses (kmg_find, kmg_reduce,
 * their _indexed and _batch forms, kmg_dev_apply[_format], kmg_reduce_quality) follows it, and kmg_sequence_output_begin[_local]
 * fixes it for the open output.  NULL or a filter outside 0 .. KMG_DIFFUSION_COUNT - 1: KMG_ERR_INVALID_ARGUMENT, nothing changes */
KMG_API int kmg_processor_set_diffusion(kmg_processor *p, int filter);
/* the table at kmg_diffusion (no device needed): weights points to 12 values, [0..1] row 0 (dx = +1, +2), [2..6] row 1 and [7..11]
 * row 2 (dx = -2 .. +2).  A NULL pointer or an unknown filter: KMG_ERR_INVALID_ARGUMENT, nothing written                          */
KMG_API int kmg_diffusion_weights(int filter, int32_t *weights, int32_t *divisor);
/* kmg_dither_map of a live processor: a built-in threshold map and the strength of the KMG_MODE_DITHER output from now on.  It is
 * read where the diffusion filter is read, when an apply plan is made: a plan keeps a copy of its map and strength for all its
 * runs, every call that dithers (kmg_find, kmg_reduce, their _indexed and _batch forms, kmg_dev_apply[_format],
 * kmg_reduce_quality[_batch], the sequence calls) follows it, and kmg_sequence_output_begin[_local] fixes it for the open output,
 * single frames and clips alike.  A plan whose device cannot hold the centroid table and the map in one workgroup's LDS (k close
 * to KMG_MAX_K with a 64 x 64 map on a device with 64 KiB) is KMG_ERR_UNSUPPORTED.
 * NULL, an unknown map, KMG_DITHER_CUSTOM, or a strength that is not finite or outside [0, 4]: KMG_ERR_INVALID_ARGUMENT, nothing
 * changes                                                                                                                        */
KMG_API int kmg_processor_set_dither(kmg_processor *p, int map, float strength);
/* the same with the caller's own map: levels points to width x height values, row-major, which are copied.  Also refused
 * (KMG_ERR_INVALID_ARGUMENT, nothing changes): a side that is 0, above 64 or not a power of two, n_levels of 0 or above 65536, a
 * level that is not below n_levels                                                                                                */
KMG_API int kmg_processor_set_dither_custom(kmg_processor *p, const uint16_t *levels, uint32_t width, uint32_t height, uint32_t n_levels,
                                            float strength);
/* the table of a built-in map (no device needed): levels points to room for 4096 values and receives width x height of them,
 * row-major.  A NULL pointer, an unknown map or KMG_DITHER_CUSTOM: KMG_ERR_INVALID_ARGUMENT, nothing written                       */
KMG_API int kmg_dither_map_values(int map, uint32_t *width, uint32_t *height, uint32_t *n_levels, uint16_t *levels);
/* KMG_WEIGHT_*: whether the palette step weighs a pixel by its alpha byte, see above                                              */
KMG_API int kmg_processor_set_weighting(kmg_processor *p, int weighting);
/* sets (n > 0: copies n x 4 bytes) or clears (n = 0) the processor's fixed colours, see above                                     */
KMG_API int kmg_processor_set_fixed_colors(kmg_processor *p, const uint8_t *rgba, uint32_t n);
/* Page-locked host memory for images that cross the boundary often (a frame loop): a result buffer from kmg_host_alloc has
 * its pages resident and is copied to by DMA directly -- kmg_reduce of 8192 x 8192 into a fresh pageable buffer spends 30-50 ms
 * in the caller's page faults, 10 ms into one of these.  Plain memory otherwise; release with kmg_host_free.  (No counterpart
 * in the reference, whose results are fresh Vecs: structures.rs:441-470.)                                                    */
KMG_API int kmg_host_alloc(size_t bytes, void **out);
KMG_API void kmg_host_free(void *ptr);
/* Test support: out[0] = device blocks the processor has allocated with hipMalloc so far, out[1] = blocks it has handed out
 * again (colour tables, workspaces and output-pass scratch of finished objects are kept and reused).                 */
KMG_API int kmg_debug_block_counts(kmg_processor *p, uint64_t out[2]);
/* Test support: out[0] = blocks the processor holds idle right now, out[1] = their bytes.  The idle list is bounded (24 blocks,
 * 3 GiB: the oldest go first) and is emptied when an allocation fails for lack of memory.                                  */
KMG_API int kmg_debug_idle_blocks(kmg_processor *p, uint64_t out[2]);
/* Test support: the meld pass turns a linear channel value into its sRGB8 byte with a 255-entry threshold table made on
 * the device by the encode of lab_to_rgb.wgsl:21-35 itself; *mismatches = the float values (every bit pattern, NaN aside)
 * for which table and encode give different bytes (0 = the table IS the encode).                                     */
KMG_API int kmg_debug_encode_table_check(kmg_processor *p, uint64_t *mismatches);
/* Test support: the device divides by the constants of lab_to_rgb.wgsl:45-59 (116, 500, 200, 100, 7.787) and of
 * rgb_to_lab.wgsl (the white point) with a reciprocal and one residual correction; out[0] = the number of binary32 x (every
 * bit pattern, NaN aside) for which that is not the IEEE quotient x / c, out[1] / out[2] = the smallest / largest |x| bit
 * pattern among them (out[1] = 2^64 - 1 when there is none).                                                          */
KMG_API int kmg_debug_division_check(kmg_processor *p, float c, uint64_t out[3]);

/* ---- ImageProcessor::palette  (core/src/lib.rs:67-77, 255-286) -------------------------
 * out_rgba: capacity color_count*4 bytes; *out_count receives the number of colours
 * (== color_count for k-means), sorted ascending by Lab L.                                 */
KMG_API int kmg_palette(kmg_processor *p, const uint8_t *rgba, uint32_t width, uint32_t height,
                        uint32_t color_count, int algo, uint8_t *out_rgba, uint32_t *out_count);

/* ---- ImageProcessor::find  (core/src/lib.rs:79-114) ------------------------------------ */
KMG_API int kmg_find(kmg_processor *p, const uint8_t *rgba, uint32_t width, uint32_t height,
                     const uint8_t *palette_rgba, uint32_t n_colors, int mode, uint8_t *out_rgba);

/* ---- ImageProcessor::reduce  (core/src/lib.rs:116-164) --------------------------------- */
KMG_API int kmg_reduce(kmg_processor *p, const uint8_t *rgba, uint32_t width, uint32_t height,
                       uint32_t color_count, int algo, int mode, uint8_t *out_rgba);

/* ---- the same two calls with an output format (kmg_output_format) ------------------------
 * out_index: width * height pixels of the format (4, 1 or 2 bytes each).  kmg_reduce_indexed also returns the palette in index
 * order -- the centroid order of the output pass, NOT sorted (k-means: the Lloyd loop's order; octree: kmg_palette's order) --
 * as the bytes the RGBA8 output writes for each index: out_palette_rgba has room for color_count x 4 bytes, *out_count
 * receives the number of entries.  KMG_FORMAT_RGBA8 writes exactly what kmg_find / kmg_reduce write.                   */
KMG_API int kmg_find_indexed(kmg_processor *p, const uint8_t *rgba, uint32_t width, uint32_t height,
                             const uint8_t *palette_rgba, uint32_t n_colors, int mode, int format, void *out_index);
KMG_API int kmg_reduce_indexed(kmg_processor *p, const uint8_t *rgba, uint32_t width, uint32_t height, uint32_t color_count,
                               int algo, int mode, int format, uint8_t *out_palette_rgba, uint32_t *out_count, void *out_index);

/* ---- batches: many small images per launch on one device ---------------------------------
 * No counterpart in the reference, which quantises image after image.  The default call works on an image shrunk to at most
 * 256 x 256: a few hundred workgroups on 256 CUs and a chain of launches whose length does not depend on the image.  A batch runs
 * that chain ONCE for all its images: launch j of the initialisation is pass j of every image, a launch of the loop is one Lloyd
 * iteration of every image that is still running (kmg_batch.hip).
 *
 * Equivalence.  kmg_palette_batch / kmg_reduce_batch write for image i exactly the bytes (and out_counts[i]) that kmg_palette /
 * kmg_reduce of image i alone write on the same processor; kmg_dev_palette_batch gives the centroids and the iteration count that
 * kmg_lloyd_init_centroids + kmg_lloyd_run + kmg_lloyd_get_centroids give for image i.  Images may differ in size, an image may
 * appear twice, and neither the order of the batch nor max_resident_bytes changes any image's result.  An image stops where
 * kmg_lloyd_run stops it -- at the check after iteration `it` (it > 0, it % check_period == 0) with every centroid converged, or at
 * max_iterations; later launches leave it alone.  kmg_options.strategy changes nothing: the batch is the per-pixel route.
 *
 * Per-image steps.  The shrink and alpha mode's compaction are the existing ones (kmg_dev_resize, kmg_dev_alpha_compact), enqueued
 * per image; the kept-pixel counts of a sub-batch come back in one copy.  A working image of 2^19 pixels or more (shrink off or
 * shrink_max_dim large) takes the per-image path inside the call and counts in `fallback`.  KMG_ALGO_OCTREE runs the host
 * algorithm per image (the report stays 0 apart from sub_batches).  A sub-batch of ONE image (a batch of one, or max_resident_bytes
 * cutting an image off alone) takes the per-image palette step of kmg_palette: no batched launch, so `launches` counts none for it;
 * `iterations` covers it all the same.  kmg_reduce_batch's output step is the per-image output pass at
 * full size with that image's centroids; the sources stay on the device between their shrink and their output pass.
 *
 * max_resident_bytes (0 = 1 GiB) bounds what a call keeps on the device at once: the batch is cut into consecutive sub-batches
 * whose images' resident bytes fit (an image that does not fit alone forms a sub-batch of its own).  An image counts with
 * 4 * width * height bytes for its source -- kmg_palette_batch: only where the image is not shrunk, a shrunk source is released as
 * soon as its shrink is enqueued -- plus 4 bytes per pixel of its shrunk copy where it has one, plus the same again in alpha mode
 * for the compacted copy.  (The batched state itself, ~ 12 bytes per working pixel + 128 k bytes per image, rides on top.)
 *
 * Refusals, KMG_ERR_INVALID_ARGUMENT, checked for the whole batch before anything is uploaded, in this order: a NULL processor;
 * n_images == 0; a NULL array; then per image in order a NULL entry or a zero dimension; color_count == 0; an algorithm or mode out
 * of range; (color_count > KMG_MAX_K with k-means: KMG_ERR_UNSUPPORTED;) fixed colours set on the processor; alpha weighting on --
 * there is no seeded or weighted batched path yet, the group calls refuse both for the same reason.  Alpha mode: an image that
 * keeps no pixel refuses the call, the message names its index; this is found on the device after the shrinks, still before
 * any output is written (with several sub-batches the call shrinks everything once more up front to find it).  Any other failure
 * returns the first error; which outputs were written by then is unspecified.
 *
 * report (may be NULL): what the call did.                                                                                         */
typedef struct kmg_batch_report {   /* 16 bytes, no padding */
    uint32_t launches;      /* kernel launches of the batched initialisation + loop (not shrink, compaction, the final gather, output) */
    uint32_t iterations;    /* largest iteration count of any image                                                                      */
    uint32_t sub_batches;   /* how many pieces max_resident_bytes cut the batch into                                                     */
    uint32_t fallback;      /* images that took the per-image path (working image >= 2^19 pixels)                                        */
} kmg_batch_report;

/* device building block: working images already on the device (d_rgba: a HOST array of n_images device pointers), centroids in
 * index order as (L, a, b, 1).  centroids4: host, n_images * k * 4 floats; iterations: host, n_images, may be NULL.  The
 * initialisation takes k launches, the loop 1 + its iterations, whatever n_images is (up to 2^20 tiles of 256 pixels in all; a
 * larger batch runs as several such chains, one after the other).  The state of the batch is carved from the
 * processor's idle blocks (no hipMalloc on a warm processor).  Ignores the processor's alpha cutoff, fixed colours and weighting,
 * as the kmg_lloyd_* calls do.  Synchronises `stream`.                                                                          */
KMG_API int kmg_dev_palette_batch(kmg_processor *p, uint32_t n_images, const uint8_t *const *d_rgba, const uint32_t *widths,
                                  const uint32_t *heights, uint32_t k, float *centroids4, uint32_t *iterations,
                                  kmg_batch_report *report, void *stream);
/* host buffers, as kmg_palette / kmg_reduce per image: rgba, widths, heights, out_rgba (and out_counts) are arrays of n_images
 * entries; out_rgba[i] has room for color_count * 4 bytes (palette) or widths[i] * heights[i] * 4 bytes (reduce)                */
KMG_API int kmg_palette_batch(kmg_processor *p, uint32_t n_images, const uint8_t *const *rgba, const uint32_t *widths,
                              const uint32_t *heights, uint32_t color_count, int algo, uint64_t max_resident_bytes,
                              uint8_t *const *out_rgba, uint32_t *out_counts, kmg_batch_report *report);
KMG_API int kmg_reduce_batch(kmg_processor *p, uint32_t n_images, const uint8_t *const *rgba, const uint32_t *widths,
                             const uint32_t *heights, uint32_t color_count, int algo, int mode, uint64_t max_resident_bytes,
                             uint8_t *const *out_rgba, kmg_batch_report *report);

/* ---- batched output: find and indexed reduce for many small images ------------------------
 * The output step of a batch in ONE launch for all its images (kmg_batch_apply.hip): a workgroup finds the image
 * its tile belongs to and runs the per-pixel output pass on it with that image's width, threshold and tables.  kmg_palette_batch,
 * kmg_reduce_batch and every per-image call keep their code paths and their bytes.
 *
 * Equivalence.  Image i receives exactly the bytes the per-image call writes for image i alone on the same processor:
 * kmg_find_batch those of kmg_find_indexed, kmg_reduce_indexed_batch those of kmg_reduce_indexed (also the palette in index order
 * and out_counts[i]), kmg_dev_apply_batch those of kmg_dev_apply_format; KMG_FORMAT_RGBA8 means the bytes of kmg_find / kmg_reduce.
 * Neither the order of the batch, an image appearing twice, max_resident_bytes nor kmg_options.strategy changes any image's bytes.
 *
 * Which images join the launch.  Image i joins when the mode is KMG_MODE_REPLACE or KMG_MODE_DITHER and its own output plan would
 * scan all centroids per pixel (the route kmg_dev_apply takes for a small image); in a batch of two images or more also a dither
 * image with 128 .. 512 colours that a plan of its own sends to the candidate lists only for the latency of one image's scan
 * (DESIGN.md 4.17).  Every other image -- KMG_MODE_MELD,
 * KMG_MODE_DIFFUSE, an image large enough for the colour table, the candidate lists or the mask words, a forced
 * KMG_STRATEGY_TABLE -- takes its own output pass inside the call and counts in `per_image`.  KMG_ALGO_OCTREE runs the host
 * algorithm and the per-image output pass, as in kmg_reduce_batch (palette sizes differ per image): every image is `per_image`.
 *
 * max_resident_bytes: as for kmg_reduce_batch -- the source stays on the device until its output -- plus the bytes of the image's
 * output (4, 1 or 2 per pixel); kmg_find_batch counts the source and the output.
 *
 * Refusals, KMG_ERR_INVALID_ARGUMENT unless stated, checked for the whole batch before anything is uploaded, in this order (the
 * order of kmg_reduce_batch, continued): a NULL processor; n_images == 0; a NULL array; then per image in order a NULL entry or a
 * zero dimension; k == 0 (color_count, n_colors or a NULL palette); an algorithm, mode or format out of range; k > KMG_MAX_K
 * (KMG_ERR_UNSUPPORTED; kmg_reduce_indexed_batch: with k-means); the rules of the index formats -- KMG_MODE_MELD has no index,
 * KMG_FORMAT_INDEX8 needs k <= 256 (k <= 255 in alpha mode), a palette entry outside the box of the index formats; fixed colours or
 * alpha weighting on the processor (kmg_reduce_indexed_batch only; kmg_find_batch ignores both, as kmg_find does); n_tables other
 * than 1 or n_images, then an INDEX16 output that is not 2-byte aligned (kmg_dev_apply_batch).  Alpha mode's "image keeps no
 * pixel" refusal of kmg_reduce_indexed_batch is that of kmg_reduce_batch.  Any other failure returns the first error; which
 * outputs were written by then is unspecified.                                                                                  */
typedef struct kmg_batch_apply_report {   /* 16 bytes, no padding */
    uint32_t launches;     /* launches of the batched output kernel                 */
    uint32_t batched;      /* images written by them                                */
    uint32_t per_image;    /* images that took their own output pass                */
    uint32_t sub_batches;  /* how many pieces max_resident_bytes cut the batch into */
} kmg_batch_apply_report;

/* device building block, as kmg_dev_palette_batch: d_rgba and d_out are HOST arrays of n_images device pointers (images of
 * widths[i] x heights[i] pixels; outputs of 4, 1 or 2 bytes per pixel); centroids4: HOST, n_tables tables of k x 4 floats in index
 * order -- n_tables = 1: one table for all images, n_tables = n_images: table i for image i.  The alpha cutoff is the
 * processor's, read as kmg_dev_apply_format reads it.  report (may be NULL): sub_batches = 1.  Synchronises `stream`.          */
KMG_API int kmg_dev_apply_batch(kmg_processor *p, uint32_t n_images, const uint8_t *const *d_rgba, const uint32_t *widths,
                                const uint32_t *heights, const float *centroids4, uint32_t n_tables, uint32_t k, int mode, int format,
                                void *const *d_out, kmg_batch_apply_report *report, void *stream);
/* host buffers, as kmg_find_indexed per image with ONE palette for all images: out[i] has room for widths[i] * heights[i]
 * outputs of `format`                                                                                                           */
KMG_API int kmg_find_batch(kmg_processor *p, uint32_t n_images, const uint8_t *const *rgba, const uint32_t *widths,
                           const uint32_t *heights, const uint8_t *palette_rgba, uint32_t n_colors, int mode, int format,
                           uint64_t max_resident_bytes, void *const *out, kmg_batch_apply_report *report);
/* host buffers, as kmg_reduce_indexed per image: out_palette_rgba[i] has room for color_count * 4 bytes, out_counts[i] receives
 * the number of entries, out_index[i] has room for widths[i] * heights[i] outputs of `format`.  batch_report: what
 * kmg_reduce_batch reports for the palettes; apply_report: the output step (both may be NULL)                                   */
KMG_API int kmg_reduce_indexed_batch(kmg_processor *p, uint32_t n_images, const uint8_t *const *rgba, const uint32_t *widths,
                                     const uint32_t *heights, uint32_t color_count, int algo, int mode, int format,
                                     uint64_t max_resident_bytes, uint8_t *const *out_palette_rgba, uint32_t *out_counts,
                                     void *const *out_index, kmg_batch_report *batch_report, kmg_batch_apply_report *apply_report);

/* ---- host-side colour helpers the reference takes from the `palette` crate -------------
 * CentroidsBuffer::fixed_centroids (core/src/structures.rs:523-553): sRGB8 -> Lab (L,a,b,1)  */
KMG_API int kmg_palette_to_centroids(const uint8_t *palette_rgba, uint32_t n_colors, float *centroids4);
/* CentroidsBuffer::pull_values (core/src/structures.rs:581-617): Lab -> sRGB8 (alpha 255)    */
KMG_API int kmg_centroids_to_palette(const float *centroids4, uint32_t k, uint8_t *out_rgba);
/* ColorTree::{add_color, reduce} (core/src/octree.rs:28-115, core/src/operations.rs:90-97): the
 * reference's CPU octree quantiser on n_pixels RGBA8 pixels.  out_rgba: capacity 4 * min(color_count,
 * n_pixels) bytes; *out_count <= color_count colours, sorted (r, g, b, a), deduplicated.  Host only.  */
KMG_API int kmg_octree_palette(const uint8_t *rgba, uint64_t n_pixels, uint32_t color_count,
                               uint8_t *out_rgba, uint32_t *out_count);

/* ======================= device-pointer API (hot path building blocks) ================== */
/* `stream` is a hipStream_t (NULL = the default stream).  Calls only enqueue work unless the
 * comment says they synchronise.                                                            */

/* ColorConverterModule, rgb_to_lab.wgsl:66-80: RGBA8 -> Lab, 3 floats per pixel.            */
KMG_API int kmg_dev_rgb_to_lab(kmg_processor *p, const uint8_t *d_rgba, uint64_t n_pixels,
                               float *d_lab3, void *stream);

/* InputTexture::resized (core/src/structures.rs:76-182, resize.wgsl:7-18).                   */
KMG_API void kmg_resized_dims(uint32_t width, uint32_t height, uint32_t max_size,
                              uint32_t *new_width, uint32_t *new_height);
KMG_API int kmg_dev_resize(kmg_processor *p, const uint8_t *d_rgba, uint32_t width, uint32_t height,
                           uint32_t new_width, uint32_t new_height, uint8_t *d_out_rgba, void *stream);

/* Ordered stream compaction for alpha mode (kmg_options.alpha_cutoff): d_out[0 .. n_kept) = the pixels of d_rgba whose alpha
 * byte is >= cutoff, in their order; *d_n_kept (a DEVICE word) = n_kept.  d_out has room for n_pixels pixels and does not
 * overlap d_rgba.  cutoff 0 keeps every pixel; above 255: KMG_ERR_INVALID_ARGUMENT.  Only enqueues work on `stream`.       */
KMG_API int kmg_dev_alpha_compact(kmg_processor *p, const uint8_t *d_rgba, uint64_t n_pixels, uint32_t cutoff,
                                  uint8_t *d_out, uint64_t *d_n_kept, void *stream);

/* One Lloyd problem = one image (or one row band of it) with k centroids.
 * ChooseCentroidModule + FindCentroidModule state (core/src/modules.rs:452-761).             */
KMG_API int kmg_lloyd_create(kmg_processor *p, uint32_t k, kmg_lloyd **out);
KMG_API void kmg_lloyd_destroy(kmg_lloyd *s);
/* centroid table up/down (synchronise `stream`) */
KMG_API int kmg_lloyd_set_centroids(kmg_lloyd *s, const float *centroids4, void *stream);
KMG_API int kmg_lloyd_get_centroids(kmg_lloyd *s, float *centroids4, void *stream);

/* PlusPlusInitModule::compute (core/src/modules.rs:946-1246, plus_plus_init.wgsl,
 * kmeans++_calc_diff.wgsl): deterministic farthest-point initialisation on the device.       */
KMG_API int kmg_lloyd_init_centroids(kmg_lloyd *s, const uint8_t *d_rgba, uint32_t width,
                                     uint32_t height, void *stream);

/* The same initialisation with the first n_seeds centroids GIVEN (seeds4: HOST, n_seeds x 4 floats, (L, a, b, ignored), finite):
 * the loop described at kmg_processor_set_fixed_colors with arbitrary Lab seeds for P -- the running distances start from all the
 * seeds, centroids n_seeds .. k - 1 are the farthest-point picks that follow.  n_seeds = 0 is kmg_lloyd_init_centroids, bit for
 * bit; n_seeds > k: KMG_ERR_INVALID_ARGUMENT.  It starts a new problem exactly as kmg_lloyd_init_centroids does (the binding
 * rules at kmg_lloyd_bind_image).  Seeding is separate from freezing: without kmg_lloyd_set_fixed the seeds move with the first
 * update (a warm start from the last frame's palette).  Synchronises `stream`.                                                   */
KMG_API int kmg_lloyd_init_centroids_seeded(kmg_lloyd *s, const uint8_t *d_rgba, uint32_t width, uint32_t height,
                                            const float *seeds4, uint32_t n_seeds, void *stream);
/* Freezes centroids 0 .. n_fixed - 1 (n_fixed <= k; default 0): every update this object performs from now on --
 * kmg_lloyd_update, _assign_update, _iterate, _run, _labels_from_tables_update -- leaves them exactly as they are and counts them
 * as converged (kmg_lloyd_converged_count includes them).  Their sums are still accumulated and returned in d_acc4.  The value
 * has reached the device when the call returns (a small blocking copy): it holds for the updates enqueued after it, on any
 * stream, not for those enqueued before.  Refused (KMG_ERR_INVALID_ARGUMENT) while a cell share is set, like the updates
 * themselves.                                                                                                                   */
KMG_API int kmg_lloyd_set_fixed(kmg_lloyd *s, uint32_t n_fixed);
/* KMG_WEIGHT_*: whether the sums of this object weigh a pixel by its alpha byte (at kmg_processor_set_weighting above)            */
KMG_API int kmg_lloyd_set_weighting(kmg_lloyd *s, int weighting);

/* The same initialisation for an image sharded in row bands (one kmg_lloyd per band / GPU).  Step j:
 *   kmg_lloyd_init_step      band-local pass for centroid j-1; *d_key (device u64) = arg-max key of
 *                            this band over IMAGE-wide pixel indices (first_index = index of the band's
 *                            first pixel).  The caller all-reduces the key with MAX (compare as signed
 *                            or unsigned 64-bit: the top bit is never set).
 *   kmg_lloyd_init_pick_band d_colour2[0..1] = {RGBA8 of the pixel the reduced key names, 1} on the band
 *                            that owns that pixel, {0, 0} elsewhere.  The caller all-reduces with SUM.
 *   kmg_lloyd_set_centroid_rgba   centroid j <- shader Lab of d_colour[0].
 * Centroid 0 uses the same two calls with kmg_init_first_key(width, height) as the key.  Everything
 * is enqueued on `stream`; nothing synchronises.                                                     */
KMG_API int kmg_lloyd_init_step(kmg_lloyd *s, const uint8_t *d_rgba, uint64_t n_local, uint64_t first_index,
                                uint32_t j, uint64_t *d_key, void *stream);
KMG_API int kmg_lloyd_init_pick_band(kmg_lloyd *s, const uint8_t *d_rgba, uint64_t n_local, uint64_t first_index,
                                     const uint64_t *d_key, uint32_t *d_colour2, void *stream);
KMG_API int kmg_lloyd_set_centroid_rgba(kmg_lloyd *s, uint32_t j, const uint32_t *d_colour, void *stream);
KMG_API uint64_t kmg_init_first_key(uint32_t width, uint32_t height);

/* FindCentroidModule::dispatch (find_centroid.wgsl:15-44) fused with the masked sums of
 * choose_centroid.wgsl:75-178: labels for every pixel AND the k x 4 int64 accumulators of this
 * pixel range, one pass over the RGBA8 data.  d_acc4 may be NULL (assignment only);
 * d_labels may be NULL (sums only).                                                          */
KMG_API int kmg_lloyd_assign_accumulate(kmg_lloyd *s, const uint8_t *d_rgba, uint64_t n_pixels,
                                        uint32_t *d_labels, int64_t *d_acc4, void *stream);

/* Optional, for large images: build the image's colour table (24-bit colour histogram + per-cell
 * sums) once.  Subsequent assign passes on the SAME (d_rgba, n_pixels) then iterate over distinct
 * colours with conservatively pruned candidate sets and materialise labels with one gather pass;
 * labels, sums and centroids are bit-identical to the per-pixel scan.  kmg_lloyd_run binds by
 * itself when its cost model says it pays (kmg_options.strategy overrides).  The caller
 * must not modify the pixel buffer while it is bound.  kmg_lloyd_init_centroids / _init_step (j = 1)
 * start a new problem: they drop any earlier binding of the buffer, for every k (and bind it afresh
 * when the initialisation itself runs over the colour table).  That binding is the library's own: it
 * serves the kmg_lloyd_run / _prepare of the problem the initialisation started, and
 * kmg_lloyd_set_centroids ends that problem -- after it, run and prepare read the buffer's current
 * contents again (the next frame in the same buffer).                                            */
KMG_API int kmg_lloyd_bind_image(kmg_lloyd *s, const uint8_t *d_rgba, uint64_t n_pixels, void *stream);
KMG_API int kmg_lloyd_unbind_image(kmg_lloyd *s);
/* Tuning support: what the binding found in the image -- out[0] = occupied cells of the 32^3 grid over the colour cube (the cube
 * pass's work list), out[1] = hot cells (the few cells that hold a tenth or more of the pixels: a photograph's dark corner; 0
 * on noise).  These are what the cost model looks at AFTER a binding (kmg_lloyd_prepare): a sparse image has a cheaper cube pass
 * than the noise the model was fitted on, an image with hot cells a dearer per-pixel scan (near-tie repairs).                  */
KMG_API int kmg_debug_bound_image(kmg_lloyd *s, uint64_t out[2]);
/* One-time preparation of (d_rgba, n_pixels) for repeated assign passes: applies the library's cost
 * model (want_labels = whether the passes will materialise labels) and binds the image if the colour
 * table pays.  *strategy (optional) receives 0 = per-pixel scan, 1 = colour table.              */
KMG_API int kmg_lloyd_prepare(kmg_lloyd *s, const uint8_t *d_rgba, uint64_t n_pixels, int want_labels,
                              int *strategy, void *stream);
/* Test support: exhaustive check over all 2^24 colours of the colour-table pass for the current
 * centroids.  out[0] = (colour, centroid) pairs whose key lies outside the interval bounds of the colour's
 * cell or sub-cell, out[1] = colours whose true arg-min is missing from its cell's candidate set,
 * out[2] = colours whose label in the per-colour table is not the true arg-min (all must be 0). */
KMG_API int kmg_debug_check_table(kmg_lloyd *s, uint64_t out[3], void *stream);
/* Tuning support: statistics of the last colour-table pass over the bound image (synchronises).
 * out = {occupied cells, sum of candidate counts, cells with one candidate, max candidates,
 *        cells with one label, occupied sub-cells, sub-cells with one label, distinct colours,
 *        sub-cells decided from their bounds, sub-cells scanned, candidates over the scanned sub-cells,
 *        cells with too many candidates for the sub-cell stage, candidates the dominance phase removed from
 *        scanned sub-cells, scanned sub-cells it left with one candidate}.                      */
KMG_API int kmg_debug_table_stats(kmg_lloyd *s, uint64_t out[14], void *stream);
/* Test support (k <= 256): checks the per-cell pair entries the label pass keeps in LDS against the
 * per-colour label table of the last colour-table pass (synchronises).  out[0] = occupied colours
 * whose entry disagrees (must be 0), out[1] = pixels resolved by the entries alone, out[2] = pixels. */
KMG_API int kmg_debug_check_pairs(kmg_lloyd *s, uint64_t out[3], void *stream);
/* Test support: exhaustive check (2^24 colours x 16 Bayer offsets) that the candidate masks of the
 * pruned dither pass for this centroid table (k >= 2, (L, a, b, pad) per entry) contain every pixel's
 * true arg-min of mix_colors.wgsl:73-80.  *violations must come back 0.                            */
KMG_API int kmg_debug_check_dither_masks(kmg_processor *p, const float *centroids4, uint32_t k, uint64_t *violations,
                                         void *stream);
/* Test support: the same exhaustive check (2^24 colours) for the pruned meld pass: the two closest
 * centroids of mix_colors.wgsl:29-48 found among a cell's candidates must be those of the full scan.  */
KMG_API int kmg_debug_check_meld_masks(kmg_processor *p, const float *centroids4, uint32_t k, uint64_t *violations,
                                       void *stream);

/* Labels only, for the CURRENT centroid table: find_centroid.wgsl:15-44 without the sums.  With a
 * bound image whose label tables are current (an assign pass ran since the last centroid change) this
 * is just the label-gather pass.                                                                 */
KMG_API int kmg_lloyd_labels(kmg_lloyd *s, const uint8_t *d_rgba, uint64_t n_pixels, uint32_t *d_labels, void *stream);
/* Cell-sharded cube pass, for ONE image sharded over `parts` ranks (strong scaling; no counterpart in the reference, which
 * is single-device: core/src/lib.rs:38-65).  Every rank binds the WHOLE image's colour histogram (its band's histogram,
 * all-reduced) and labels the colours of one share of the colour cube per iteration: after _set_cell_share(part, parts)
 * the assign passes of a bound image visit only the occupied cells whose index lies in [32768 part / parts,
 * 32768 (part + 1) / parts) -- equal RANGES of the colour cube (slabs of the red axis), so that the shares of the label tables
 * are equal contiguous chunks an in-place all-gather can move; the WORK per share is equal only when the occupied cells are
 * spread evenly (noise: yes; the test photograph: the fullest of 2 / 4 / 8 shares holds 1.20 / 1.25 / 1.31 x the mean number of
 * occupied cells -- counted, not timed; its crowded dark cells carry more candidates each).  The sums such a pass returns
 * are those of the share's colours (the all-reduce of the k x 4 accumulators makes them the image's), and only the share's
 * per-colour labels and cell entries are (re)written.  The ranks then exchange their shares of the label tables
 * (_table_buffers: the per-colour labels, cell-major, 512 per cell, and the cell entries) and write their band's label map
 * with _labels_from_tables, which applies the tables as they stand to ANY pixels whose colours occur in the bound image.
 * While a share is set, a pass that asks for a label map, a centroid update (kmg_lloyd_assign_update with do_update,
 * kmg_lloyd_run, kmg_lloyd_iterate) or the two-step partial sums is refused with KMG_ERR_INVALID_ARGUMENT -- it would be that
 * of a fraction of the image.  parts = 1 restores the whole list.                                                        */
KMG_API int kmg_lloyd_set_cell_share(kmg_lloyd *s, uint32_t part, uint32_t parts, void *stream);
/* The bound image's colour histogram (2^24 u32 counts in the library's cell-major colour order) for the all-reduce that
 * turns the band's histogram into the image's, and the call that re-derives everything a binding derives from it (cell
 * sums, occupied and hot cells; synchronises) -- n_pixels = the pixels the histogram now counts (< 2^32).            */
KMG_API int kmg_lloyd_histogram_buffer(kmg_lloyd *s, void **hist, uint64_t *bytes);
KMG_API int kmg_lloyd_rebuild_from_histogram(kmg_lloyd *s, uint64_t n_pixels, void *stream);
KMG_API int kmg_lloyd_labels_from_tables(kmg_lloyd *s, const uint8_t *d_rgba, uint64_t n_pixels, uint32_t *d_labels,
                                         void *stream);
KMG_API int kmg_lloyd_table_buffers(kmg_lloyd *s, void **colour_labels, uint64_t *colour_label_bytes, void **entries,
                                    uint64_t *entry_bytes);
/* Two launches fewer per iteration of such a loop (k <= 256): the cube pass ADDS its sums to d_acc4 as it stands -- the caller keeps
 * the buffer zero between passes; no hand-over launch -- and the label pass of the band also performs kmg_lloyd_update from
 * d_acc4 (the all-reduced sums) and clears it for the next pass: per iteration  _accumulate_into -> all-reduce -> all-gather ->
 * _labels_from_tables_update  instead of  _assign_accumulate -> all-reduce -> all-gather -> _labels_from_tables -> _update.
 * One assignment with its label map and one update per iteration, shifted by half a step (as kmg_lloyd_assign_update).        */
KMG_API int kmg_lloyd_accumulate_into(kmg_lloyd *s, const uint8_t *d_rgba, uint64_t n_pixels, int64_t *d_acc4, void *stream);
KMG_API int kmg_lloyd_labels_from_tables_update(kmg_lloyd *s, const uint8_t *d_rgba, uint64_t n_pixels, uint32_t *d_labels,
                                                int64_t *d_acc4, void *stream);

/* The label pass of the colour-table strategy (k <= 256) runs one 1024-thread workgroup per compute unit for its whole
 * duration.  A kernel launched beside it on another stream -- the RCCL all-reduce of the sums that a sharded loop issues
 * asynchronously: 256 threads, 20 KiB LDS, 280 registers per lane -- finds no CU it fits on and would run
 * BEHIND the pass.  n_cus > 0 leaves that many CUs without a label workgroup (n_cus / 256 of the pass's throughput) so
 * that the collective runs beside it.  0 (default): all CUs.                                                          */
KMG_API int kmg_lloyd_reserve_cus(kmg_lloyd *s, uint32_t n_cus);

/* The two halves of kmg_lloyd_assign_accumulate, for callers that time or batch them:
 * _assign_partials runs the fused per-pixel kernel (labels + per-workgroup partial sums kept in
 * the state), _reduce_partials folds the partial sums of that same launch into d_acc4.        */
KMG_API int kmg_lloyd_assign_partials(kmg_lloyd *s, const uint8_t *d_rgba, uint64_t n_pixels,
                                      uint32_t *d_labels, void *stream);
KMG_API int kmg_lloyd_reduce_partials(kmg_lloyd *s, uint64_t n_pixels, int64_t *d_acc4, void *stream);

/* Per-launch timing of the state's kernels with HIP events recorded on the launch stream itself
 * (bench.py's roofline leg).  _profile(mask) starts collecting for the kernel ids whose bit is set
 * (-1 = all, 0 = stop); _profile_read synchronises the recorded events, returns the summed duration
 * and launch count per kernel id and resets.  Every timed launch adds two event records to the
 * stream, so time only what is needed inside a throughput measurement.
 * KMG_K_CUBE covers the launches of the cube pass (k_cube_stage, k_cube_scan, k_cube_pairs; k <= 32: k_cube_small) as one interval;
 * KMG_K_CANDIDATES is the candidate kernel of the first release, now the first phase of k_cube_stage: the id is
 * kept so that the others do not move, nothing is reported under it.                                             */
typedef enum kmg_kernel_id {
    KMG_K_ASSIGN = 0, KMG_K_REDUCE = 1, KMG_K_UPDATE = 2, KMG_K_CANDIDATES = 3, KMG_K_CUBE = 4,
    KMG_K_LABELS = 5, KMG_K_COUNT = 6
} kmg_kernel_id;
KMG_API const char *kmg_kernel_name(int id);
KMG_API int kmg_lloyd_profile(kmg_lloyd *s, int enable);
KMG_API int kmg_lloyd_profile_read(kmg_lloyd *s, double total_ms[KMG_K_COUNT], uint32_t launches[KMG_K_COUNT]);

/* choose_centroid.wgsl:180-206 `pick` for all k at once: centroid <- sum/count, convergence
 * flags.  d_acc4 holds the (all-reduced) accumulators.                                        */
KMG_API int kmg_lloyd_update(kmg_lloyd *s, const int64_t *d_acc4, void *stream);
/* The loop body of ChooseCentroidModule::compute (modules.rs:769-800) shifted by half a step: the assign pass of
 * kmg_lloyd_assign_accumulate (labels optional, sums into d_acc4) and then -- do_update != 0 -- kmg_lloyd_update from
 * those sums.  Same results as the two calls; with a bound image (colour table) the update is done by the last launch of
 * the assign pass itself (one launch and one memset fewer per iteration).  d_acc4 holds the sums on return, the label
 * tables keep describing the assignment just made.  Sharded images need the all-reduce between the two halves and use
 * the separate calls.                                                                           */
KMG_API int kmg_lloyd_assign_update(kmg_lloyd *s, const uint8_t *d_rgba, uint64_t n_pixels, uint32_t *d_labels,
                                    int64_t *d_acc4, int do_update, void *stream);
/* convergence[K] of choose_centroid.wgsl:196-202 after the last update (synchronises).       */
KMG_API int kmg_lloyd_converged_count(kmg_lloyd *s, uint32_t *count, void *stream);

/* One iteration of the loop of ChooseCentroidModule::compute (modules.rs:769-800) as ONE asynchronous call:
 * update_first != 0: centroids <- kmg_lloyd_update(d_acc4); then labels (optional) + sums of the new
 * assignment into d_acc4 (cleared first).  With a bound image (colour table) and d_labels != NULL the label
 * pass runs on an internal high-priority stream beside the NEXT iteration's update + cube pass -- it feeds
 * nothing in the loop; `stream` is ordered after everything that produces d_acc4 and the centroids, but NOT
 * after the label map: call kmg_lloyd_flush (or synchronise the device) before reading d_labels.
 * Between two calls the caller may all-reduce d_acc4 on `stream` (sharded images).  Without a bound image it
 * is kmg_lloyd_update + kmg_lloyd_assign_accumulate.                                                  */
KMG_API int kmg_lloyd_iterate(kmg_lloyd *s, const uint8_t *d_rgba, uint64_t n_pixels, uint32_t *d_labels,
                              int64_t *d_acc4, int update_first, void *stream);
/* `stream` waits (on the device, no host synchronisation) for the label passes kmg_lloyd_iterate started. */
KMG_API int kmg_lloyd_flush(kmg_lloyd *s, void *stream);

/* ChooseCentroidModule::compute (core/src/modules.rs:763-840): the whole loop on one device.
 * Expects the centroid table initialised.  Synchronises.  *iterations = the reference's
 * `current_iteration` when the loop stopped.  d_labels (optional) receives the final assignment;
 * the loop applies kmg_lloyd_prepare's cost model itself and, with the colour table, iterates on the
 * sums only and writes the label map once after the last iteration (same result).               */
KMG_API int kmg_lloyd_run(kmg_lloyd *s, const uint8_t *d_rgba, uint64_t n_pixels,
                          uint32_t *d_labels, uint32_t *iterations, void *stream);

/* find_colors / dither_colors (core/src/operations.rs:99-155,215-271; find_centroid.wgsl,
 * swap.wgsl, mix_colors.wgsl main_dither, lab_to_rgb.wgsl) on a row band: `row0` is the image
 * row of the band's first pixel (the Bayer index uses image coordinates).  centroids4 is a
 * HOST table.  Output RGBA8 in d_out_rgba.  mode = replace, dither or meld (mix_colors.wgsl main_meld).  */
KMG_API int kmg_dev_apply(kmg_processor *p, const uint8_t *d_rgba, uint32_t width, uint32_t rows,
                          uint32_t row0, const float *centroids4, uint32_t k, int mode,
                          uint8_t *d_out_rgba, void *stream);

/* The same output pass as a PLAN, for callers that process an image in row bands (a multi-GPU runtime, an image streamed
 * through a pinned double buffer): _create builds everything that depends on the centroid table only -- the device copies of
 * centroids and palette, the dither threshold, the candidate lists / masks or the label tables of the colour cube -- once,
 * asynchronously on `stream`; n_pixels_hint = the pixels the plan is made for (it selects the route exactly as kmg_dev_apply
 * does for a band of that size).  _run launches the per-pixel kernel of one band on any stream (it waits for the tables on the
 * device, never on the host) and returns at once; any number of bands, any order.  _destroy returns the plan's scratch block:
 * the caller has synchronised every stream that ran the plan, or passes synchronise != 0.  kmg_dev_apply = create + run +
 * stream synchronisation + destroy.  (The reference runs the pass on whole textures only: operations.rs:99-155.)              */
KMG_API int kmg_apply_plan_create(kmg_processor *p, const float *centroids4, uint32_t k, int mode, uint64_t n_pixels_hint,
                                  void *stream, kmg_apply_plan **out);
/* The same with an output format (kmg_output_format): kmg_apply_plan_run then writes that format into its d_out_rgba (a
 * uint8_t / uint16_t per pixel for the index formats); kmg_dev_apply_format = kmg_dev_apply with it.  KMG_FORMAT_RGBA8: the
 * calls above, byte for byte.                                                                                             */
KMG_API int kmg_apply_plan_create_format(kmg_processor *p, const float *centroids4, uint32_t k, int mode, int format,
                                         uint64_t n_pixels_hint, void *stream, kmg_apply_plan **out);
KMG_API int kmg_dev_apply_format(kmg_processor *p, const uint8_t *d_rgba, uint32_t width, uint32_t rows, uint32_t row0,
                                 const float *centroids4, uint32_t k, int mode, int format, void *d_out, void *stream);
KMG_API int kmg_apply_plan_run(kmg_apply_plan *plan, const uint8_t *d_rgba, uint32_t width, uint32_t rows, uint32_t row0,
                               uint8_t *d_out_rgba, void *stream);
KMG_API void kmg_apply_plan_destroy(kmg_apply_plan *plan, int synchronise);
/* KMG_MODE_DIFFUSE: waits for the plan's last run and returns KMG_ERR_HIP if any run of the plan timed out (a band that timed
 * out also fails every later kmg_apply_plan_run issued after it completed); KMG_OK for the other modes.                          */
KMG_API int kmg_apply_plan_status(kmg_apply_plan *plan);

/* mix_colors.wgsl:53-67: the dither threshold of a centroid table (host helper).             */
KMG_API int kmg_dither_threshold(const float *centroids4, uint32_t k, float *threshold);

/* ======================= quantisation error statistics, quality-targeted colour count =====
 * How far an output is from its source, as exact integers: every field is a sum or a maximum of integers, so a record does not
 * depend on tiling, order or stream (the rule of the accumulators above).  No counterpart in the reference.
 *  - Counted pixels.  alpha_cutoff t = 0 counts every pixel; t = 1..255 counts a pixel iff the SOURCE's alpha byte is >= t.  The
 *    output's alpha is never read.
 *  - Output side.  KMG_FORMAT_RGBA8: o = the output's R, G, B bytes.  KMG_FORMAT_INDEX8 / INDEX16 with a HOST palette of k x 4
 *    bytes: o = palette[index].  Index k, the transparent slot, is legal on uncounted pixels only: a counted pixel whose index is
 *    >= k adds 1 to `invalid` and nothing to any other field (`pixels` included).
 *  - Lab terms.  q(c) = (rint(64 L), rint(64 a), rint(64 b)) as int32, (L, a, b) = the Lab kmg_dev_rgb_to_lab gives the sRGB8
 *    colour c, rint = round half to even (the product by 64 is exact).  Per pixel dq = q(s) - q(o); the term dqL^2 + dqa^2 + dqb^2
 *    is at most 347 973 309 < 2^29 (from the Lab range of all 2^24 colours), so lab_sse < 2^61 for 2^32 pixels.
 *    mean dE76^2 = lab_sse / (4096 pixels).  (CIE94 is asymmetric and a float: it has no exact sum.)
 *  - Combination.  kmg_dev_compare COMBINES into d_stats as it stands -- sums are added, maxima are maxed (the convention of
 *    kmg_lloyd_accumulate_into) -- so the bands of an image or the frames of a sequence accumulate into one record in any order, on
 *    any streams; the caller clears the record (112 zero bytes) for a fresh measurement.  The fields of a part (KMG_ERROR_RGB,
 *    KMG_ERROR_LAB) that `what` does not request are left alone; pixels, changed and invalid are always combined.
 * The kmg_group_* calls have no error statistics.                                                                            */
#define KMG_ERROR_RGB 1u
#define KMG_ERROR_LAB 2u
typedef struct kmg_error_stats {   /* 14 x uint64_t, no padding */
    uint64_t pixels;      /* counted pixels (those with an invalid index aside)                                  */
    uint64_t changed;     /* counted pixels whose R, G or B differs                                              */
    uint64_t invalid;     /* index formats: counted pixels whose index is >= k (they add nothing else)           */
    uint64_t sse[3];      /* sum (s_c - o_c)^2, c = R, G, B                     [KMG_ERROR_RGB]                  */
    uint64_t sad[3];      /* sum |s_c - o_c|                                    [KMG_ERROR_RGB]                  */
    uint64_t max_abs[3];  /* max |s_c - o_c|                                    [KMG_ERROR_RGB]                  */
    uint64_t lab_sse;     /* sum (dqL^2 + dqa^2 + dqb^2)                        [KMG_ERROR_LAB]                  */
    uint64_t lab_max;     /* max of that per-pixel sum                          [KMG_ERROR_LAB]                  */
} kmg_error_stats;

/* d_src_rgba / d_out: n_pixels (< 2^32) pixels in DEVICE memory (d_out: 4, 1 or 2 bytes per pixel for `format`, INDEX16 2-byte
 * aligned); palette_rgba: HOST, k x 4 bytes, NULL (and k ignored) for KMG_FORMAT_RGBA8 -- it is read before the call returns;
 * d_stats: DEVICE, 8-byte aligned.  Only enqueues work on `stream`.  KMG_ERR_INVALID_ARGUMENT: INDEX8 with k > 256 (k > 255 when
 * alpha_cutoff != 0), k = 0 or k > KMG_MAX_K with an index format, `what` = 0 or with unknown bits, alpha_cutoff > 255.          */
KMG_API int kmg_dev_compare(kmg_processor *p, const uint8_t *d_src_rgba, const void *d_out, uint64_t n_pixels, int format,
                            const uint8_t *palette_rgba, uint32_t k, uint32_t alpha_cutoff, uint32_t what, kmg_error_stats *d_stats,
                            void *stream);
/* The same on HOST buffers, with the processor's alpha_cutoff: uploads both images, OVERWRITES *stats, synchronises.           */
KMG_API int kmg_compare(kmg_processor *p, const uint8_t *src_rgba, const void *out, uint32_t width, uint32_t height, int format,
                        const uint8_t *palette_rgba, uint32_t k, uint32_t what, kmg_error_stats *stats);
/* kmg_reduce_indexed with the colour count chosen by a quality target: as few colours in [k_min, k_max] as keep the mean squared
 * Lab error of the palette step's working image at or below `target` (units of 1/4096 dE76^2).  KMG_ALGO_KMEANS only (the octree
 * is a host algorithm whose colour count is not a monotone knob).
 *   W    = the working image of the palette step: the image after the shrink (kmg_options.shrink_max_dim), then -- alpha mode -- its
 *          kept pixels in raster order (include/kmeans_hip.h at kmg_options); made once per call
 *   C_k  = the centroids the palette pipeline gives W at k (those of kmg_reduce_indexed(k))
 *   E(k) = lab_sse of W against P[label]: label = the KMG_MODE_REPLACE index of each pixel of W under C_k, P = the palette bytes
 *          of the output pass (what kmg_reduce_indexed returns); every pixel of W is counted
 *   k is ACCEPTED iff E(k) <= (uint64_t)target * |W|
 * The search is fixed: evaluate k_max; not accepted: k* = k_max, *reached = 0.  Otherwise lo = k_min, hi = k_max; while lo < hi:
 * mid = (lo + hi) / 2, accepted: hi = mid, else lo = mid + 1; k* = hi, *reached = 1.  At most 1 + ceil(log2(k_max - k_min + 1))
 * palette runs, each a new Lloyd problem on W.  Output (mode, format: the rules of kmg_reduce_indexed, KMG_FORMAT_RGBA8 included;
 * KMG_FORMAT_INDEX8 is checked against k_max), palette and *out_count are byte for byte what kmg_reduce_indexed(k*) writes for
 * the image; out_palette_rgba has room for k_max x 4 bytes.  *achieved (optional) = the RGB and Lab statistics of W at k*;
 * *reached is optional too.  k_min < 1, k_min > k_max or k_max > KMG_MAX_K: KMG_ERR_INVALID_ARGUMENT.
 * The kmg_group_* calls have no counterpart.                                                                                   */
KMG_API int kmg_reduce_quality(kmg_processor *p, const uint8_t *rgba, uint32_t width, uint32_t height, uint32_t k_min, uint32_t k_max,
                               uint32_t target, int mode, int format, uint8_t *out_palette_rgba, uint32_t *out_count, void *out,
                               kmg_error_stats *achieved, int *reached);

/* ---- batched quality targets: a colour count per image in one launch chain -----------------
 * kmg_reduce_quality for many small images (kmg_batch.hip, kmg_batch_apply.hip, kmg_batch_error.hip).  The
 * batched kernels take a colour count PER IMAGE, so one round of every image's search is ONE launch chain: all images that
 * still search, each at its own count.
 *
 * Equivalence.  kmg_reduce_quality_batch gives image i exactly what kmg_reduce_quality of image i alone gives on the same
 * processor: out[i], the palette, out_counts[i], achieved[i], reached[i].  The order of the batch, an image appearing twice,
 * max_resident_bytes and kmg_options.strategy change nothing.  The device calls: kmg_dev_palette_batch_counts gives image i the
 * centroid bits and the iteration count of kmg_lloyd_init_centroids + kmg_lloyd_run + kmg_lloyd_get_centroids at ks[i];
 * kmg_dev_apply_batch_counts the bytes of kmg_dev_apply_format at ks[i]; kmg_dev_compare_batch the record of kmg_dev_compare.
 *
 * The search is kmg_reduce_quality's fixed bisection in lock step (kmg_quality_search.h): round 0 evaluates k_max for every
 * image, round r every image that still searches at its own mid-point; a finished image is in no later launch.  One round: the
 * palette chain with a count per image on the working images W (resident for the whole sub-batch), the labels of W under the
 * resulting tables (the batched output pass: replace, KMG_FORMAT_INDEX16, no cutoff -- W is compacted already), one batched
 * record; acceptance is lab_sse <= (uint64_t)target * |W| per image, on the host.  The final output is the batched output pass
 * at every image's own k* on the full-size sources (meld and diffusion: the per-image pass).  k-means only.
 *
 * Per-image paths inside the call: a working image of 2^19 pixels or more takes kmg_reduce_quality's own search (`fallback`), and
 * so do the images of a sub-batch with fewer than two smaller ones (a batch of one, or max_resident_bytes cutting an image off).
 * max_resident_bytes: as for kmg_reduce_indexed_batch, plus 2 bytes per working pixel for the labels.
 *
 * Refusals, KMG_ERR_INVALID_ARGUMENT, checked for the whole batch before anything is uploaded, in this order: a NULL processor;
 * n_images == 0; a NULL array (achieved and reached may be NULL); then per image in order a NULL entry or a zero side (more than
 * 2^32-1 pixels: KMG_ERR_UNSUPPORTED); k_min < 1, k_min > k_max or k_max > KMG_MAX_K; an unknown mode; an unknown format;
 * KMG_MODE_MELD with an index format; KMG_FORMAT_INDEX8 without room for k_max colours (alpha mode: plus the transparent slot);
 * fixed colours on the processor; alpha weighting on the processor; then, after the shrinks, alpha mode's "image i: no pixel
 * reaches alpha_cutoff", before any output is written.
 * kmg_dev_palette_batch_counts: those of kmg_dev_palette_batch, then per image in order ks[i] == 0 or ks[i] > KMG_MAX_K
 * (KMG_ERR_UNSUPPORTED).  kmg_dev_apply_batch_counts: those of kmg_dev_apply_batch with each image's own count -- a NULL
 * processor, n_images == 0, a NULL array, per image a NULL entry or a zero side; a zero entry of ks; mode; format; an entry of ks
 * above KMG_MAX_K (KMG_ERR_UNSUPPORTED); the rules of the index formats table by table; an INDEX16 output that is not 2-byte
 * aligned.  kmg_dev_compare_batch: a NULL processor; n_images == 0; a NULL array; format; what; alpha_cutoff above 255; an index
 * format without palettes or counts; then per image in order a NULL entry, no pixel, more than 2^32-1 pixels (KMG_ERR_UNSUPPORTED),
 * and for the index formats a count outside 1 .. KMG_MAX_K, no room in INDEX8, an INDEX16 map that is not 2-byte aligned; records
 * that are not 8-byte aligned.                                                                                                    */
typedef struct kmg_batch_quality_report {   /* 32 bytes, no padding */
    uint32_t rounds;            /* rounds of the lock-step search: the most evaluations of any image of a batched search            */
    uint32_t palette_runs;      /* palette chains run, summed over images (the per-image searches included)                         */
    uint32_t launches;          /* kernel launches of the batched palette chains (kmg_batch_report.launches, summed over rounds)    */
    uint32_t measure_launches;  /* launches of the batched error record                                                             */
    uint32_t batched;           /* final output: images written by the batched output launches                                      */
    uint32_t per_image;         /* final output: images written by a per-image output pass                                          */
    uint32_t sub_batches;       /* how many pieces max_resident_bytes cut the batch into                                            */
    uint32_t fallback;          /* working images of 2^19 pixels or more: the per-image search                                      */
} kmg_batch_quality_report;

/* kmg_dev_palette_batch with a colour count per image: ks is a HOST array of n_images counts; centroids4 (HOST) is concatenated,
 * image i's table of ks[i] x 4 floats starts at 4 * (ks[0] + ... + ks[i - 1]) floats.  kmg_dev_palette_batch is the case where all
 * counts are equal.  report->launches: per piece the largest count + 2 + the most iterations.                                    */
KMG_API int kmg_dev_palette_batch_counts(kmg_processor *p, uint32_t n_images, const uint8_t *const *d_rgba, const uint32_t *widths,
                                         const uint32_t *heights, const uint32_t *ks, float *centroids4, uint32_t *iterations,
                                         kmg_batch_report *report, void *stream);
/* kmg_dev_apply_batch with a table per image of its own size: centroids4 concatenated as above.  The images that join go out as
 * at most two chains of launches (those with k < 32 and the others: the chunked scan is a launch's).                            */
KMG_API int kmg_dev_apply_batch_counts(kmg_processor *p, uint32_t n_images, const uint8_t *const *d_rgba, const uint32_t *widths,
                                       const uint32_t *heights, const float *centroids4, const uint32_t *ks, int mode, int format,
                                       void *const *d_out, kmg_batch_apply_report *report, void *stream);
/* kmg_dev_compare for n_images images in one launch: d_src_rgba and d_out are HOST arrays of device pointers, n_pixels a HOST array;
 * palettes_rgba (HOST; index formats) is concatenated, image i's ks[i] x 4 bytes start at 4 * (ks[0] + ... + ks[i - 1]); d_stats:
 * n_images records in device memory.  COMBINES into record i exactly what kmg_dev_compare combines for image i alone (all fields,
 * every `what`, the invalid-index rule).  Enqueues on `stream`; does not synchronise.                                              */
KMG_API int kmg_dev_compare_batch(kmg_processor *p, uint32_t n_images, const uint8_t *const *d_src_rgba, const void *const *d_out,
                                  const uint64_t *n_pixels, int format, const uint8_t *palettes_rgba, const uint32_t *ks,
                                  uint32_t alpha_cutoff, uint32_t what, kmg_error_stats *d_stats, void *stream);
/* host buffers, as kmg_reduce_quality per image: out_palette_rgba[i] has room for k_max * 4 bytes, out_counts[i] receives k*,
 * out[i] has room for widths[i] * heights[i] outputs of `format`; achieved and reached (n_images entries each) may be NULL, and
 * so may report.                                                                                                                  */
KMG_API int kmg_reduce_quality_batch(kmg_processor *p, uint32_t n_images, const uint8_t *const *rgba, const uint32_t *widths,
                                     const uint32_t *heights, uint32_t k_min, uint32_t k_max, uint32_t target, int mode, int format,
                                     uint64_t max_resident_bytes, uint8_t *const *out_palette_rgba, uint32_t *out_counts,
                                     void *const *out, kmg_error_stats *achieved, int *reached, kmg_batch_quality_report *report);

/* ======================= frame sequences: a shared palette, delta frames ==================
 * What an indexed-colour encoder does with many frames (an animation, a sprite sheet, a set of related images): ONE palette for
 * all of them, and per frame the index map of the pixels that changed.  No counterpart in the reference.
 *
 * The working sequence.  For frame i, in the order of the kmg_sequence_add* calls:
 *   S_i = the frame after the shrink of kmg_options.shrink_max_dim, exactly as kmg_palette shrinks it (frames may differ in size)
 *   K_i = the kept pixels of S_i in raster order (kmg_options.alpha_cutoff, read when the add starts; 0: all of them)
 *   W   = K_0 || K_1 || ...
 * The centroids of a sequence are those the default pipeline (initialisation + Lloyd loop: max_iterations, check_period,
 * convergence of the processor) gives W as an image of
 *   (sw, sh) of S_0   when exactly one frame was added and every pixel of it was kept -- kmg_palette / kmg_reduce_indexed of
 *                     that frame, byte for byte;
 *   |W| x 1           otherwise (the rule of alpha mode, see kmg_options: c_0 = W[floor(|W| * 0.5625f)], ties over W's indices).
 * A frame without a kept pixel counts as a frame and adds nothing.  |W| = 0 at _centroids / _palette / _output_begin:
 * KMG_ERR_INVALID_ARGUMENT ("no pixel reaches alpha_cutoff").  An add that would make |W| >= 2^32 is refused with
 * KMG_ERR_UNSUPPORTED and leaves the sequence as it was.  KMG_ALGO_KMEANS only.  _centroids returns the Lloyd loop's order, the
 * one the index maps refer to; _palette converts and sorts as kmg_palette does.  Every call is a new Lloyd problem on W.
 * _add_device reads the frame from DEVICE memory on `stream`; both adds return when W holds the frame (they synchronise).
 * _clear empties W and the frame count; _info: out[0] = frames added, out[1] = |W|.
 *
 * A kmg_sequence is NOT re-entrant: one thread at a time per sequence, any number of sequences per processor (each has its own
 * stream and blocks).  The processor outlives its sequences.                                                                   */
typedef struct kmg_sequence kmg_sequence;
KMG_API int kmg_sequence_create(kmg_processor *p, kmg_sequence **out);
KMG_API void kmg_sequence_destroy(kmg_sequence *s);
KMG_API int kmg_sequence_add(kmg_sequence *s, const uint8_t *rgba, uint32_t width, uint32_t height);
KMG_API int kmg_sequence_add_device(kmg_sequence *s, const uint8_t *d_rgba, uint32_t width, uint32_t height, void *stream);
KMG_API int kmg_sequence_clear(kmg_sequence *s);
KMG_API int kmg_sequence_info(kmg_sequence *s, uint64_t out[2]);
KMG_API int kmg_sequence_centroids(kmg_sequence *s, uint32_t k, float *centroids4);
KMG_API int kmg_sequence_palette(kmg_sequence *s, uint32_t k, uint8_t *out_rgba, uint32_t *out_count);

/* The delta pass: an index map against the canvas of what is shown.  For the pixel (x, row0 + r) of the band, c = its index in
 * d_index, v = its index in d_canvas:
 *   c == v:   delta = k                 (the transparent slot: "over" blending keeps what is shown)
 *   c != v:   delta = c, changed += 1, the box takes in (x, row0 + r), and cleared += 1 when c == k
 *   always:   canvas = c
 * All integers, no order: the pass COMBINES into *d_info as it stands -- the two sums are added, x0 / y0 are minned, x1 / y1 are
 * maxed (the convention of kmg_dev_compare) -- so the bands of one frame may run in any order, on any streams, and end in the same
 * record.  The caller writes the fresh record {0, 0, 0xFFFFFFFF, 0xFFFFFFFF, 0, 0} before a frame; a record that is still fresh
 * afterwards (changed = 0) has no box.  cleared > 0 means a pixel that showed a colour turns transparent: a delta map cannot
 * express that under "over" blending, the frame has to be sent in full.
 * d_index, d_canvas, d_delta: DEVICE, width * rows (< 2^32) elements of `format` each, tightly packed, aligned to their element
 * only (the 16-byte accesses of the pass need the three pointers at one offset within 16 bytes; otherwise it goes element by
 * element); d_delta overlaps neither of the others.  d_info: DEVICE, 8-byte aligned.  KMG_FORMAT_INDEX8 needs k <= 255 (slot k
 * must fit), KMG_FORMAT_INDEX16 takes any k <= KMG_MAX_K; KMG_FORMAT_RGBA8, k = 0, zero width or rows, a NULL pointer:
 * KMG_ERR_INVALID_ARGUMENT.  Indices above k are compared like any other.  Only enqueues work on `stream`.                      */
typedef struct kmg_frame_delta {      /* 32 bytes, no padding */
    uint64_t changed;                 /* pixels whose index differs from the canvas                                */
    uint64_t cleared;                 /* of those: the frame's index is the transparent slot k                     */
    uint32_t x0, y0;                  /* min x, min y of the changed pixels   (fresh record: 0xFFFFFFFF)           */
    uint32_t x1, y1;                  /* max x + 1, max y + 1                 (fresh record: 0)                    */
} kmg_frame_delta;
KMG_API int kmg_dev_frame_delta(kmg_processor *p, const void *d_index, void *d_canvas, uint32_t width, uint32_t rows, uint32_t row0,
                                int format, uint32_t k, void *d_delta, kmg_frame_delta *d_info, void *stream);

/* The lossy delta pass: a pixel whose source moved within a tolerance keeps the index it shows.  Real input (sensor noise, video
 * compression artefacts, dithered or diffused maps) changes nearly every index from frame to frame even when the scene is still;
 * the exact rule above then sends the whole frame.  A second per-pixel state joins the canvas: the HELD SOURCE h, the RGBA8
 * source word the pixel had when its canvas index was last written.  It is the anchor of the comparison -- never the previous
 * frame -- so a slow drift cannot accumulate: once the source has moved more than the tolerance from the anchor, the pixel is sent.
 *   D(x, y) = dqL^2 + dqa^2 + dqb^2,  dq = q(x) - q(y) over the R, G, B bytes, q = rint(64 Lab): the grid of kmg_error_stats.
 *             An exact integer, at most 347 973 309, in units of 1/4096 dE76^2 (those of kmg_reduce_quality's target); D = 0 when
 *             the R, G, B bytes are equal (no conversion is made then).  `tolerance` is in the same unit.
 * For the pixel (x, row0 + r) of the band, s = its source word, c = its index in d_index, v = its index in d_canvas, h = its held
 * source:
 *   hold := v != k  &&  c != k  &&  D(s, h) <= tolerance
 *   hold:      delta = k; canvas and held source stay; when c != v: held += 1, held_sse += D(s, h)
 *   not hold:  the exact rule of kmg_dev_frame_delta (c == v: delta = k; c != v: delta = c, changed += 1, the box takes the pixel
 *              in, cleared += 1 when c == k); canvas = c; held source = s
 * A pixel that shows nothing (v == k) is never held, nor is one that turns transparent (c == k).  tolerance = 0 holds only where
 * D = 0.  After any frame every pixel of the canvas either equals this frame's exact index or shows the exact index of an earlier
 * frame whose source at that pixel is within `tolerance` of this frame's.
 * The record starts with the fields of kmg_frame_delta (same fresh values, same combination rule); held and held_sse are sums:
 * fresh 0, combined by addition (held_sse < 2^61 for 2^32 pixels).  Bands may run in any order on any streams, as above.
 * d_src_rgba, d_held_rgba: DEVICE, width * rows RGBA8 words each, 4-byte aligned; the index buffers as for kmg_dev_frame_delta.
 * The 16-byte accesses of the pass need the two RGBA8 buffers 16-byte aligned and the three index buffers 4- (INDEX8) or 8-byte
 * (INDEX16) aligned; otherwise it goes pixel by pixel.  No two buffers overlap.  Refusals: those of kmg_dev_frame_delta, and a NULL
 * or misaligned source or held pointer.  Only enqueues work on `stream`.                                                        */
typedef struct kmg_frame_hold {       /* 48 bytes, no padding */
    uint64_t changed;                 /* as kmg_frame_delta: pixels sent                                            */
    uint64_t cleared;
    uint32_t x0, y0;
    uint32_t x1, y1;
    uint64_t held;                    /* pixels whose exact index differs from the canvas and that were held        */
    uint64_t held_sse;                /* sum of D(s, h) over those pixels                                           */
} kmg_frame_hold;
KMG_API int kmg_dev_frame_delta_lossy(kmg_processor *p, const uint8_t *d_src_rgba, const void *d_index, void *d_canvas,
                                      uint8_t *d_held_rgba, uint32_t width, uint32_t rows, uint32_t row0, int format, uint32_t k,
                                      uint32_t tolerance, void *d_delta, kmg_frame_hold *d_info, void *stream);

/* All frames of a clip through the delta pass in one launch chain.  The outputs, the records, the canvas and the held source are
 * exactly what n_frames calls of kmg_dev_frame_delta (tolerances == NULL) or of kmg_dev_frame_delta_lossy (frame t at
 * tolerances[t]) leave, in order, each on the whole frame with row0 = 0 -- but a lane keeps its pixels' canvas index and held
 * source in registers across the frames, so that state crosses the memory bus once per KMG_CLIP_FRAMES frames instead of once
 * per frame (a longer clip runs as several launches over the same pixels).
 *   d_src_rgba, d_index, d_out: HOST arrays of n_frames DEVICE pointers: the frames' sources (NULL when tolerances == NULL), their
 *   maps I_t, and where delta map t goes.  d_canvas, d_held_rgba: as for the two passes; d_held_rgba may be NULL when tolerances ==
 *   NULL.  An exact clip writes only the first 32 bytes of each record and updates the held source only when d_held_rgba and the
 *   sources are both given: it then is the last frame.  tolerances: HOST, n_frames words.  d_info: DEVICE, n_frames records of 48
 *   bytes, combined into as they stand.  The table of pointers goes to the device in one stream-ordered copy; the arrays may change
 *   as soon as the call returns.
 *   KMG_CLIP_FULL_ON_CLEAR: a frame whose own record has cleared > 0 follows the rule of kmg_sequence_output_frame_lossy: d_out[t]
 *   = I_t, d_full[t] = 1 (every other word of d_full: 0), and after it the canvas equals I_t and the held source the frame at every
 *   pixel; the record stays as measured; every later frame sees that state.  Which frames those are follows from the maps alone:
 *   after any frame the canvas shows slot k exactly where that frame's map does, so frame t >= 1 clears a pixel exactly when some
 *   pixel has I_t == k and I_{t-1} != k (frame 0: the canvas in place of I_{t-1}).  d_full: DEVICE, n_frames words, 4-byte aligned;
 *   may be NULL without the flag, and is not touched then.
 * Pointer rules: those of the two passes, frame by frame, and across the frames: a lane has the next frame's source and map in
 * flight while it stores this frame's delta map, so no buffer that is written (any d_out[t], the canvas, the held source, the
 * records, d_full) may overlap any other buffer of any frame; the sources and maps, which are only read, may overlap each other
 * (the same map may serve two frames).  As in the two passes, no overlap is checked.  No alignment beyond the element's (RGBA8: 4 bytes) is required -- each
 * buffer whose pointer does not allow the vector access goes element by element.  Indices above k are compared like any other.
 * Refusals, in this order: those of kmg_dev_frame_delta_lossy (RGBA8, format, k, a NULL pointer -- the arrays, the canvas, the
 * records, and for a lossy clip the held source --, the size, a misaligned canvas, held source or record); n_frames == 0; a NULL
 * or misaligned entry of an array; unknown flags; KMG_CLIP_FULL_ON_CLEAR without d_full.  Only enqueues work on `stream`.        */
#define KMG_CLIP_FULL_ON_CLEAR 1u
#define KMG_CLIP_FRAMES 32u            /* frames one launch of the walk takes */
#define KMG_CLIP_MIN_FRAMES 8u         /* the shortest clip kmg_sequence_output_frames sends through the launch chain */
KMG_API int kmg_dev_frame_delta_clip(kmg_processor *p, uint32_t n_frames, const uint8_t *const *d_src_rgba, const void *const *d_index,
                                     void *d_canvas, uint8_t *d_held_rgba, uint32_t width, uint32_t height, int format, uint32_t k,
                                     const uint32_t *tolerances, uint32_t flags, void *const *d_out, kmg_frame_hold *d_info,
                                     uint32_t *d_full, void *stream);

/* Frame output with the sequence's palette, on HOST buffers.
 *   _output_begin   the centroids of W at k (as _centroids); out_palette_rgba (k x 4 bytes) / *out_count: the palette in index
 *                   order, exactly as kmg_reduce_indexed returns it; one apply plan (kmg_apply_plan_create_format with
 *                   n_pixels_hint = width * height, the processor's alpha_cutoff as it is now), the frame buffers and a canvas
 *                   filled with k.  Mode and format: the rules of the index formats (meld has no index; KMG_FORMAT_INDEX8 needs
 *                   k <= 255 here, alpha mode or not: the canvas uses slot k).  KMG_FORMAT_RGBA8 takes every mode, but no delta.
 *                   A second _begin ends the first.
 *   _output_frame   rgba: a frame of width x height.  Without KMG_FRAME_DELTA: out = I_t, the full map -- byte for byte what
 *                   kmg_dev_apply_format writes for the frame with these centroids; each frame is an image of its own (row0 = 0:
 *                   Bayer coordinates and diffusion start over); info and is_full are optional (a fresh record, 1); the canvas
 *                   becomes I_t.  With KMG_FRAME_DELTA: out = the delta map of I_t against the canvas, *info = its record,
 *                   *is_full = 0 -- unless info->cleared > 0: then out = I_t and *is_full = 1, *info as measured.  The first
 *                   frame needs no special case: against a canvas of k the delta IS I_0.  Replaying the delta maps with "over"
 *                   (index k keeps the pixel) and the full maps with "source" reproduces every I_t.
 *                   No output open, KMG_FRAME_DELTA with KMG_FORMAT_RGBA8 or without info / is_full: KMG_ERR_INVALID_ARGUMENT.
 *   _output_frame_lossy   the same with the rule of kmg_dev_frame_delta_lossy at `tolerance`: out = the lossy delta map, *info = its
 *                   record, *is_full = 0 -- unless info->cleared > 0: then out = I_t, *is_full = 1, *info as measured, and the
 *                   canvas becomes I_t with the frame as every pixel's held source.  An exact frame (_output_frame, delta or
 *                   full) leaves the canvas equal to its map everywhere, so its held source is that frame: exact and lossy
 *                   frames may alternate freely on one open output.  Needs KMG_FRAME_DELTA in flags, an index format, info and
 *                   is_full: otherwise KMG_ERR_INVALID_ARGUMENT.  Replaying its maps as above reproduces the canvas.
 *   _output_end     returns the plan and the buffers; so does _destroy.
 * Frames may be added while an output is open: they do not affect it.                                                         */
#define KMG_FRAME_DELTA 1u
KMG_API int kmg_sequence_output_begin(kmg_sequence *s, uint32_t k, int mode, int format, uint32_t width, uint32_t height,
                                      uint8_t *out_palette_rgba, uint32_t *out_count);
KMG_API int kmg_sequence_output_frame(kmg_sequence *s, const uint8_t *rgba, uint32_t flags, void *out, kmg_frame_delta *info,
                                      int *is_full);
KMG_API int kmg_sequence_output_frame_lossy(kmg_sequence *s, const uint8_t *rgba, uint32_t flags, uint32_t tolerance, void *out,
                                            kmg_frame_hold *info, int *is_full);
KMG_API int kmg_sequence_output_end(kmg_sequence *s);

/* A whole clip through the open output: out[t], info[t] and is_full[t] are exactly what frame t gets from _output_frame (tolerances
 * == NULL) or _output_frame_lossy (at tolerances[t]) called one after another, and the output is left in the same state (canvas
 * and held source), so clips and single frames alternate freely.  The frames are staged in one block, their maps come from the
 * batched output launch where they can join it (kmg_dev_apply_batch's rule, with the plan's alpha cutoff) and from a pass of their
 * own otherwise (every diffuse frame), the delta maps from kmg_dev_frame_delta_clip, the records come back in one copy.  Without
 * KMG_FRAME_DELTA (every RGBA8 clip) the call writes the full maps; the canvas becomes the last map, the held source the last
 * frame; info and is_full are optional.  info: n_frames records of kmg_frame_hold -- an exact clip leaves held = held_sse = 0.
 * max_resident_bytes: the clip is cut (kmg_reduce_batch's rule) over the 4 + 2e bytes per pixel a frame keeps on the device, e the
 * bytes of an index; 0 = no bound of the caller's.  A clip of fewer than KMG_CLIP_MIN_FRAMES frames -- where the chain was measured
 * not to pay: profiles/r12_clip_time.txt, two frames of 256 x 256 take up to 1.63 of the per-frame calls, eight at most 0.80 -- is that
 * many _output_frame calls: nothing is staged, max_resident_bytes has nothing to cut, and the report says launches = batched = 0,
 * per_image = n_frames, sub_clips = 1.  report: optional.
 * Refusals, in this order, for the whole clip before anything is uploaded: those of _output_frame / _output_frame_lossy (no
 * sequence, a local output, no open output, a NULL rgba or out array, unknown flags, a lossy clip without KMG_FRAME_DELTA,
 * KMG_FRAME_DELTA with RGBA8 or without info / is_full), n_frames == 0, a NULL entry.  A refused call leaves the output untouched.
 * Any later failure, on the chain or in one of a short clip's frames, ENDS the open output, as a second _begin does: no half-updated
 * canvas can be used.                          */
typedef struct kmg_clip_report {   /* 16 bytes, no padding */
    uint32_t launches;    /* launches of the batched output kernel and of the two clip kernels */
    uint32_t batched;     /* frames whose map came from the batched output launch              */
    uint32_t per_image;   /* frames whose map took its own output pass                         */
    uint32_t sub_clips;   /* pieces max_resident_bytes cut the clip into                       */
} kmg_clip_report;
KMG_API int kmg_sequence_output_frames(kmg_sequence *s, uint32_t n_frames, const uint8_t *const *rgba, uint32_t flags,
                                       const uint32_t *tolerances, uint64_t max_resident_bytes, void *const *out, kmg_frame_hold *info,
                                       int *is_full, kmg_clip_report *report);

/* ======================= per-frame palettes: colour-keyed delta frames =====================
 * One palette for all frames is what limits a 256-entry format on a clip whose content changes (a cut, a pan, a fade); GIF has
 * local colour tables for that.  Once entry 7 of frame t is another colour than entry 7 of frame t - 1, comparing indices means
 * nothing: the canvas has to hold what is SHOWN, and the comparison goes through the frame's palette.  No counterpart in the
 * reference.
 *
 * The colour-keyed delta pass.  State per pixel: shown, an RGBA8 word -- what the viewer shows; the word 0 means nothing is shown
 * -- and, in the lossy form, the held source of kmg_dev_frame_delta_lossy.  For the pixel (x, row0 + r) of the band:
 *   c = its index in d_index;  p = P[c] as a 32-bit word when c < k, else 0 (an index >= k shows nothing; indices above k are
 *   treated as k);  v = its word in d_shown.
 * Exact rule:
 *   p == v:   delta = k
 *   p != v:   delta = c (k when c > k), changed += 1, the box takes the pixel in, cleared += 1 when p == 0
 *   always:   shown = p
 * Lossy rule, s = the source word, h = the held source, D and `tolerance` exactly as at kmg_dev_frame_delta_lossy:
 *   hold := v != 0  &&  p != 0  &&  D(s, h) <= tolerance
 *   hold:      delta = k; shown and held stay; when p != v: held += 1, held_sse += D(s, h)
 *   not hold:  the exact rule; shown = p; held = s
 * The records are kmg_frame_delta (exact) and kmg_frame_hold (lossy), unchanged: same fresh values, same combination rule (sums
 * added, minima minned, maxima maxed), so the bands of a frame may run in any order on any streams.
 * Two consequences:
 *   same palette       with one palette whose entries are distinct and non-zero, and indices <= k, the exact pass writes the delta
 *                      map and the record of kmg_dev_frame_delta (the lossy one those of kmg_dev_frame_delta_lossy); afterwards
 *                      shown == P'[canvas] with P'[k] = 0.
 *   duplicate entries  a pixel whose index changes between two entries with equal bytes is NOT sent (the index pass would send it).
 * d_palette_rgba: DEVICE, k words, 4-byte aligned, read when the pass runs.  d_shown_rgba (and d_src_rgba, d_held_rgba): DEVICE,
 * width * rows RGBA8 words, 4-byte aligned.  d_index, d_delta, formats and refusals: those of kmg_dev_frame_delta / _lossy
 * (KMG_FORMAT_INDEX8 needs k <= 255, KMG_FORMAT_INDEX16 takes k <= KMG_MAX_K); a NULL or misaligned palette or shown pointer is
 * refused as well.  The pass takes its vector route -- 16-byte accesses of the RGBA8 buffers, 4- / 8-byte accesses of the index
 * buffers -- when d_shown_rgba (lossy: also d_src_rgba and d_held_rgba) is 16-byte aligned and d_index and d_delta are 4- (INDEX8)
 * or 8-byte (INDEX16) aligned; otherwise it goes pixel by pixel, correct but not fast.  No two buffers overlap.  Both only enqueue
 * work on `stream`.                                                                                                            */
KMG_API int kmg_dev_frame_delta_colour(kmg_processor *p, const void *d_index, const uint8_t *d_palette_rgba, uint8_t *d_shown_rgba,
                                       uint32_t width, uint32_t rows, uint32_t row0, int format, uint32_t k, void *d_delta,
                                       kmg_frame_delta *d_info, void *stream);
KMG_API int kmg_dev_frame_delta_colour_lossy(kmg_processor *p, const uint8_t *d_src_rgba, const void *d_index,
                                             const uint8_t *d_palette_rgba, uint8_t *d_shown_rgba, uint8_t *d_held_rgba, uint32_t width,
                                             uint32_t rows, uint32_t row0, int format, uint32_t k, uint32_t tolerance, void *d_delta,
                                             kmg_frame_hold *d_info, void *stream);

/* Frame output with a palette per frame, on HOST buffers.
 *   _output_begin_local   needs no added frame (W is not used).  Takes the frame buffers, a shown canvas filled with 0, the held
 *                   source, the palette and the record.  Mode and format: the rules of _output_begin for delta frames -- index
 *                   formats only, no meld, KMG_FORMAT_INDEX8 needs k <= 255.  flags: 0 or KMG_LOCAL_WARM.  A second begin of
 *                   either kind ends the first; _output_end and _destroy end either kind.  _output_frame / _output_frame_lossy
 *                   on a local output, and _output_frame_local on a shared one, are refused with KMG_ERR_INVALID_ARGUMENT; the
 *                   output stays open.
 *   _output_frame_local   rgba: a frame of width x height.  Its centroids C_t:
 *                     cold   (flags of the begin 0; the first frame; the frame after one whose palette step failed)  C_t, the palette
 *                            bytes in index order and the full map I_t are those of kmg_reduce_indexed(frame, k, KMG_ALGO_KMEANS, mode)
 *                            byte for byte; alpha cutoff and fixed colours are read when the call starts.
 *                     warm   (KMG_LOCAL_WARM, every later frame)  the processor's Lloyd loop on the frame's working image -- the
 *                            one cold would use -- started from all k of C_{t-1} (kmg_lloyd_init_centroids_seeded with
 *                            n_seeds = k: no farthest-point pick); palette bytes and I_t from the usual output pass with C_t.  A
 *                            frame of a warm output while the processor has fixed colours: KMG_ERR_UNSUPPORTED.
 *                   A call refused before any work is enqueued changes nothing, not even whether the next frame is warm.  Such
 *                   calls are: bad arguments, fixed colours on a warm output, k below the fixed colours.  A frame that fails in
 *                   its palette step (for example "no pixel reaches alpha_cutoff") returns that status, leaves shown and held as
 *                   they were and makes the next frame cold.
 *                   out_palette_rgba (k x 4 bytes) / *out_count: P_t.  Without KMG_FRAME_DELTA in `flags`: out = I_t,
 *                   *is_full = 1, *info fresh.  With it: out = the delta map of (I_t, P_t) against shown -- the exact rule when
 *                   `tolerance` is NULL, else the lossy rule at *tolerance -- and *is_full = 0; unless info->cleared > 0: then
 *                   out = I_t, *is_full = 1, *info as measured.  After every full frame shown = P_t[I_t] and every pixel's held
 *                   source is this frame; exact and lossy frames alternate freely.  The exact form fills the first 32 bytes of
 *                   *info and leaves held = held_sse = 0.  A tolerance without KMG_FRAME_DELTA, unknown flags, a NULL pointer
 *                   other than `tolerance`: KMG_ERR_INVALID_ARGUMENT.
 * Replay: decode each coded frame through ITS OWN palette, compose delta maps "over" (index k keeps the pixel) and full maps as
 * "source".  For exact frames this gives P_t[I_t]; for lossy frames it gives the shown canvas.                                  */
#define KMG_LOCAL_WARM 1u
KMG_API int kmg_sequence_output_begin_local(kmg_sequence *s, uint32_t k, int mode, int format, uint32_t width, uint32_t height,
                                            uint32_t flags);
KMG_API int kmg_sequence_output_frame_local(kmg_sequence *s, const uint8_t *rgba, uint32_t flags, const uint32_t *tolerance, void *out,
                                            uint8_t *out_palette_rgba, uint32_t *out_count, kmg_frame_hold *info, int *is_full);

/* ======================= index-map optimisation: usage counts, palette pruning, packed maps ===
 * The last step before a PNG8 / GIF / APNG writer: which palette entries a map uses, a palette without the unused ones in the
 * order a writer wants, and the map rewritten for it at 1, 2, 4, 8 or 16 bits per pixel.  All integers.  No counterpart in the
 * reference.  Three building blocks -- count (device), plan (host), rewrite (device) -- and host-buffer calls over them.
 *
 * The usage record of a map with k colours is k + 2 uint64_t:
 *   usage[i], i < k   pixels with index i
 *   usage[k]          pixels with index k: the transparent slot of alpha mode, the "keep what is shown" value of delta maps
 *   usage[k + 1]      pixels with an index above k (the `invalid` of kmg_error_stats)
 * kmg_dev_index_usage COMBINES (adds) into d_usage as it stands -- the convention of kmg_dev_compare -- so the bands of a frame and
 * the frames of a sequence, in any order, on any streams, end in the same record; the caller zeroes a fresh record.  d_index:
 * DEVICE, n_pixels (< 2^32) elements of `format`, aligned to its element (a 4-element-aligned pointer allows the vector loads);
 * d_usage: DEVICE, k + 2 entries, 8-byte aligned.  KMG_FORMAT_INDEX8 takes k <= 256 -- at k = 256 no byte can be slot k or above:
 * usage[256] and usage[257] stay as they were -- KMG_FORMAT_INDEX16 any k <= KMG_MAX_K.  KMG_ERR_INVALID_ARGUMENT, nothing
 * enqueued: KMG_FORMAT_RGBA8, k = 0 or above the format's limit, n_pixels = 0, a NULL pointer, a misaligned INDEX16 map or
 * record.  Only enqueues work on `stream`.                                                                                  */
KMG_API int kmg_dev_index_usage(kmg_processor *p, const void *d_index, uint64_t n_pixels, int format, uint32_t k, uint64_t *d_usage,
                                void *stream);

/* The plan: host arithmetic on a usage record and the palette it counts, no processor, no device.
 *   kept colours   the entries i < k with usage[i] > 0; with KMG_INDEX_KEEP_UNUSED every i < k
 *   their order    the low two bits of `flags`: KMG_INDEX_ORDER_KEEP ascending old index (fixed colours keep their relative
 *                  order); _USAGE descending usage; _LUMA ascending 2126 R + 7152 G + 722 B of the palette bytes; ties by
 *                  ascending old index
 *   the slot       the transparent slot is present iff usage[k] > 0 or KMG_INDEX_KEEP_TRANSPARENT is set.  With
 *                  KMG_INDEX_TRANSPARENT_FIRST it is new index 0 and the colours follow from 1 (a PNG tRNS chunk is then one
 *                  byte); otherwise it is new index n_colors.  info->transparent = its new index, -1 when absent
 *   n_slots        n_colors + (present ? 1 : 0); bits = the smallest of 1, 2, 4, 8, 16 with 2^bits >= n_slots
 *   remap[old]     old = 0 .. k: the new index, 0xFFFF for a dropped entry
 *   out_palette    [new] = the four palette bytes of the colour, (0, 0, 0, 0) for the transparent slot: n_slots x 4 bytes are
 *                  written (PLTE + tRNS material as it stands); room for (k + 1) x 4; it may be `palette_rgba` itself
 * ORDER_KEEP | KEEP_UNUSED | KEEP_TRANSPARENT without TRANSPARENT_FIRST is the identity: remap[i] = i for i <= k.
 * KMG_ERR_INVALID_ARGUMENT, nothing written: usage[k + 1] != 0 ("the map holds indices above k"); n_slots = 0 (an all-zero
 * record without the keep flags); unknown flag bits or order value 3; k = 0 or k > KMG_MAX_K; a NULL pointer.                */
#define KMG_INDEX_ORDER_KEEP        0u
#define KMG_INDEX_ORDER_USAGE       1u
#define KMG_INDEX_ORDER_LUMA        2u
#define KMG_INDEX_KEEP_UNUSED       4u
#define KMG_INDEX_KEEP_TRANSPARENT  8u
#define KMG_INDEX_TRANSPARENT_FIRST 16u
typedef struct kmg_index_plan_info {  /* 16 bytes, no padding */
    uint32_t n_colors;                /* kept colours                                                              */
    uint32_t n_slots;                 /* n_colors, plus 1 when the transparent slot is present                     */
    int32_t transparent;              /* the slot's new index, -1 when absent                                      */
    uint32_t bits;                    /* 1, 2, 4, 8 or 16: what an index of n_slots needs                          */
} kmg_index_plan_info;
KMG_API int kmg_index_plan(const uint64_t *usage, const uint8_t *palette_rgba, uint32_t k, uint32_t flags, uint16_t *remap,
                           uint8_t *out_palette_rgba, kmg_index_plan_info *info);

/* Rewrite and pack: d_out = remap[d_in] at out_bits per pixel.
 *   out_bits 8, 16     one uint8_t / uint16_t per pixel, rows contiguous: the layouts of KMG_FORMAT_INDEX8 / INDEX16; narrowing
 *                      16 -> 8 and widening 8 -> 16 are both allowed
 *   out_bits 1, 2, 4   packed rows as PNG stores them (a filter-0 scanline without its filter byte): every row starts on a byte,
 *                      the stride is ceil(width * out_bits / 8), the leftmost pixel sits in the high bits, the padding bits of a
 *                      row's last byte are zero
 * A pixel is BAD if its index is above k, its remap entry is 0xFFFF, or its new index does not fit out_bits: it is written as 0
 * and counted; the pass COMBINES (adds) the count into *d_bad.  d_in: DEVICE, width * rows (< 2^32) elements of in_format;
 * remap: HOST, k + 1 entries, read before the call returns; d_out: DEVICE, 2-byte aligned for out_bits = 16; d_bad: DEVICE,
 * 8-byte aligned.  d_out == d_in is allowed when out_bits equals the input's own width; otherwise the buffers must not overlap.
 * Refusals: those of kmg_dev_index_usage, and out_bits outside {1, 2, 4, 8, 16}, zero width, zero rows.  Only enqueues work on
 * `stream`.                                                                                                                 */
KMG_API int kmg_dev_index_remap(kmg_processor *p, const void *d_in, int in_format, uint32_t width, uint32_t rows, uint32_t k,
                                const uint16_t *remap, uint32_t out_bits, void *d_out, uint64_t *d_bad, void *stream);

/* The same on HOST buffers; each uploads, runs and synchronises.
 *   kmg_index_usage     COMBINES into the host record `usage` (k + 2 entries) as it stands
 *   kmg_index_remap     out: ceil(width * out_bits / 8) * height bytes (1, 2 or width * height elements for 8 / 16);
 *                       *bad (optional) = the number of bad pixels (overwritten)
 *   kmg_index_optimize  one upload, usage, plan with `flags`, remap, download.  out_bits = 0 takes the plan's bits; a non-zero
 *                       out_bits below them, and bits (given or the plan's) above the input map's own width, are
 *                       KMG_ERR_INVALID_ARGUMENT, so out_map needs no more room than the input map.  out_palette_rgba: room for
 *                       (k + 1) x 4 bytes, n_slots x 4 written; *info: the plan's; the refusals of kmg_index_plan apply.          */
KMG_API int kmg_index_usage(kmg_processor *p, const void *index, int format, uint64_t n_pixels, uint32_t k, uint64_t *usage);
KMG_API int kmg_index_remap(kmg_processor *p, const void *in, int in_format, uint32_t width, uint32_t height, uint32_t k,
                            const uint16_t *remap, uint32_t out_bits, void *out, uint64_t *bad);
KMG_API int kmg_index_optimize(kmg_processor *p, const void *index, int format, uint32_t width, uint32_t height,
                               const uint8_t *palette_rgba, uint32_t k, uint32_t flags, uint32_t out_bits, uint8_t *out_palette_rgba,
                               kmg_index_plan_info *info, void *out_map);

/* ======================= several GPUs: a group of devices ================================
 * ImageProcessor::new (core/src/lib.rs:38-65) picks ONE adapter; the reference has no multi-device path.  A kmg_group is the
 * same constructor over a device LIST: one kmg_processor, one compute stream and one RCCL communicator rank per device.
 * RCCL is loaded at run time (dlopen of librccl.so.1 -- the copy a host process already maps, e.g. PyTorch's, is reused),
 * so a single-GPU host needs no RCCL at all.  The path's one exchange step is ncclAllReduce(sum) of the
 * k x 4 int64 accumulators over xGMI between the assign pass and the centroid update; because the sums are exact integers,
 * centroids and labels are bit-identical for any number of devices.
 *
 *   one process, n devices   kmg_group_create: ncclCommInitAll, one worker thread per device inside the library; the
 *                            host-buffer calls kmg_group_{palette, find, reduce} tile one image in row bands (device g of G
 *                            owns rows [g H / G, (g + 1) H / G)), kmg_group_reduce_batch places whole images (BASELINE
 *                            config 4: no collective at all).
 *   one process per GPU      rank 0 calls kmg_group_unique_id, the host runtime hands the 128 bytes to every process (MPI,
 *                            a file, torch.distributed ...), each calls kmg_group_create_rank(first_rank = its rank): the
 *                            kmg_group_lloyd_* calls then drive THIS process's band(s) of the sharded image.
 * Ranks are numbered first_rank + i for the group's local device i; `world` = ranks over all processes.
 *
 * Failures.  A call that issues no collective (kmg_group_find, kmg_group_reduce_batch, kmg_group_palette / _reduce unless the
 * k-means itself runs sharded) fails like its single-device counterpart: the error is returned, the group stays usable.  A rank
 * that fails where a collective may be in flight (kmg_group_lloyd_*, the sharded full-resolution k-means) would leave its peers
 * waiting inside RCCL for ever, so the communicators of this process are aborted (ncclCommAbort) and the group is BROKEN: every
 * later call on it returns KMG_ERR_HIP at once; destroy it and create a new one (the other processes of a multi-process world
 * see their own collectives fail or time out and must do the same).  No C++ exception crosses this ABI: std::bad_alloc comes
 * back as KMG_ERR_OUT_OF_MEMORY, anything else as KMG_ERR_HIP with the text in kmg_last_error().                              */
#define KMG_MAX_DEVICES 16
#define KMG_UNIQUE_ID_BYTES 128
/* kmg_group_options.flags */
#define KMG_GROUP_FORCE_COLLECTIVES 1u /* issue every collective even in a world of ONE rank (a one-GPU box then drives the
                                          RCCL calls exactly as a multi-rank job does: tests)                              */
#define KMG_GROUP_LOOPBACK          2u /* exchange through this process's device memory instead of RCCL; the device list may
                                          then name a device more than once (RCCL refuses two ranks on one device) -- the
                                          multi-rank code path on a one-GPU box (tests); one process only                  */
typedef struct kmg_group_options {
    uint32_t struct_size;               /* sizeof(kmg_group_options)                                                    */
    uint32_t n_devices;                 /* 0 = every visible HIP device, in ordinal order                               */
    int32_t  devices[KMG_MAX_DEVICES];  /* HIP device ordinals of the n_devices local ranks                             */
    uint32_t flags;                     /* KMG_GROUP_*                                                                  */
    kmg_options processor;              /* options of every member processor (its `device` field is ignored)            */
} kmg_group_options;

typedef struct kmg_group kmg_group;
typedef struct kmg_group_lloyd kmg_group_lloyd;

KMG_API void kmg_default_group_options(kmg_group_options *opt);
KMG_API int kmg_group_create(const kmg_group_options *opt, kmg_group **out);
KMG_API int kmg_group_unique_id(uint8_t id[KMG_UNIQUE_ID_BYTES]);
KMG_API int kmg_group_create_rank(const kmg_group_options *opt, const uint8_t id[KMG_UNIQUE_ID_BYTES], uint32_t first_rank,
                                  uint32_t world, kmg_group **out);
KMG_API void kmg_group_destroy(kmg_group *g);
/* n_local = devices of this process, first_rank / world as above, rccl_version = ncclGetVersion() or 0 when RCCL was not
 * needed (one rank without KMG_GROUP_FORCE_COLLECTIVES, or KMG_GROUP_LOOPBACK).  Any out pointer may be NULL.            */
KMG_API int kmg_group_info(kmg_group *g, uint32_t *n_local, uint32_t *first_rank, uint32_t *world, int *rccl_version);
/* local device i's processor / compute stream (hipStream_t): everything the group enqueues for that device runs on it   */
KMG_API kmg_processor *kmg_group_processor(kmg_group *g, uint32_t i);
KMG_API void *kmg_group_stream(kmg_group *g, uint32_t i);

/* ---- ImageProcessor::{palette, find, reduce} (core/src/lib.rs:67-164) on a one-process group: same arguments and results
 * as kmg_palette / kmg_find / kmg_reduce, byte for byte.  Every device uploads its band (and one halo row for the bilinear
 * shrink), shrinks its share of the <= 256-pixel working image (structures.rs:67-182), device 0 runs the k-means of that tiny
 * image (launch-bound: nothing to shard), and every device runs the output pass of its band -- the step that touches every
 * pixel -- and downloads it.  With shrink_max_dim = 0 and an image of at least 2^20 pixels the k-means itself runs sharded
 * (kmg_group_lloyd_*: initialisation, loop and the RCCL all-reduce per iteration).                                        */
KMG_API int kmg_group_palette(kmg_group *g, const uint8_t *rgba, uint32_t width, uint32_t height, uint32_t color_count, int algo,
                              uint8_t *out_rgba, uint32_t *out_count);
KMG_API int kmg_group_find(kmg_group *g, const uint8_t *rgba, uint32_t width, uint32_t height, const uint8_t *palette_rgba,
                           uint32_t n_colors, int mode, uint8_t *out_rgba);
KMG_API int kmg_group_reduce(kmg_group *g, const uint8_t *rgba, uint32_t width, uint32_t height, uint32_t color_count, int algo,
                             int mode, uint8_t *out_rgba);
/* A batch of images, WHOLE images per device (image i on local device i % n_local), no collective: kmg_reduce of every image
 * on its device's processor, the devices side by side (BASELINE config 4 as this build places it).  Returns the first failure.  */
KMG_API int kmg_group_reduce_batch(kmg_group *g, uint32_t n_images, const uint8_t *const *rgba, const uint32_t *widths,
                                   const uint32_t *heights, uint32_t color_count, int algo, int mode, uint8_t *const *out_rgba);

/* ---- ChooseCentroidModule::compute (core/src/modules.rs:763-840) over row bands that are resident on the group's devices.
 * d_rgba[i] (device memory of local device i) holds image rows [row0[i], row0[i] + rows[i]) of a width x height image,
 * d_labels[i] (optional) receives that band's u32 label map; rows[i] may be 0.  d_labels may be NULL as a whole, and any single
 * entry may be NULL: that band's label map is then not written, the other bands' are (a band without rows has none either way).
 * The bands of all ranks of the world tile the image: any split into whole rows, in any owner order (rank 0 may own the bottom
 * rows); results do not depend on the split.  _bind only records the bands, the image size and the flags, and replaces all three
 * of an earlier _bind of the same object (another image, other bands, other flags: any change in any direction; call it again too
 * when new pixels were written into bound bands); the centroids stay.  A refused _bind leaves the earlier one in place.  Argument
 * errors of every call below are refused on the host before any rank starts: the group stays usable.  The calls below
 * enqueue on the devices' compute streams and return -- only _run, _sync and _get_centroids synchronise.
 *   _init       PlusPlusInitModule::compute (modules.rs:946-1246) sharded: per centroid ONE all-gather of every band's
 *               {64-bit arg-max key, colour of the pixel it names} (kmg_lloyd_init_step / _init_pick_band); the largest key wins
 *   _prime      the initial assignment (operations.rs:75-83) with its sums, all-reduced
 *   _step       one iteration (modules.rs:769-800): centroid update from the global sums, labels + sums of the new
 *               assignment, all-reduce of the sums
 *   _run        _prime, then _step until the convergence count read every check_period-th iteration reaches k or
 *               max_iterations (kmg_options of the group's processors); *iterations as kmg_lloyd_run
 * flags (kmg_group_lloyd_bind):                                                                                            */
#define KMG_GROUP_CELLS   1u /* strong scaling of ONE image (colour table, k <= 256): the cube pass is sharded by cells of the
                                colour cube as well -- band histograms all-reduced once per image, per iteration the k x 4
                                all-reduce and an in-place all-gather of the label tables (kmg_lloyd_set_cell_share)        */
#define KMG_GROUP_OVERLAP 2u /* the all-reduce of the sums runs on a second stream beside the label pass (two cross-stream
                                dependencies per iteration) instead of in line on the compute stream                       */
#define KMG_GROUP_FUSED_UPDATE 4u /* _prime and _step perform the update on the last launch of the assignment that produced its sums:
                                     per call still one assignment with its label map and one update, shifted by half a step.  A
                                     world of ONE rank without collectives: kmg_lloyd_assign_update.  With KMG_GROUP_CELLS (bands
                                     with rows and label maps): the cube pass adds into the accumulators, the band's label pass
                                     updates from the all-reduced sums and clears them (kmg_lloyd_accumulate_into /
                                     _labels_from_tables_update: two launches per iteration instead of four).  Refused by _run,
                                     which reads the convergence count between update and re-assignment.
                                     What _prime + n x _step amount to, from centroids c0 (u = one update, A(c) = the assignment
                                     under c with its label maps and sums):
                                       flags                 world                      updates   centroids   label maps describe
                                       no FUSED_UPDATE       any                        n         c_n         A(c_n): after the last update
                                       FUSED_UPDATE          one rank, no collectives   n + 1     c_(n+1)     A(c_n): before the last update
                                        (with or without CELLS, any k: CELLS needs collectives)
                                       FUSED_UPDATE | CELLS  collectives, k <= 256      n + 1     c_(n+1)     A(c_n): before the last update
                                       FUSED_UPDATE alone    collectives                n         c_n         A(c_n): the flag is ignored
                                        (the all-reduce lies between assignment and update: the plain loop)
                                     FUSED_UPDATE | CELLS with collectives is refused by _bind (KMG_ERR_INVALID_ARGUMENT) when k > 256,
                                     a local rank has no rows, or a local rank has no label map.  KMG_GROUP_CELLS alone with
                                     k > 256 is the plain loop.  _step takes its sums from the _prime or _step before it; _prime
                                     starts over from the current centroids (after _bind, _set_centroids, _init, _run).               */
KMG_API int kmg_group_lloyd_create(kmg_group *g, uint32_t k, kmg_group_lloyd **out);
KMG_API void kmg_group_lloyd_destroy(kmg_group_lloyd *gl);
KMG_API int kmg_group_lloyd_bind(kmg_group_lloyd *gl, const uint8_t *const *d_rgba, const uint32_t *row0, const uint32_t *rows,
                                 uint32_t width, uint32_t height, uint32_t *const *d_labels, uint32_t flags);
KMG_API int kmg_group_lloyd_set_centroids(kmg_group_lloyd *gl, const float *centroids4);
KMG_API int kmg_group_lloyd_get_centroids(kmg_group_lloyd *gl, float *centroids4);
KMG_API int kmg_group_lloyd_init(kmg_group_lloyd *gl);
KMG_API int kmg_group_lloyd_prime(kmg_group_lloyd *gl);
KMG_API int kmg_group_lloyd_step(kmg_group_lloyd *gl);
KMG_API int kmg_group_lloyd_sync(kmg_group_lloyd *gl);
KMG_API int kmg_group_lloyd_run(kmg_group_lloyd *gl, uint32_t *iterations);
/* local device i's kmg_lloyd (profiling, statistics) and "table" (1) / "scan" (0) strategy of its band, once primed          */
KMG_API kmg_lloyd *kmg_group_lloyd_member(kmg_group_lloyd *gl, uint32_t i, int *strategy);

/* ---- a BATCH of images, each tiled over ALL ranks in row bands (BASELINE config 4 as north_star words it: "16 x 8192^2 tiled across 8
 * GPUs with one centroid all-reduce"; SURVEY 8e: "batch the 16 images' accumulators into one collective").  Every image is an
 * independent k-means problem with the same k; the accumulators of the whole batch are ONE block of n_images x k x 4 int64 per
 * rank, so an iteration costs a single ncclAllReduce of n_images * k * 32 bytes instead of one per image; the sharded
 * initialisation batches its keys and colours the same way.  (kmg_group_reduce_batch PLACES whole images instead -- zero
 * collectives, the faster split whenever the batch has at least as many images as the node has GPUs; this is for batches of fewer,
 * larger images, and for the configuration as worded.)
 *   _create_batch   like _create, n_images >= 1 (1 = kmg_group_lloyd_create)
 *   _bind_batch     d_rgba / row0 / rows / d_labels are indexed [image * n_local + local device], widths / heights [image];
 *                   KMG_GROUP_CELLS is refused (it shards ONE image's cube pass; a batch's cube passes already fill the ranks)
 *   _set / _get_centroids_image     one image's centroid table
 *   _init / _prime / _step / _sync  as above, over all images: one collective per exchange
 *   _run_batch      ChooseCentroidModule::compute for every image: an image whose convergence count reaches k at one of its
 *                   every-check_period checks stops being updated (its rows stay in the collective, zero); iterations[image] as
 *                   kmg_lloyd_run.  Results per image are those of kmg_lloyd_run on the whole image, bit for bit.              */
KMG_API int kmg_group_lloyd_create_batch(kmg_group *g, uint32_t k, uint32_t n_images, kmg_group_lloyd **out);
KMG_API int kmg_group_lloyd_bind_batch(kmg_group_lloyd *gl, const uint8_t *const *d_rgba, const uint32_t *row0, const uint32_t *rows,
                                       const uint32_t *widths, const uint32_t *heights, uint32_t *const *d_labels, uint32_t flags);
KMG_API int kmg_group_lloyd_set_centroids_image(kmg_group_lloyd *gl, uint32_t image, const float *centroids4);
KMG_API int kmg_group_lloyd_get_centroids_image(kmg_group_lloyd *gl, uint32_t image, float *centroids4);
KMG_API int kmg_group_lloyd_run_batch(kmg_group_lloyd *gl, uint32_t *iterations);

#ifdef __cplusplus
}
#endif
#endif /* KMEANS_HIP_H */
