// kmg_kernels.h -- launchers of the gfx950 kernels (internal to libkmeans_hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

namespace kmg {

// Device centroid entry: (L, a, b, C = sqrt(a^2 + b^2)).  C is hoisted out of the per-pixel loop
// (delta_e.wgsl:9 recomputes it for every pixel-centroid pair).
struct alignas(16) Centroid { float L, a, b, C; };

constexpr int kBlock = 256;          // threads per workgroup (4 waves of 64)

// The state words of a Lloyd object in device memory, which every update receives as `n_converged`: [0] the convergence count,
// [1 .. 3] the sparsity probe's, [kFixedWord] the number of frozen centroids (kmg_lloyd_set_fixed; update_centroids, kmg_device.h).
constexpr uint32_t kFixedWord = 8;
constexpr uint32_t kStateWords = 16;

// What the launchers size grids and LDS requests by, per device ORDINAL: a process may drive several devices (kmg_group's worker
// threads) and they need not be alike (a partitioned or mixed node).  Of the calling thread's current device; read once per ordinal.
struct DeviceInfo { uint32_t cus; size_t lds_max; };
const DeviceInfo &device_info();



// Number of workgroups the assign/accumulate pass uses for n pixels (also the number of rows of
// the per-workgroup partial-sum slab).
uint32_t assign_grid(uint64_t n_pixels);

hipError_t launch_rgb_to_lab(const uint32_t *rgba, uint64_t n, const float *lut, float *lab3,
                             hipStream_t st);

// labels and/or partial sums.  partials: [assign_grid(n)][k][4] int64, fully overwritten.
// weighted (kmg_lloyd_set_weighting; it changes the sums only): every pixel adds its alpha byte times (qL, qa, qb, 1); n <= 2^28.
hipError_t launch_assign(const uint32_t *rgba, uint64_t n, const Centroid *cent, uint32_t k,
                         const float *lut, uint32_t *labels, int64_t *partials, hipStream_t st, bool weighted = false);

// acc[k][4] = sum over rows of partials
hipError_t launch_reduce_partials(const int64_t *partials, uint32_t rows, uint32_t k,
                                  int64_t *acc, hipStream_t st);

// choose_centroid.wgsl `pick` for all k
// Small images (assign_loop_fits): one launch per Lloyd iteration -- every workgroup updates its own copy of the centroids from
// acc_in (do_update; workgroup 0 writes them to cent_out and the convergence count to n_converged), assigns, adds its sums to
// acc_out (zero on entry) and workgroup 0 clears acc_clear.  The caller rotates three k x 4 sum buffers and two centroid
// buffers (assign_loop_scratch_bytes(k) bytes hold the three sum buffers and the second centroid buffer).
bool assign_loop_fits(uint64_t n_pixels);
size_t assign_loop_scratch_bytes(uint32_t k);
hipError_t launch_assign_loop(const uint32_t *rgba, uint64_t n, const Centroid *cent, Centroid *cent_out, uint32_t k, const float *lut,
                              uint32_t *labels, const int64_t *acc_in, int64_t *acc_out, int64_t *acc_clear, int do_update,
                              float convergence, uint32_t *n_converged, hipStream_t st, bool weighted = false);
// rows x k x 4 values small enough (reduce_update_fits): reduction and -- do_update -- the update in one launch of one workgroup
bool reduce_update_fits(uint32_t rows, uint32_t k);
hipError_t launch_reduce_update(const int64_t *partials, uint32_t rows, uint32_t k, int64_t *acc, int do_update, float convergence,
                                Centroid *cent, uint32_t *n_converged, hipStream_t st);
// (all three updates: n_converged points at the object's state words -- the count, and kFixedWord behind it the number of frozen
// centroids, kmg_device.h)
hipError_t launch_update(const int64_t *acc, uint32_t k, float convergence, Centroid *cent,
                         uint32_t *n_converged, hipStream_t st);

// farthest-point init
hipError_t launch_init_first(const uint32_t *rgba, uint64_t index, const float *lut,
                             Centroid *cent, unsigned long long *key, hipStream_t st);
// pick = false: pass j into *key (atomicMax).  pick = true (whole image, one device): `key` = init_slots_bytes() of slots; the
// launch first picks centroid j - 1 from the slots of launch j - 1 (j >= 2), runs pass j and leaves its keys in the other slot
// set; launch_init_pick_slots picks the last centroid (j = k - 1) from the slots of the last pass
hipError_t launch_init_pass(const uint32_t *rgba, uint64_t n, const float *lut,
                            Centroid *cent, uint32_t j, float *dist,
                            unsigned long long *key, uint64_t first_index, hipStream_t st, bool pick = false);
size_t init_slots_bytes();
// Seeded initialisation: cent[0 .. n_seeds - 1] are given (1 <= n_seeds <= KMG_MAX_K).  One sweep does what passes 1 .. n_seeds do
// to the distance map and leaves pass n_seeds's keys in `slots`: launch_init_pass(j = n_seeds + 1, pick = true) continues from there.
hipError_t launch_init_seed(const uint32_t *rgba, uint64_t n, const float *lut, const Centroid *cent, uint32_t n_seeds, float *dist,
                            unsigned long long *slots, hipStream_t st);
// The same over the colours of a bound image (kmg_seed.hip): one sweep over every occupied cell does what launches 1 .. n_seeds of
// launch_init_pass_cells (kmg_table.h) do to the distance map, the cell records and the slots of init_scratch; that launcher
// continues from there with j = n_seeds + 1.
hipError_t launch_init_seed_cells(const uint32_t *tie, const uint8_t *occ_bits, const float4 *lab_table, const Centroid *cent,
                                  uint32_t n_seeds, float *dist, void *init_scratch, hipStream_t st);
// Whole image on one device, SEVERAL centroids per launch (kmg_kernels.hip k_init_multi): launch L = 1, 2, ... picks up to four
// centroids from what launch L - 1 left in `scratch` (init_multi_bytes(n); centroid 0 is there: launch_init_first) and sweeps the
// running distances against all of them; a launch that finds the table complete does nothing.  *init_multi_count(scratch, n, L)
// (device memory) = centroids chosen after launch L: the host enqueues launches in chunks and reads it in between.
size_t init_multi_bytes(uint64_t n);
hipError_t launch_init_multi(const uint32_t *rgba, uint64_t n, const float *lut, Centroid *cent, uint32_t k, uint32_t launch,
                             float *dist, void *scratch, hipStream_t st);
const uint32_t *init_multi_count(const void *scratch, uint64_t n, uint32_t launch);
hipError_t launch_init_pick_slots(const uint32_t *rgba, uint64_t n, const float *lut, const unsigned long long *slots, Centroid *cent,
                                  uint32_t j, hipStream_t st);
// sharded init (row bands): publish the colour of the pixel named by an all-reduced key; set one centroid
hipError_t launch_init_pick_band(const uint32_t *rgba, uint64_t n, uint64_t first_index,
                                 const unsigned long long *key, uint32_t *colour2, hipStream_t st);
hipError_t launch_set_centroid_rgba(const uint32_t *colour, const float *lut, Centroid *cent, uint32_t j,
                                    hipStream_t st);

hipError_t launch_resize(const uint32_t *rgba, uint32_t w, uint32_t h, uint32_t nw, uint32_t nh,
                         uint32_t *out, hipStream_t st);
// The same resize for a row band of a sharded image: `band` holds the image rows from src_row0 on (at least every source row
// the requested output rows sample: resize_source_row(gy) and the row below it), `out` receives output rows
// [out_row0, out_row0 + out_rows).  Same values as launch_resize of the whole image, row for row.
hipError_t launch_resize_band(const uint32_t *band, uint32_t w, uint32_t h, uint32_t src_row0, uint32_t nw, uint32_t nh,
                              uint32_t out_row0, uint32_t out_rows, uint32_t *out, hipStream_t st);
uint32_t resize_source_row(uint32_t gy, uint32_t h, uint32_t nh);

// alpha mode (kmg_alpha.hip): out[0 .. n_kept) = the pixels whose alpha byte is >= cutoff, in order; *n_kept (device) = their
// number.  counts: alpha_compact_grid(n) words of scratch.  Two launches on st.
uint32_t alpha_compact_grid(uint64_t n);
hipError_t launch_alpha_compact(const uint32_t *rgba, uint64_t n, uint32_t cutoff, uint32_t *out, unsigned long long *n_kept,
                                unsigned long long *counts, hipStream_t st);
// out[i] = (out[i] & 0x00FFFFFF) | (rgba[i] & 0xFF000000): alpha mode after an output kernel without the compile-time switch
hipError_t launch_alpha_merge(const uint32_t *rgba, uint32_t *out, uint64_t n, hipStream_t st);

// ---- The output passes.  Where a family has index output (kmg_output_format) its launcher takes (void *out, int format,
// alpha_cutoff): out holds RGBA8 words (format 0), or the label of every pixel as u8 (1) / u16 (2).  alpha_cutoff != 0 is alpha
// mode, a separate instantiation of the kernel (alpha_cutoff = 0 runs the code of the passes without alpha mode): RGBA8 keeps the
// pixel's own alpha byte over the output's, an index format writes k where the pixel's alpha is below the cutoff.  pal is read by
// RGBA8 only.  A format (or route) that does not exist: hipErrorInvalidValue, nothing launched.

// ---- The offsets of KMG_MODE_DITHER, the last template parameter and a by-value argument of the kernels that dither per image
// (k_apply, k_dither_lists): the reference's matrix, which the kernels carry in their code, or a threshold map
// (include/kmeans_hip.h at kmg_dither_map).  A workgroup stages its offsets into LDS behind the sRGB table.
// v: mw x mh values in device memory, row-major; the sides are powers of two, so pixel (x, y) reads
// v[(x & xmask) + ((y & ymask) << xshift)].
struct DitherMapDev { const float *v; uint32_t xmask, ymask, xshift; };
static inline uint32_t dither_map_entries(const DitherMapDev &m) { return (m.xmask + 1u) * (m.ymask + 1u); }
struct BayerOffsets { float threshold; };              // 16 offsets threshold * (M / 16 - 0.5): as a kernel argument, the float
struct MapOffsets { float t; DitherMapDev map; };      // mw x mh offsets t * v, t = threshold * strength
// (The two places where the forms differ -- staging the offsets, and which of them pixel (x, y) reads -- are `if constexpr (MAP)`
// inside the two kernels, not helpers here: as inlined functions the 16-entry index came out with its operands in another order
// and the staging loop four instructions longer (tools/compare_kernels.py), and the instantiations keep the code they had.)
// The launchers take a MapOffsets: map.v == nullptr is the reference's matrix at threshold t (dither_offsets<BayerOffsets>).
template <typename Off>
inline Off dither_offsets(const MapOffsets &o)
{
    if constexpr (std::is_same<Off, MapOffsets>::value) return o; else return BayerOffsets{o.t};
}

// the list-based dither and meld passes (kmg_lists.hip); kmg_table.h declares them without alpha mode (RGBA8)
hipError_t launch_meld_lists(const uint32_t *rgba, uint64_t n, const Centroid *cent, uint32_t k, const float *lut,
                             const uint8_t *lists, uint32_t *out, hipStream_t st, bool alpha);
hipError_t launch_dither_lists(const uint32_t *rgba, uint32_t w, uint32_t rows, uint32_t row0, const Centroid *cent, uint32_t k,
                               const float *lut, const uint32_t *pal, const MapOffsets &off, const uint8_t *lists, void *out, int format,
                               hipStream_t st, uint32_t alpha_cutoff);

// replace / dither output pass.  pal: k+1 RGBA8 words (entry k = the converted sentinel).  off is read when `dither`.  With a map
// the pass needs apply_map_lds_bytes of dynamic LDS, which the caller compares with device_info().lds_max (the launcher refuses a
// request above it: hipErrorInvalidValue).
size_t apply_map_lds_bytes(uint32_t k, uint32_t map_entries);
hipError_t launch_apply(const uint32_t *rgba, uint32_t w, uint32_t rows, uint32_t row0, const Centroid *cent, uint32_t k, const float *lut,
                        const uint32_t *pal, bool dither, const MapOffsets &off, void *out, int format, hipStream_t st, uint32_t alpha_cutoff = 0);

// launch_lab_candidates (kmg_table.h) of the dither pass for offsets in [off_lo, off_hi] instead of the reference matrix's
// threshold * [-0.5, 0.4375]: the box of cells that get a list (speed only; cells outside mean "scan everything")
hipError_t launch_lab_candidates_range(const Centroid *cent, uint32_t k, float off_lo, float off_hi, bool two_closest, uint8_t *lists,
                                       hipStream_t st);

// thr[256] (device): the linear-channel thresholds of the 256 sRGB8 output bytes (k_meld), made by the device's own encode
hipError_t launch_encode_thresholds(float *thr, hipStream_t st);
// out[0..2] (device; the caller sets {0, ~0, 0}): mismatches of div_const(x, c) against x / c over every binary32 x, and the
// smallest / largest |x| bit pattern among them
hipError_t launch_division_check(float c, unsigned long long *out, hipStream_t st);
// *bad (device, zeroed by the caller) += the floats (all of them, NaN aside) whose table byte is not the encode's byte
hipError_t launch_encode_check(const float *thr, unsigned long long *bad, hipStream_t st);
// meld output pass (mix_colors.wgsl main_meld + lab_to_rgb.wgsl); lut: 256 decode entries followed by the 256 thresholds
// masks: NULL, or per colour cell the candidate centroids of kmg_table.h's launch_meld_candidates
hipError_t launch_meld(const uint32_t *rgba, uint64_t n, const Centroid *cent, uint32_t k, const float *lut,
                       const uint64_t *masks, uint32_t *out, hipStream_t st, bool alpha = false);

// error-diffusion output pass, KMG_MODE_DIFFUSE (kmg_diffuse.hip).  route: how a quantised colour finds its label --
// kDiffuseScan: per-lane arg-min over cent (LDS); kDiffusePairs (k <= 256) / kDiffuseCells (k > 256): the replace pass's colour
// table (colour_labels + sub_table of launch_cube without histogram).  erow: two slots of packed error words, slot `parity` = the
// error of the row above the band (zero for a first band); the band leaves its last row's error in slot (parity + chunks) & 1.
// ctl: diffuse_ctl_bytes() of per-call control words, zero on entry; ctl word 1 != 0 afterwards = the pass timed out.
// sticky: a word the caller zeroes once; a pass that times out also sets it (so a later pass does not hide the failure).
// alpha_cutoff != 0: alpha mode -- pixels below the cutoff take no part in the diffusion, every output keeps its pixel's alpha.
enum { kDiffuseScan = 0, kDiffusePairs = 1, kDiffuseCells = 2 };
constexpr uint32_t kDiffuseRing = 1024;
size_t diffuse_ctl_bytes();
uint32_t diffuse_grid(int route, uint32_t rows);
// filter (kmg_diffusion): Floyd-Steinberg runs k_diffuse, the others k_diffuse_wide (kmg_diffuse_wide.hip), whose slots hold TWO
// rows -- the errors of the row above the band and of the row above that -- and which leaves its last two rows' errors.
// diffuse_erow_bytes(w): the size of erow for any filter; diffuse_slot_bytes(filter, w): the bytes of slot `parity` (at
// erow + parity * that) which the caller zeroes before the first band of an image.
size_t diffuse_erow_bytes(uint32_t w);
size_t diffuse_slot_bytes(int filter, uint32_t w);
hipError_t launch_diffuse(int route, int filter, const uint32_t *rgba, uint32_t w, uint32_t rows, void *out, int format, void *erow,
                          uint32_t parity, void *ctl, uint32_t *sticky, const Centroid *cent, uint32_t k, const float *lut,
                          const uint32_t *pal, const void *colour_labels, const uint16_t *sub_table, hipStream_t st, uint32_t alpha_cutoff);

// kmg_index.hip, index formats only: the replace pass through the colour cube's label tables (those launch_labels reads: the pair
// entries and u8 per-colour labels for k <= 256, the 8x8x8 / 4x4x4 summaries and u16 per-colour labels above)
hipError_t launch_labels_index(const uint32_t *rgba, uint64_t n, const void *colour_labels, const uint16_t *sub_table, uint32_t k,
                               void *out, int format, hipStream_t st, uint32_t alpha_cutoff);
// kmg_index.hip, index formats only: out[i] = labels[i] (u32 labels of a pass that ran with an identity palette) as u8 / u16, or k
// where alpha mode drops the pixel
hipError_t launch_narrow_index(const uint32_t *rgba, const uint32_t *labels, uint64_t n, uint32_t k, void *out, int format, hipStream_t st,
                               uint32_t alpha_cutoff);

// ---- error statistics (kmg_error.hip; kmg_error_stats of include/kmeans_hip.h): `stats` = 14 u64 the launch COMBINES into (sums
// added, maxima maxed).  form: what `out` holds per pixel -- an RGBA8 word, a u8 / u16 palette index, or a u32 label (the quality
// search's own).  Index forms: pal = k palette words, entries = error_palette_bytes(k) written by launch_error_palette from them
// (both in device memory; entries are read only when `what` has KMG_ERROR_LAB).  n < 2^32.
enum { kErrorRgba8 = 0, kErrorIndex8 = 1, kErrorIndex16 = 2, kErrorLabel32 = 3 };
size_t error_palette_bytes(uint32_t k);
hipError_t launch_error_palette(const uint32_t *pal, uint32_t k, const float *lut, void *entries, hipStream_t st);
hipError_t launch_error_stats(int form, uint32_t what, const uint32_t *src, const void *out, uint64_t n, const uint32_t *pal,
                              const void *entries, uint32_t k, uint32_t cutoff, const float *lut, unsigned long long *stats, hipStream_t st);

// ---- index-map optimisation (kmg_usage.hip; kmg_dev_index_usage / kmg_dev_index_remap of include/kmeans_hip.h).  wide: the map
// holds u16 (else u8).  usage: k + 2 u64 the launch ADDS to (bin k: the transparent slot, bin k + 1: indices above k).  n < 2^32.
hipError_t launch_index_usage(const void *index, bool wide, uint64_t n, uint32_t k, unsigned long long *usage, hipStream_t st);
// out = map[in] at out_bits (8 / 16: one element per pixel; 1 / 2 / 4: packed rows, each starting on a byte); map: k + 1 u16 in
// device memory, 0xFFFF = dropped; *bad += the pixels written as 0 because they have no new index that fits.  width * rows < 2^32.
hipError_t launch_index_remap(const void *in, bool wide, uint32_t width, uint32_t rows, uint32_t k, const uint16_t *map, uint32_t out_bits,
                              void *out, unsigned long long *bad, hipStream_t st);

}  // namespace kmg
