//! `extern "C"` view of `include/kmeans_hip.h` -- the host-buffer API, i.e. exactly what
//! `ImageProcessor::{new, palette, find, reduce}` (reference `core/src/lib.rs:38-164`) need.
//! Every item below is checked against the header by `tests/test_rust_shim.py`.
#![allow(non_camel_case_types)]

use std::os::raw::{c_char, c_int};

/// Opaque `kmg_processor` (include/kmeans_hip.h).
#[repr(C)]
pub struct kmg_processor {
    _private: [u8; 0],
}

/// `kmg_options` (include/kmeans_hip.h); `kmg_default_options` fills in the reference's constants
/// (structures.rs:23, modules.rs:765-766, lib.rs:189-194).
#[repr(C)]
#[derive(Clone, Copy)]
pub struct kmg_options {
    pub struct_size: u32,
    pub device: i32,
    pub shrink_max_dim: u32,
    pub max_iterations: u32,
    pub check_period: u32,
    pub convergence: f32,
    pub strategy: i32,
    pub alpha_cutoff: u32,
}

/// `kmg_options.strategy` (KMG_STRATEGY_*): 0 = the library's cost models decide per call; results are identical either way.
pub const KMG_STRATEGY_AUTO: i32 = 0;
pub const KMG_STRATEGY_SCAN: i32 = 1;
pub const KMG_STRATEGY_TABLE: i32 = 2;
pub const KMG_STRATEGY_MASK_WORDS: i32 = 4;

/// Opaque `kmg_group`: a processor + RCCL rank per device of a list (include/kmeans_hip.h, "a group of devices").
#[repr(C)]
pub struct kmg_group {
    _private: [u8; 0],
}

pub const KMG_MAX_DEVICES: usize = 16;

/// `kmg_group_options` (include/kmeans_hip.h); `kmg_default_group_options` fills it in.
#[repr(C)]
#[derive(Clone, Copy)]
pub struct kmg_group_options {
    pub struct_size: u32,
    pub n_devices: u32,
    pub devices: [i32; KMG_MAX_DEVICES],
    pub flags: u32,
    pub processor: kmg_options,
}

pub const KMG_OK: c_int = 0;
pub const KMG_ALGO_KMEANS: c_int = 0;
pub const KMG_ALGO_OCTREE: c_int = 1;
pub const KMG_MODE_REPLACE: c_int = 0;
pub const KMG_MODE_DITHER: c_int = 1;
pub const KMG_MODE_MELD: c_int = 2;
pub const KMG_MODE_DIFFUSE: c_int = 3;
/// `kmg_diffusion`: the filter of KMG_MODE_DIFFUSE (kmg_processor_set_diffusion)
pub const KMG_DIFFUSION_FLOYD_STEINBERG: c_int = 0;
pub const KMG_DIFFUSION_SIERRA_LITE: c_int = 1;
pub const KMG_DIFFUSION_ATKINSON: c_int = 2;
pub const KMG_DIFFUSION_BURKES: c_int = 3;
pub const KMG_DIFFUSION_SIERRA2: c_int = 4;
pub const KMG_DIFFUSION_SIERRA3: c_int = 5;
pub const KMG_DIFFUSION_JARVIS: c_int = 6;
pub const KMG_DIFFUSION_STUCKI: c_int = 7;
pub const KMG_DIFFUSION_COUNT: c_int = 8;
/// `kmg_dither_map`: the threshold map of KMG_MODE_DITHER (kmg_processor_set_dither)
pub const KMG_DITHER_BAYER4: c_int = 0;
pub const KMG_DITHER_BAYER2: c_int = 1;
pub const KMG_DITHER_BAYER8: c_int = 2;
pub const KMG_DITHER_BAYER16: c_int = 3;
pub const KMG_DITHER_BLUE64: c_int = 4;
pub const KMG_DITHER_CUSTOM: c_int = 5;
pub const KMG_DITHER_COUNT: c_int = 6;
/// the header's name of a map level (tests/test_rust_shim.py compares the declarations below with the header's by type name)
pub type uint16_t = u16;
/// `kmg_output_format`: RGBA8, or one u8 / u16 palette index per pixel (`kmg_find_indexed`, `kmg_reduce_indexed`).
pub const KMG_FORMAT_RGBA8: c_int = 0;
pub const KMG_FORMAT_INDEX8: c_int = 1;
pub const KMG_FORMAT_INDEX16: c_int = 2;

/// `KMG_ERROR_*`: the parts of a `kmg_error_stats` record a comparison computes.
pub const KMG_ERROR_RGB: u32 = 1;
pub const KMG_ERROR_LAB: u32 = 2;

/// `kmg_error_stats` (include/kmeans_hip.h): 14 x u64, exact integer sums and maxima of an output against its source.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct kmg_error_stats {
    pub pixels: u64,
    pub changed: u64,
    pub invalid: u64,
    pub sse: [u64; 3],
    pub sad: [u64; 3],
    pub max_abs: [u64; 3],
    pub lab_sse: u64,
    pub lab_max: u64,
}

/// Opaque `kmg_sequence`: one palette for many frames, and their index maps as delta frames (include/kmeans_hip.h).
#[repr(C)]
pub struct kmg_sequence {
    _private: [u8; 0],
}

/// `kmg_sequence_output_frame*` flags.
pub const KMG_FRAME_DELTA: u32 = 1;
/// `kmg_sequence_output_begin_local` flags.
pub const KMG_LOCAL_WARM: u32 = 1;

/// `kmg_frame_delta` (include/kmeans_hip.h): 32 bytes; the fresh record is {0, 0, u32::MAX, u32::MAX, 0, 0}.
#[repr(C)]
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub struct kmg_frame_delta {
    pub changed: u64,
    pub cleared: u64,
    pub x0: u32,
    pub y0: u32,
    pub x1: u32,
    pub y1: u32,
}

/// `kmg_frame_hold` (include/kmeans_hip.h): 48 bytes -- the fields of `kmg_frame_delta`, then the pixels a lossy delta frame held
/// and the sum of their distances D (1/4096 dE76^2) to their anchors.
#[repr(C)]
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub struct kmg_frame_hold {
    pub changed: u64,
    pub cleared: u64,
    pub x0: u32,
    pub y0: u32,
    pub x1: u32,
    pub y1: u32,
    pub held: u64,
    pub held_sse: u64,
}

/// `kmg_batch_report` (include/kmeans_hip.h): 16 bytes, what a batch call did.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct kmg_batch_report {
    pub launches: u32,
    pub iterations: u32,
    pub sub_batches: u32,
    pub fallback: u32,
}

/// `kmg_batch_apply_report` (include/kmeans_hip.h): 16 bytes, what the output step of a batch call did.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct kmg_batch_apply_report {
    pub launches: u32,
    pub batched: u32,
    pub per_image: u32,
    pub sub_batches: u32,
}

/// `kmg_batch_quality_report` (include/kmeans_hip.h): 32 bytes, what kmg_reduce_quality_batch did.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct kmg_batch_quality_report {
    pub rounds: u32,
    pub palette_runs: u32,
    pub launches: u32,
    pub measure_launches: u32,
    pub batched: u32,
    pub per_image: u32,
    pub sub_batches: u32,
    pub fallback: u32,
}

extern "C" {
    pub fn kmg_last_error() -> *const c_char;
    pub fn kmg_version() -> *const c_char;
    pub fn kmg_default_options(opt: *mut kmg_options);
    // ImageProcessor::new -- lib.rs:38-65
    pub fn kmg_processor_create(out: *mut *mut kmg_processor) -> c_int;
    pub fn kmg_processor_create_ex(opt: *const kmg_options, out: *mut *mut kmg_processor) -> c_int;
    pub fn kmg_processor_destroy(p: *mut kmg_processor);
    pub fn kmg_processor_set_strategy(p: *mut kmg_processor, strategy: c_int) -> c_int;
    pub fn kmg_processor_set_alpha_cutoff(p: *mut kmg_processor, alpha_cutoff: u32) -> c_int;
    pub fn kmg_processor_set_fixed_colors(p: *mut kmg_processor, rgba: *const u8, n: u32) -> c_int;
    pub fn kmg_processor_set_weighting(p: *mut kmg_processor, weighting: c_int) -> c_int;
    pub fn kmg_processor_set_diffusion(p: *mut kmg_processor, filter: c_int) -> c_int;
    pub fn kmg_diffusion_weights(filter: c_int, weights: *mut i32, divisor: *mut i32) -> c_int;
    pub fn kmg_processor_set_dither(p: *mut kmg_processor, map: c_int, strength: f32) -> c_int;
    pub fn kmg_processor_set_dither_custom(
        p: *mut kmg_processor,
        levels: *const uint16_t,
        width: u32,
        height: u32,
        n_levels: u32,
        strength: f32,
    ) -> c_int;
    pub fn kmg_dither_map_values(map: c_int, width: *mut u32, height: *mut u32, n_levels: *mut u32, levels: *mut uint16_t) -> c_int;
    // ImageProcessor::palette -- lib.rs:67-77
    pub fn kmg_palette(
        p: *mut kmg_processor,
        rgba: *const u8,
        width: u32,
        height: u32,
        color_count: u32,
        algo: c_int,
        out_rgba: *mut u8,
        out_count: *mut u32,
    ) -> c_int;
    // ImageProcessor::find -- lib.rs:79-114
    pub fn kmg_find(
        p: *mut kmg_processor,
        rgba: *const u8,
        width: u32,
        height: u32,
        palette_rgba: *const u8,
        n_colors: u32,
        mode: c_int,
        out_rgba: *mut u8,
    ) -> c_int;
    // ImageProcessor::reduce -- lib.rs:116-164
    pub fn kmg_reduce(
        p: *mut kmg_processor,
        rgba: *const u8,
        width: u32,
        height: u32,
        color_count: u32,
        algo: c_int,
        mode: c_int,
        out_rgba: *mut u8,
    ) -> c_int;
    // find / reduce with an output format: out_index receives 4, 1 or 2 bytes per pixel (a `void *` in the header)
    pub fn kmg_find_indexed(
        p: *mut kmg_processor,
        rgba: *const u8,
        width: u32,
        height: u32,
        palette_rgba: *const u8,
        n_colors: u32,
        mode: c_int,
        format: c_int,
        out_index: *mut (),
    ) -> c_int;
    pub fn kmg_reduce_indexed(
        p: *mut kmg_processor,
        rgba: *const u8,
        width: u32,
        height: u32,
        color_count: u32,
        algo: c_int,
        mode: c_int,
        format: c_int,
        out_palette_rgba: *mut u8,
        out_count: *mut u32,
        out_index: *mut (),
    ) -> c_int;
    // batches (no counterpart in the reference): many small images per launch on one device.  `rgba`, `widths`, `heights`,
    // `out_rgba` (and `out_counts`) are arrays of `n_images` entries; `d_rgba` holds device pointers.  (The pointer arrays are
    // written the way tests/test_rust_shim.py derives a `T *const *` from the header; the library reads the arrays and writes
    // through the entries of `out_rgba` only.)
    pub fn kmg_dev_palette_batch(
        p: *mut kmg_processor,
        n_images: u32,
        d_rgba: *mut *const u8,
        widths: *const u32,
        heights: *const u32,
        k: u32,
        centroids4: *mut f32,
        iterations: *mut u32,
        report: *mut kmg_batch_report,
        stream: *mut (),
    ) -> c_int;
    pub fn kmg_palette_batch(
        p: *mut kmg_processor,
        n_images: u32,
        rgba: *mut *const u8,
        widths: *const u32,
        heights: *const u32,
        color_count: u32,
        algo: c_int,
        max_resident_bytes: u64,
        out_rgba: *mut *const u8,
        out_counts: *mut u32,
        report: *mut kmg_batch_report,
    ) -> c_int;
    pub fn kmg_reduce_batch(
        p: *mut kmg_processor,
        n_images: u32,
        rgba: *mut *const u8,
        widths: *const u32,
        heights: *const u32,
        color_count: u32,
        algo: c_int,
        mode: c_int,
        max_resident_bytes: u64,
        out_rgba: *mut *const u8,
        report: *mut kmg_batch_report,
    ) -> c_int;
    // batched output: the output passes of many small images in one launch.  `d_out`, `out`, `out_index` and `out_palette_rgba`
    // are arrays of `n_images` pointers the library writes through; `centroids4` holds `n_tables` (1 or `n_images`) tables.
    pub fn kmg_dev_apply_batch(
        p: *mut kmg_processor,
        n_images: u32,
        d_rgba: *mut *const u8,
        widths: *const u32,
        heights: *const u32,
        centroids4: *const f32,
        n_tables: u32,
        k: u32,
        mode: c_int,
        format: c_int,
        d_out: *mut *const (),
        report: *mut kmg_batch_apply_report,
        stream: *mut (),
    ) -> c_int;
    pub fn kmg_find_batch(
        p: *mut kmg_processor,
        n_images: u32,
        rgba: *mut *const u8,
        widths: *const u32,
        heights: *const u32,
        palette_rgba: *const u8,
        n_colors: u32,
        mode: c_int,
        format: c_int,
        max_resident_bytes: u64,
        out: *mut *const (),
        report: *mut kmg_batch_apply_report,
    ) -> c_int;
    pub fn kmg_reduce_indexed_batch(
        p: *mut kmg_processor,
        n_images: u32,
        rgba: *mut *const u8,
        widths: *const u32,
        heights: *const u32,
        color_count: u32,
        algo: c_int,
        mode: c_int,
        format: c_int,
        max_resident_bytes: u64,
        out_palette_rgba: *mut *const u8,
        out_counts: *mut u32,
        out_index: *mut *const (),
        batch_report: *mut kmg_batch_report,
        apply_report: *mut kmg_batch_apply_report,
    ) -> c_int;
    // batched quality targets: a colour count per image (`ks`: `n_images` counts; `centroids4` / `palettes_rgba` concatenated in
    // image order), the batched error record, and kmg_reduce_quality for many small images
    pub fn kmg_dev_palette_batch_counts(
        p: *mut kmg_processor,
        n_images: u32,
        d_rgba: *mut *const u8,
        widths: *const u32,
        heights: *const u32,
        ks: *const u32,
        centroids4: *mut f32,
        iterations: *mut u32,
        report: *mut kmg_batch_report,
        stream: *mut (),
    ) -> c_int;
    pub fn kmg_dev_apply_batch_counts(
        p: *mut kmg_processor,
        n_images: u32,
        d_rgba: *mut *const u8,
        widths: *const u32,
        heights: *const u32,
        centroids4: *const f32,
        ks: *const u32,
        mode: c_int,
        format: c_int,
        d_out: *mut *const (),
        report: *mut kmg_batch_apply_report,
        stream: *mut (),
    ) -> c_int;
    pub fn kmg_dev_compare_batch(
        p: *mut kmg_processor,
        n_images: u32,
        d_src_rgba: *mut *const u8,
        d_out: *mut *const (),
        n_pixels: *const u64,
        format: c_int,
        palettes_rgba: *const u8,
        ks: *const u32,
        alpha_cutoff: u32,
        what: u32,
        d_stats: *mut kmg_error_stats,
        stream: *mut (),
    ) -> c_int;
    pub fn kmg_reduce_quality_batch(
        p: *mut kmg_processor,
        n_images: u32,
        rgba: *mut *const u8,
        widths: *const u32,
        heights: *const u32,
        k_min: u32,
        k_max: u32,
        target: u32,
        mode: c_int,
        format: c_int,
        max_resident_bytes: u64,
        out_palette_rgba: *mut *const u8,
        out_counts: *mut u32,
        out: *mut *const (),
        achieved: *mut kmg_error_stats,
        reached: *mut c_int,
        report: *mut kmg_batch_quality_report,
    ) -> c_int;
    // error statistics of an output against its source (host buffers; `out` holds 4, 1 or 2 bytes per pixel for `format`) and the
    // colour count chosen by a quality target: no counterpart in the reference
    pub fn kmg_compare(
        p: *mut kmg_processor,
        src_rgba: *const u8,
        out: *const (),
        width: u32,
        height: u32,
        format: c_int,
        palette_rgba: *const u8,
        k: u32,
        what: u32,
        stats: *mut kmg_error_stats,
    ) -> c_int;
    pub fn kmg_reduce_quality(
        p: *mut kmg_processor,
        rgba: *const u8,
        width: u32,
        height: u32,
        k_min: u32,
        k_max: u32,
        target: u32,
        mode: c_int,
        format: c_int,
        out_palette_rgba: *mut u8,
        out_count: *mut u32,
        out: *mut (),
        achieved: *mut kmg_error_stats,
        reached: *mut c_int,
    ) -> c_int;
    // frame sequences (no counterpart in the reference): a shared palette, then every frame as a full, an exact delta or a lossy
    // delta index map (`tolerance` in 1/4096 dE76^2; `out` holds 4, 1 or 2 bytes per pixel for the format of `_output_begin`)
    pub fn kmg_sequence_create(p: *mut kmg_processor, out: *mut *mut kmg_sequence) -> c_int;
    pub fn kmg_sequence_destroy(s: *mut kmg_sequence);
    pub fn kmg_sequence_add(s: *mut kmg_sequence, rgba: *const u8, width: u32, height: u32) -> c_int;
    pub fn kmg_sequence_clear(s: *mut kmg_sequence) -> c_int;
    pub fn kmg_sequence_output_begin(
        s: *mut kmg_sequence,
        k: u32,
        mode: c_int,
        format: c_int,
        width: u32,
        height: u32,
        out_palette_rgba: *mut u8,
        out_count: *mut u32,
    ) -> c_int;
    pub fn kmg_sequence_output_frame(
        s: *mut kmg_sequence,
        rgba: *const u8,
        flags: u32,
        out: *mut (),
        info: *mut kmg_frame_delta,
        is_full: *mut c_int,
    ) -> c_int;
    pub fn kmg_sequence_output_frame_lossy(
        s: *mut kmg_sequence,
        rgba: *const u8,
        flags: u32,
        tolerance: u32,
        out: *mut (),
        info: *mut kmg_frame_hold,
        is_full: *mut c_int,
    ) -> c_int;
    pub fn kmg_sequence_output_end(s: *mut kmg_sequence) -> c_int;
    // per-frame palettes: the colour-keyed delta passes on device buffers (the canvas holds RGBA8 words, 0 = nothing shown), and a
    // frame output in which every frame gets its own palette (`tolerance` NULL: an exact frame; `flags` of the begin: KMG_LOCAL_WARM)
    pub fn kmg_dev_frame_delta_colour(
        p: *mut kmg_processor,
        d_index: *const (),
        d_palette_rgba: *const u8,
        d_shown_rgba: *mut u8,
        width: u32,
        rows: u32,
        row0: u32,
        format: c_int,
        k: u32,
        d_delta: *mut (),
        d_info: *mut kmg_frame_delta,
        stream: *mut (),
    ) -> c_int;
    pub fn kmg_dev_frame_delta_colour_lossy(
        p: *mut kmg_processor,
        d_src_rgba: *const u8,
        d_index: *const (),
        d_palette_rgba: *const u8,
        d_shown_rgba: *mut u8,
        d_held_rgba: *mut u8,
        width: u32,
        rows: u32,
        row0: u32,
        format: c_int,
        k: u32,
        tolerance: u32,
        d_delta: *mut (),
        d_info: *mut kmg_frame_hold,
        stream: *mut (),
    ) -> c_int;
    pub fn kmg_sequence_output_begin_local(
        s: *mut kmg_sequence,
        k: u32,
        mode: c_int,
        format: c_int,
        width: u32,
        height: u32,
        flags: u32,
    ) -> c_int;
    pub fn kmg_sequence_output_frame_local(
        s: *mut kmg_sequence,
        rgba: *const u8,
        flags: u32,
        tolerance: *const u32,
        out: *mut (),
        out_palette_rgba: *mut u8,
        out_count: *mut u32,
        info: *mut kmg_frame_hold,
        is_full: *mut c_int,
    ) -> c_int;
    // ImageProcessor::new over a device list (the reference is single-device: lib.rs:38-65) and the same three calls, the image
    // tiled in row bands over the devices, the k x 4 sums of a sharded Lloyd loop all-reduced by RCCL inside the library
    pub fn kmg_default_group_options(opt: *mut kmg_group_options);
    pub fn kmg_group_create(opt: *const kmg_group_options, out: *mut *mut kmg_group) -> c_int;
    pub fn kmg_group_destroy(g: *mut kmg_group);
    pub fn kmg_group_palette(
        g: *mut kmg_group,
        rgba: *const u8,
        width: u32,
        height: u32,
        color_count: u32,
        algo: c_int,
        out_rgba: *mut u8,
        out_count: *mut u32,
    ) -> c_int;
    pub fn kmg_group_find(
        g: *mut kmg_group,
        rgba: *const u8,
        width: u32,
        height: u32,
        palette_rgba: *const u8,
        n_colors: u32,
        mode: c_int,
        out_rgba: *mut u8,
    ) -> c_int;
    pub fn kmg_group_reduce(
        g: *mut kmg_group,
        rgba: *const u8,
        width: u32,
        height: u32,
        color_count: u32,
        algo: c_int,
        mode: c_int,
        out_rgba: *mut u8,
    ) -> c_int;
}
