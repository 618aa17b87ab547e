//! `kmeans_color_gpu` on AMD MI355X: the public surface of the reference crate
//! (`core/src/lib.rs:24-253`: `ImageProcessor::{new, palette, find, reduce}`, `Image`, `Algorithm`,
//! `ReduceMode`, `ColorSpace`, `RGBA8`) implemented by `libkmeans_hip.so` through `ffi`.
//!
//! The methods stay `async` so that callers that `block_on` them (cli/src/main.rs:27-40, core/examples) compile
//! unchanged; the futures are ready immediately -- the library call is synchronous and thread safe
//! (one `ImageProcessor` may be shared by many threads, core/examples/parallel.rs:36-50).
use std::ffi::CStr;
use std::fmt::Display;
use std::os::raw::c_int;
use std::str::FromStr;

use anyhow::{anyhow, Result};
pub use rgb::RGBA8;

use crate::image::{Container, Image};

mod ffi;
pub mod image;

pub struct ImageProcessor {
    raw: *mut ffi::kmg_processor,
    /// non-null: the processor spans several devices (`with_devices`); the calls go through `kmg_group_*`
    group: *mut ffi::kmg_group,
}

// every entry point of libkmeans_hip is re-entrant on one processor (per-call stream and workspace)
unsafe impl Send for ImageProcessor {}
unsafe impl Sync for ImageProcessor {}

fn check(rc: c_int) -> Result<()> {
    if rc == ffi::KMG_OK {
        return Ok(());
    }
    let msg = unsafe { CStr::from_ptr(ffi::kmg_last_error()) }.to_string_lossy().into_owned();
    Err(anyhow!("kmeans_hip error {rc}: {msg}"))
}

impl ImageProcessor {
    /// lib.rs:38-65.  Fails when no HIP device is usable (there is no CPU path), as the reference fails
    /// without a wgpu adapter.
    pub async fn new() -> Result<Self> {
        let mut raw = std::ptr::null_mut();
        check(unsafe { ffi::kmg_processor_create(&mut raw) })?;
        log::debug!("{}", unsafe { CStr::from_ptr(ffi::kmg_version()) }.to_string_lossy());
        Ok(ImageProcessor { raw, group: std::ptr::null_mut() })
    }

    /// The same constructor over several GPUs of the node (HIP ordinals; empty = every visible device).  No counterpart in
    /// the reference, which picks one adapter (lib.rs:38-65): `palette`, `find` and `reduce` then tile the image in row bands
    /// over the devices and return the same bytes; a sharded Lloyd loop all-reduces its k x 4 integer sums with RCCL.
    pub async fn with_devices(devices: &[i32]) -> Result<Self> {
        let mut opt: ffi::kmg_group_options = unsafe { std::mem::zeroed() };
        unsafe { ffi::kmg_default_group_options(&mut opt) };
        if devices.len() > ffi::KMG_MAX_DEVICES {
            return Err(anyhow!("at most {} devices", ffi::KMG_MAX_DEVICES));
        }
        opt.n_devices = devices.len() as u32;
        opt.devices[..devices.len()].copy_from_slice(devices);
        let mut group = std::ptr::null_mut();
        check(unsafe { ffi::kmg_group_create(&opt, &mut group) })?;
        Ok(ImageProcessor { raw: std::ptr::null_mut(), group })
    }

    /// Alpha mode (`kmg_options.alpha_cutoff`, include/kmeans_hip.h): 0 ignores alpha as the reference does; 1..=255 lets
    /// only pixels whose alpha is at least `alpha_cutoff` shape the palette, and the outputs keep the input's alpha.  No
    /// counterpart in the reference.  A processor over several devices has no alpha mode.
    pub fn set_alpha_cutoff(&self, alpha_cutoff: u32) -> Result<()> {
        if !self.group.is_null() {
            return Err(anyhow!("a processor over several devices has no alpha mode"));
        }
        check(unsafe { ffi::kmg_processor_set_alpha_cutoff(self.raw, alpha_cutoff) })
    }

    /// The error-diffusion filter of `ReduceMode::Diffuse` (`kmg_processor_set_diffusion`, include/kmeans_hip.h at
    /// `kmg_diffusion`): one of `ffi::KMG_DIFFUSION_*`, 0 = Floyd-Steinberg, the default.  It holds for the outputs made from
    /// now on; the other modes ignore it.  No counterpart in the reference.  A processor over several devices has no such mode.
    pub fn set_diffusion(&self, filter: i32) -> Result<()> {
        if !self.group.is_null() {
            return Err(anyhow!("a processor over several devices has no diffusion mode"));
        }
        check(unsafe { ffi::kmg_processor_set_diffusion(self.raw, filter) })
    }

    /// The threshold map and the strength of `ReduceMode::Dither` (`kmg_processor_set_dither`, include/kmeans_hip.h at
    /// `kmg_dither_map`): one of the built-in `ffi::KMG_DITHER_*` maps and a factor 0 ..= 4 on the dither's amplitude;
    /// `KMG_DITHER_BAYER4` at 1.0, the reference's dither, is the default.  It holds for the outputs made from now on; the other
    /// modes ignore it.  No counterpart in the reference.  A processor over several devices dithers with the default only.
    pub fn set_dither(&self, map: i32, strength: f32) -> Result<()> {
        if !self.group.is_null() {
            return Err(anyhow!("a processor over several devices has no dither maps"));
        }
        check(unsafe { ffi::kmg_processor_set_dither(self.raw, map, strength) })
    }

    /// The same with the caller's own map (`kmg_processor_set_dither_custom`): `levels` holds `width * height` values below
    /// `n_levels`, row-major; each side is a power of two up to 64.
    pub fn set_dither_custom(&self, levels: &[u16], width: u32, height: u32, n_levels: u32, strength: f32) -> Result<()> {
        if !self.group.is_null() {
            return Err(anyhow!("a processor over several devices has no dither maps"));
        }
        if levels.len() as u64 != width as u64 * height as u64 {
            return Err(anyhow!("a dither map of {}x{} has {} levels, {} given", width, height, width as u64 * height as u64, levels.len()));
        }
        check(unsafe { ffi::kmg_processor_set_dither_custom(self.raw, levels.as_ptr(), width, height, n_levels, strength) })
    }

    /// Alpha weighting (`kmg_processor_set_weighting`, include/kmeans_hip.h): `true` lets every k-means palette of the calls that
    /// start from now on weigh a pixel by its alpha byte (pixels of alpha 0 do not shape it at all); `Algorithm::Octree` is then
    /// an error.  `false`, the default, weighs every kept pixel 1.  No counterpart in the reference.  A processor over several
    /// devices has none.
    pub fn set_alpha_weight(&self, on: bool) -> Result<()> {
        if !self.group.is_null() {
            return Err(anyhow!("a processor over several devices has no alpha weighting"));
        }
        check(unsafe { ffi::kmg_processor_set_weighting(self.raw, if on { 1 } else { 0 }) })
    }

    /// Fixed palette colours (`kmg_processor_set_fixed_colors`, include/kmeans_hip.h): every k-means palette of the calls that
    /// start from now on keeps `colors` exactly (alpha ignored), as entries `0..colors.len()` in index order, and places the
    /// others around them; an empty slice clears them.  `color_count` below the number of fixed colours and
    /// `Algorithm::Octree` are then errors.  No counterpart in the reference.  A processor over several devices has none.
    pub fn set_fixed_colors(&self, colors: &[RGBA8]) -> Result<()> {
        if !self.group.is_null() {
            return Err(anyhow!("a processor over several devices has no fixed colours"));
        }
        let list = if colors.is_empty() { std::ptr::null() } else { colors.as_ptr() as *const u8 };
        check(unsafe { ffi::kmg_processor_set_fixed_colors(self.raw, list, colors.len() as u32) })
    }

    /// lib.rs:67-77: `color_count` dominant colours, sorted by Lab lightness (k-means: exactly
    /// `color_count`; octree: at most).
    pub async fn palette<C: Container>(
        &self,
        color_count: u32,
        image: &Image<C>,
        algo: Algorithm,
    ) -> Result<Vec<RGBA8>> {
        let (width, height) = image.dimensions();
        let mut out = vec![RGBA8::default(); color_count.max(1) as usize];
        let mut count = 0u32;
        let (px, dst) = (image.as_bytes().as_ptr(), out.as_mut_ptr() as *mut u8);
        check(unsafe {
            if self.group.is_null() {
                ffi::kmg_palette(self.raw, px, width, height, color_count, algo.as_c(), dst, &mut count)
            } else {
                ffi::kmg_group_palette(self.group, px, width, height, color_count, algo.as_c(), dst, &mut count)
            }
        })?;
        out.truncate(count as usize);
        Ok(out)
    }

    /// lib.rs:79-114: every pixel replaced by (or dithered / melded towards) the closest of `colors`.
    pub async fn find<C: Container>(
        &self,
        image: &Image<C>,
        colors: &[RGBA8],
        reduce_mode: &ReduceMode,
    ) -> Result<Image<Vec<RGBA8>>> {
        let (width, height) = image.dimensions();
        let mut out = vec![RGBA8::default(); width as usize * height as usize];
        let (px, pal, dst) = (image.as_bytes().as_ptr(), colors.as_ptr() as *const u8, out.as_mut_ptr() as *mut u8);
        check(unsafe {
            if self.group.is_null() {
                ffi::kmg_find(self.raw, px, width, height, pal, colors.len() as u32, reduce_mode.as_c(), dst)
            } else {
                ffi::kmg_group_find(self.group, px, width, height, pal, colors.len() as u32, reduce_mode.as_c(), dst)
            }
        })?;
        Ok(Image::new((width, height), out))
    }

    /// lib.rs:116-164: palette extraction (`algo`) followed by `find` with that palette.
    pub async fn reduce<C: Container>(
        &self,
        color_count: u32,
        image: &Image<C>,
        algo: &Algorithm,
        reduce_mode: &ReduceMode,
    ) -> Result<Image<Vec<RGBA8>>> {
        let (width, height) = image.dimensions();
        let mut out = vec![RGBA8::default(); width as usize * height as usize];
        let (px, dst) = (image.as_bytes().as_ptr(), out.as_mut_ptr() as *mut u8);
        check(unsafe {
            if self.group.is_null() {
                ffi::kmg_reduce(self.raw, px, width, height, color_count, algo.as_c(), reduce_mode.as_c(), dst)
            } else {
                ffi::kmg_group_reduce(self.group, px, width, height, color_count, algo.as_c(), reduce_mode.as_c(), dst)
            }
        })?;
        Ok(Image::new((width, height), out))
    }
}

/// `kmg_error_stats`: exact integer error sums of an output against its source (include/kmeans_hip.h).
pub use ffi::kmg_error_stats as ErrorStats;

impl ErrorStats {
    /// root mean square dE76 on the 1/64 Lab grid
    pub fn delta_e_rms(&self) -> f64 {
        if self.pixels == 0 {
            return 0.0;
        }
        (self.lab_sse as f64 / (4096.0 * self.pixels as f64)).sqrt()
    }

    /// per-channel mean squared error (R, G, B)
    pub fn mse(&self) -> [f64; 3] {
        let n = self.pixels.max(1) as f64;
        [self.sse[0] as f64 / n, self.sse[1] as f64 / n, self.sse[2] as f64 / n]
    }
}

/// What `reduce_quality` returns: the colour count it chose, the palette in index order, the reduced image, the statistics of
/// the palette step's working image at that count, and whether the target was reached.
pub struct QualityReduction {
    pub color_count: u32,
    pub colors: Vec<RGBA8>,
    pub image: Image<Vec<RGBA8>>,
    pub achieved: ErrorStats,
    pub reached: bool,
}

impl ImageProcessor {
    fn single(&self) -> Result<*mut ffi::kmg_processor> {
        if !self.group.is_null() {
            return Err(anyhow!("error statistics need a single-device processor"));
        }
        Ok(self.raw)
    }

    /// `kmg_compare` of two RGBA8 images of the same size: RGB and Lab statistics over the pixels whose source alpha reaches the
    /// processor's alpha cutoff.  No counterpart in the reference.
    pub fn compare<C: Container, D: Container>(&self, source: &Image<C>, output: &Image<D>) -> Result<ErrorStats> {
        let (width, height) = source.dimensions();
        if output.dimensions() != (width, height) {
            return Err(anyhow!("compare: the images differ in size"));
        }
        let mut stats = ErrorStats::default();
        check(unsafe {
            ffi::kmg_compare(
                self.single()?,
                source.as_bytes().as_ptr(),
                output.as_bytes().as_ptr() as *const (),
                width,
                height,
                ffi::KMG_FORMAT_RGBA8,
                std::ptr::null(),
                0,
                ffi::KMG_ERROR_RGB | ffi::KMG_ERROR_LAB,
                &mut stats,
            )
        })?;
        Ok(stats)
    }

    /// `kmg_reduce_quality`: `reduce` with as few colours in `[k_min, k_max]` as keep the dE76 RMS of the shrunk image at or below
    /// `max_delta_e` (k-means only).  No counterpart in the reference.
    pub fn reduce_quality<C: Container>(
        &self,
        image: &Image<C>,
        max_delta_e: f64,
        k_min: u32,
        k_max: u32,
        reduce_mode: &ReduceMode,
    ) -> Result<QualityReduction> {
        let (width, height) = image.dimensions();
        let mut out = vec![RGBA8::default(); width as usize * height as usize];
        let mut colors = vec![RGBA8::default(); k_max.max(1) as usize];
        let target = (4096.0 * max_delta_e * max_delta_e).floor().clamp(0.0, u32::MAX as f64) as u32;
        let (mut count, mut reached, mut achieved) = (0u32, 0 as c_int, ErrorStats::default());
        check(unsafe {
            ffi::kmg_reduce_quality(
                self.single()?,
                image.as_bytes().as_ptr(),
                width,
                height,
                k_min,
                k_max,
                target,
                reduce_mode.as_c(),
                ffi::KMG_FORMAT_RGBA8,
                colors.as_mut_ptr() as *mut u8,
                &mut count,
                out.as_mut_ptr() as *mut (),
                &mut achieved,
                &mut reached,
            )
        })?;
        colors.truncate(count as usize);
        Ok(QualityReduction { color_count: count, colors, image: Image::new((width, height), out), achieved, reached: reached != 0 })
    }
}

impl Drop for ImageProcessor {
    fn drop(&mut self) {
        unsafe {
            if !self.group.is_null() {
                ffi::kmg_group_destroy(self.group)
            }
            ffi::kmg_processor_destroy(self.raw)
        }
    }
}

/// lib.rs:167-213.  Only `Lab` is reachable from the reference's public API (lib.rs:87,94,130,266); kept
/// because `cli/src/args.rs:131-137` converts into it.
#[derive(Clone, Copy)]
pub enum ColorSpace {
    Lab,
    Rgb,
}

impl ColorSpace {
    pub fn from(s: &str) -> Option<ColorSpace> {
        s.parse().ok()
    }

    pub fn name(&self) -> &'static str {
        match self {
            ColorSpace::Lab => "lab",
            ColorSpace::Rgb => "rgb",
        }
    }

    pub fn convergence(&self) -> f32 {
        match self {
            ColorSpace::Lab => 1.0,
            ColorSpace::Rgb => 0.01,
        }
    }
}

impl FromStr for ColorSpace {
    type Err = anyhow::Error;

    fn from_str(s: &str) -> Result<Self, Self::Err> {
        match s {
            "lab" => Ok(ColorSpace::Lab),
            "rgb" => Ok(ColorSpace::Rgb),
            other => Err(anyhow!("Unsupported color space {other}")),
        }
    }
}

impl Display for ColorSpace {
    fn fmt(&self, f: &mut std::fmt::Formatter<'_>) -> std::fmt::Result {
        f.write_str(self.name())
    }
}

/// lib.rs:215-232
#[derive(Clone, Copy)]
pub enum Algorithm {
    Kmeans,
    Octree,
}

impl Algorithm {
    fn as_c(&self) -> c_int {
        match self {
            Algorithm::Kmeans => ffi::KMG_ALGO_KMEANS,
            Algorithm::Octree => ffi::KMG_ALGO_OCTREE,
        }
    }
}

impl Display for Algorithm {
    fn fmt(&self, f: &mut std::fmt::Formatter<'_>) -> std::fmt::Result {
        f.write_str(match self {
            Algorithm::Kmeans => "kmeans",
            Algorithm::Octree => "octree",
        })
    }
}

/// lib.rs:234-253
#[derive(Clone, Copy)]
pub enum ReduceMode {
    Replace,
    Dither,
    Meld,
    /// Floyd-Steinberg error diffusion (KMG_MODE_DIFFUSE; not in the reference)
    Diffuse,
}

impl ReduceMode {
    fn as_c(&self) -> c_int {
        match self {
            ReduceMode::Replace => ffi::KMG_MODE_REPLACE,
            ReduceMode::Dither => ffi::KMG_MODE_DITHER,
            ReduceMode::Meld => ffi::KMG_MODE_MELD,
            ReduceMode::Diffuse => ffi::KMG_MODE_DIFFUSE,
        }
    }
}

impl Display for ReduceMode {
    fn fmt(&self, f: &mut std::fmt::Formatter<'_>) -> std::fmt::Result {
        f.write_str(match self {
            ReduceMode::Replace => "replace",
            ReduceMode::Dither => "dither",
            ReduceMode::Meld => "meld",
            ReduceMode::Diffuse => "diffuse",
        })
    }
}
