// kmeans_color_gpu.hpp -- C++ host-side mirror of the reference crate's public API
// (core/src/lib.rs:24-165, core/src/image.rs) on top of the C ABI of include/kmeans_hip.h.
//
// Same names, argument meaning and error behaviour as the Rust crate `kmeans_color_gpu`:
//   ImageProcessor::new()                      -> ImageProcessor::create()   (throws on failure)
//   processor.palette(color_count, &image, algo)           -> std::vector<RGBA8>
//   processor.find(&image, &colors, &reduce_mode)          -> Image
//   processor.reduce(color_count, &image, &algo, &mode)    -> Image
// and, with no counterpart in the single-device reference (lib.rs:38-65 picks one adapter):
//   ImageProcessor::create_on({0, 1, ..})      -> the same object over a device LIST (kmg_group_*: one processor + RCCL rank per
//                                                 device; palette / find / reduce tile the image in row bands, same bytes)
//   processor.reduce_batch(color_count, images, algo, mode) -> whole images per device, side by side
//   processor.palette_batch(color_count, images, algo) / reduce_batch(color_count, images, algo, mode, max_resident_bytes)
//                                                          -> many small images per launch on one device (kmg_*_batch)
//   processor.reduce_quality_batch(images, max_delta_e, k_min, k_max, mode) -> reduce_quality of many small images, searched in lock step
//   processor.find_batch(images, colors, mode) / reduce_indexed_batch(color_count, images, algo, mode)
//                                                          -> their index maps, the output passes in one launch
//   processor.compare(source, output[, colors])         -> kmg_error_stats: exact error sums of an output against its source
//   processor.reduce_quality(image, max_delta_e, k_min, k_max, mode) -> the colour count chosen by a quality target
//   processor.optimize_indexed(indexed[, flags, bits])     -> the palette without unused entries, ordered, and the map packed for it
//   processor.set_fixed_colors(colors)                     -> palette entries the k-means keeps exactly and builds around
//   processor.set_alpha_weight(on)                         -> the k-means palette weighs every pixel by its alpha byte
//   Sequence seq(processor); seq.add(frame) ...; seq.output(k, mode, w, h); seq.frame(image) / seq.frame_lossy(image, delta_e)
//                                                          -> one palette for many frames, exact and lossy delta frames (kmg_sequence_*)
//   seq.begin_local(k, mode, w, h, warm); seq.frame_local(image) -> a palette per frame, colour-keyed delta frames
// `anyhow::Result` errors become kmeans_color_gpu::Error exceptions carrying the kmg_status and the
// library's message.  Header only; link with -lkmeans_hip.
#pragma once

#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../../include/kmeans_hip.h"

namespace kmeans_color_gpu {

struct RGBA8 {                      // rgb::RGBA8 re-export (lib.rs:3)
    uint8_t r, g, b, a;
    bool operator==(const RGBA8 &o) const { return r == o.r && g == o.g && b == o.b && a == o.a; }
};
static_assert(sizeof(RGBA8) == 4, "RGBA8 must be 4 tightly packed bytes");

enum class Algorithm { Kmeans = KMG_ALGO_KMEANS, Octree = KMG_ALGO_OCTREE };                  // lib.rs:215-219
enum class ReduceMode { Replace = KMG_MODE_REPLACE, Dither = KMG_MODE_DITHER, Meld = KMG_MODE_MELD, Diffuse = KMG_MODE_DIFFUSE };  // lib.rs:234-239

inline const char *to_string(Algorithm a) { return a == Algorithm::Kmeans ? "kmeans" : "octree"; }   // lib.rs:221-232
inline const char *to_string(ReduceMode m)                                                           // lib.rs:241-253
{
    return m == ReduceMode::Replace ? "replace" : m == ReduceMode::Dither ? "dither" : m == ReduceMode::Meld ? "meld" : "diffuse";
}

struct Error : std::runtime_error {
    int status;
    Error(int s, const std::string &msg) : std::runtime_error(msg), status(s) {}
};

// image.rs:20-48: tightly packed row-major RGBA8, dimensions = (width, height)
struct Image {
    std::pair<uint32_t, uint32_t> dims;
    std::vector<RGBA8> rgba;

    Image(std::pair<uint32_t, uint32_t> dimensions, std::vector<RGBA8> pixels)
        : dims(dimensions), rgba(std::move(pixels)) {}
    const RGBA8 &get_pixel(uint32_t x, uint32_t y) const { return rgba[(size_t)x + (size_t)y * dims.first]; }
    std::pair<uint32_t, uint32_t> dimensions() const { return dims; }
    std::vector<uint8_t> into_raw_pixels() const
    {
        const uint8_t *p = reinterpret_cast<const uint8_t *>(rgba.data());
        return std::vector<uint8_t>(p, p + rgba.size() * 4);
    }
};

// image.rs:50-64 copied_pixel
inline Image copied_pixel(std::pair<uint32_t, uint32_t> dimensions, const uint8_t *rgba_bytes)
{
    const RGBA8 *p = reinterpret_cast<const RGBA8 *>(rgba_bytes);
    return Image(dimensions, std::vector<RGBA8>(p, p + (size_t)dimensions.first * dimensions.second));
}

class ImageProcessor {
public:
    // lib.rs:38-65
    static ImageProcessor create() { return ImageProcessor(nullptr); }
    static ImageProcessor create(const kmg_options &opt) { return ImageProcessor(&opt); }
    // the same constructor over several devices of the node (HIP ordinals; empty = every visible device)
    static ImageProcessor create_on(const std::vector<int> &devices, const kmg_options *opt = nullptr, uint32_t flags = 0)
    {
        kmg_group_options go;
        kmg_default_group_options(&go);
        if (devices.size() > KMG_MAX_DEVICES) throw Error(KMG_ERR_INVALID_ARGUMENT, "too many devices");
        go.n_devices = (uint32_t)devices.size();
        for (size_t i = 0; i < devices.size(); ++i) go.devices[i] = devices[i];
        go.flags = flags;
        if (opt) go.processor = *opt;
        ImageProcessor p;
        check(kmg_group_create(&go, &p.g_));
        return p;
    }

    ImageProcessor(ImageProcessor &&o) noexcept : p_(o.p_), g_(o.g_) { o.p_ = nullptr; o.g_ = nullptr; }
    ImageProcessor &operator=(ImageProcessor &&o) noexcept
    {
        if (this != &o) { release(); p_ = o.p_; g_ = o.g_; o.p_ = nullptr; o.g_ = nullptr; }
        return *this;
    }
    ImageProcessor(const ImageProcessor &) = delete;
    ImageProcessor &operator=(const ImageProcessor &) = delete;
    ~ImageProcessor() { release(); }

    // lib.rs:67-77
    std::vector<RGBA8> palette(uint32_t color_count, const Image &image, Algorithm algo) const
    {
        std::vector<RGBA8> out(color_count ? color_count : 1);
        uint32_t n = 0;
        uint8_t *dst = reinterpret_cast<uint8_t *>(out.data());
        check(g_ ? kmg_group_palette(g_, bytes(image), image.dims.first, image.dims.second, color_count, (int)algo, dst, &n)
                 : kmg_palette(p_, bytes(image), image.dims.first, image.dims.second, color_count, (int)algo, dst, &n));
        out.resize(n);
        return out;
    }

    // lib.rs:79-114
    Image find(const Image &image, const std::vector<RGBA8> &colors, ReduceMode reduce_mode) const
    {
        Image out(image.dims, std::vector<RGBA8>(image.rgba.size()));
        const uint8_t *pal = reinterpret_cast<const uint8_t *>(colors.data());
        uint8_t *dst = reinterpret_cast<uint8_t *>(out.rgba.data());
        check(g_ ? kmg_group_find(g_, bytes(image), image.dims.first, image.dims.second, pal, (uint32_t)colors.size(), (int)reduce_mode, dst)
                 : kmg_find(p_, bytes(image), image.dims.first, image.dims.second, pal, (uint32_t)colors.size(), (int)reduce_mode, dst));
        return out;
    }

    // lib.rs:116-164
    Image reduce(uint32_t color_count, const Image &image, Algorithm algo, ReduceMode reduce_mode) const
    {
        Image out(image.dims, std::vector<RGBA8>(image.rgba.size()));
        uint8_t *dst = reinterpret_cast<uint8_t *>(out.rgba.data());
        check(g_ ? kmg_group_reduce(g_, bytes(image), image.dims.first, image.dims.second, color_count, (int)algo, (int)reduce_mode, dst)
                 : kmg_reduce(p_, bytes(image), image.dims.first, image.dims.second, color_count, (int)algo, (int)reduce_mode, dst));
        return out;
    }

    // palette-index output (include/kmeans_hip.h kmg_output_format; single-device processors only): one index per pixel, u8 when
    // the colours -- and the transparent slot of alpha mode -- fit a byte, else u16
    struct Indexed {
        std::pair<uint32_t, uint32_t> dims;
        int format = KMG_FORMAT_INDEX8;
        std::vector<uint8_t> index8;              // KMG_FORMAT_INDEX8
        std::vector<uint16_t> index16;            // KMG_FORMAT_INDEX16
        std::vector<RGBA8> palette;               // reduce_indexed: the colour of every index, in index order
        uint32_t at(uint32_t x, uint32_t y) const
        {
            const size_t i = (size_t)x + (size_t)y * dims.first;
            return format == KMG_FORMAT_INDEX8 ? index8[i] : index16[i];
        }
    };
    Indexed find_indexed(const Image &image, const std::vector<RGBA8> &colors, ReduceMode reduce_mode, bool alpha_mode = false) const
    {
        Indexed out = indexed_for(image, (uint32_t)colors.size(), alpha_mode);
        check(kmg_find_indexed(single(), bytes(image), image.dims.first, image.dims.second, reinterpret_cast<const uint8_t *>(colors.data()),
                               (uint32_t)colors.size(), (int)reduce_mode, out.format, index_data(out)));
        return out;
    }
    Indexed reduce_indexed(uint32_t color_count, const Image &image, Algorithm algo, ReduceMode reduce_mode, bool alpha_mode = false) const
    {
        Indexed out = indexed_for(image, color_count, alpha_mode);
        out.palette.resize(color_count ? color_count : 1);
        uint32_t n = 0;
        check(kmg_reduce_indexed(single(), bytes(image), image.dims.first, image.dims.second, color_count, (int)algo, (int)reduce_mode,
                                 out.format, reinterpret_cast<uint8_t *>(out.palette.data()), &n, index_data(out)));
        out.palette.resize(n);
        return out;
    }

    // error statistics (include/kmeans_hip.h kmg_error_stats; single-device processors only): exact integer sums and maxima of
    // an output against its source, over the pixels whose source alpha reaches the processor's alpha_cutoff
    kmg_error_stats compare(const Image &source, const Image &output, uint32_t what = KMG_ERROR_RGB | KMG_ERROR_LAB) const
    {
        if (source.dims != output.dims) throw Error(KMG_ERR_INVALID_ARGUMENT, "compare: the images differ in size");
        kmg_error_stats s;
        check(kmg_compare(single(), bytes(source), bytes(output), source.dims.first, source.dims.second, KMG_FORMAT_RGBA8, nullptr, 0, what, &s));
        return s;
    }
    // ... of an index map against its source: `colors` is the palette the indices point into (Indexed::palette of reduce_indexed
    // and reduce_quality, the caller's palette for find_indexed)
    kmg_error_stats compare(const Image &source, const Indexed &output, const std::vector<RGBA8> &colors,
                            uint32_t what = KMG_ERROR_RGB | KMG_ERROR_LAB) const
    {
        if (source.dims != output.dims) throw Error(KMG_ERR_INVALID_ARGUMENT, "compare: the images differ in size");
        kmg_error_stats s;
        const void *idx = output.format == KMG_FORMAT_INDEX8 ? static_cast<const void *>(output.index8.data())
                                                             : static_cast<const void *>(output.index16.data());
        check(kmg_compare(single(), bytes(source), idx, source.dims.first, source.dims.second, output.format,
                          reinterpret_cast<const uint8_t *>(colors.data()), (uint32_t)colors.size(), what, &s));
        return s;
    }
    static double delta_e_rms(const kmg_error_stats &s) { return s.pixels ? std::sqrt((double)s.lab_sse / (4096.0 * (double)s.pixels)) : 0.0; }

    // kmg_reduce_quality: as few colours in [k_min, k_max] as keep the dE76 RMS of the palette step's working image at or below
    // max_delta_e (target = floor(4096 max_delta_e^2)); k-means only.  The index map and its palette are those of
    // reduce_indexed(k) for the k chosen; `achieved` = the statistics of the working image at that k.
    struct Quality {
        Indexed indexed;
        kmg_error_stats achieved;
        bool reached = false;
    };
    Quality reduce_quality(const Image &image, double max_delta_e, uint32_t k_min, uint32_t k_max, ReduceMode reduce_mode,
                           bool alpha_mode = false) const
    {
        Quality q;
        q.indexed = indexed_for(image, k_max, alpha_mode);
        q.indexed.palette.resize(k_max ? k_max : 1);
        const double t = std::floor(4096.0 * max_delta_e * max_delta_e);
        const uint32_t target = t >= 4294967295.0 ? 0xFFFFFFFFu : (t > 0.0 ? (uint32_t)t : 0u);
        uint32_t n = 0;
        int reached = 0;
        check(kmg_reduce_quality(single(), bytes(image), image.dims.first, image.dims.second, k_min, k_max, target, (int)reduce_mode,
                                 q.indexed.format, reinterpret_cast<uint8_t *>(q.indexed.palette.data()), &n, index_data(q.indexed), &q.achieved,
                                 &reached));
        q.indexed.palette.resize(n);
        q.reached = reached != 0;
        return q;
    }

    // kmg_index_optimize (single-device processors only): the palette of an index map without the entries no pixel uses, in the
    // order `flags` asks for (KMG_INDEX_*), and the map rewritten for it -- packed rows of info.bits (or `bits`) per pixel, every row
    // starting on a byte, as a PNG of colour type 3 stores them.  palette[info.transparent] is (0, 0, 0, 0) when the slot is there.
    struct Optimized {
        std::pair<uint32_t, uint32_t> dims;
        kmg_index_plan_info info;
        uint32_t bits = 0;                        // bits per pixel of `rows`
        size_t stride = 0;                        // bytes per row: ceil(width * bits / 8)
        std::vector<uint8_t> rows;                // stride * height bytes (bits = 16: uint16_t values in host order)
        std::vector<RGBA8> palette;               // info.n_slots entries in the new index order
    };
    Optimized optimize_indexed(const Indexed &indexed, uint32_t flags = KMG_INDEX_ORDER_USAGE | KMG_INDEX_TRANSPARENT_FIRST,
                               uint32_t bits = 0) const
    {
        Optimized out;
        out.dims = indexed.dims;
        const size_t n = (size_t)indexed.dims.first * indexed.dims.second;
        const void *idx = indexed.format == KMG_FORMAT_INDEX8 ? static_cast<const void *>(indexed.index8.data())
                                                              : static_cast<const void *>(indexed.index16.data());
        out.rows.resize(n * (indexed.format == KMG_FORMAT_INDEX8 ? 1u : 2u));
        out.palette.resize(indexed.palette.size() + 1);
        check(kmg_index_optimize(single(), idx, indexed.format, indexed.dims.first, indexed.dims.second,
                                 reinterpret_cast<const uint8_t *>(indexed.palette.data()), (uint32_t)indexed.palette.size(), flags, bits,
                                 reinterpret_cast<uint8_t *>(out.palette.data()), &out.info, out.rows.data()));
        out.bits = bits ? bits : out.info.bits;
        out.stride = ((size_t)indexed.dims.first * out.bits + 7u) / 8u;
        out.rows.resize(out.stride * indexed.dims.second);
        out.palette.resize(out.info.n_slots);
        return out;
    }

    // a batch: whole images per device (a single-device processor takes them one after the other)
    std::vector<Image> reduce_batch(uint32_t color_count, const std::vector<Image> &images, Algorithm algo, ReduceMode reduce_mode) const
    {
        std::vector<Image> out;
        for (const Image &im : images) out.emplace_back(im.dims, std::vector<RGBA8>(im.rgba.size()));
        if (!g_) {
            for (size_t i = 0; i < images.size(); ++i) out[i] = reduce(color_count, images[i], algo, reduce_mode);
            return out;
        }
        std::vector<const uint8_t *> src;
        std::vector<uint8_t *> dst;
        std::vector<uint32_t> ws, hs;
        for (size_t i = 0; i < images.size(); ++i) {
            src.push_back(bytes(images[i])); dst.push_back(reinterpret_cast<uint8_t *>(out[i].rgba.data()));
            ws.push_back(images[i].dims.first); hs.push_back(images[i].dims.second);
        }
        check(kmg_group_reduce_batch(g_, (uint32_t)images.size(), src.data(), ws.data(), hs.data(), color_count, (int)algo, (int)reduce_mode,
                                     dst.data()));
        return out;
    }

    // Many small images per launch on a single-device processor (kmg_palette_batch / kmg_reduce_batch, include/kmeans_hip.h): the
    // palettes / results that palette() / reduce() give image by image, from one launch chain for all of them.  max_resident_bytes
    // bounds what the call keeps on the device at once (0 = 1 GiB); report: what the call did.  The batch must not be empty.
    std::vector<std::vector<RGBA8>> palette_batch(uint32_t color_count, const std::vector<Image> &images, Algorithm algo,
                                                  uint64_t max_resident_bytes = 0, kmg_batch_report *report = nullptr) const
    {
        std::vector<std::vector<RGBA8>> out(images.size(), std::vector<RGBA8>(color_count ? color_count : 1));
        std::vector<const uint8_t *> src;
        std::vector<uint8_t *> dst;
        std::vector<uint32_t> ws, hs, counts(images.size() ? images.size() : 1);
        for (size_t i = 0; i < images.size(); ++i) {
            src.push_back(bytes(images[i])); dst.push_back(reinterpret_cast<uint8_t *>(out[i].data()));
            ws.push_back(images[i].dims.first); hs.push_back(images[i].dims.second);
        }
        check(kmg_palette_batch(single(), (uint32_t)images.size(), src.data(), ws.data(), hs.data(), color_count, (int)algo, max_resident_bytes,
                                dst.data(), counts.data(), report));
        for (size_t i = 0; i < images.size(); ++i) out[i].resize(counts[i]);
        return out;
    }

    std::vector<Image> reduce_batch(uint32_t color_count, const std::vector<Image> &images, Algorithm algo, ReduceMode reduce_mode,
                                    uint64_t max_resident_bytes, kmg_batch_report *report = nullptr) const
    {
        std::vector<Image> out;
        std::vector<const uint8_t *> src;
        std::vector<uint8_t *> dst;
        std::vector<uint32_t> ws, hs;
        for (const Image &im : images) out.emplace_back(im.dims, std::vector<RGBA8>(im.rgba.size()));
        for (size_t i = 0; i < images.size(); ++i) {
            src.push_back(bytes(images[i])); dst.push_back(reinterpret_cast<uint8_t *>(out[i].rgba.data()));
            ws.push_back(images[i].dims.first); hs.push_back(images[i].dims.second);
        }
        check(kmg_reduce_batch(single(), (uint32_t)images.size(), src.data(), ws.data(), hs.data(), color_count, (int)algo, (int)reduce_mode,
                               max_resident_bytes, dst.data(), report));
        return out;
    }

    // Batched output on a single-device processor (kmg_find_batch / kmg_reduce_indexed_batch, include/kmeans_hip.h): what
    // find_indexed() / reduce_indexed() give image by image, the output passes of the images in one launch.  apply_report (and
    // batch_report, the palettes' chain): what the call did.  The batch must not be empty.
    std::vector<Indexed> find_batch(const std::vector<Image> &images, const std::vector<RGBA8> &colors, ReduceMode reduce_mode,
                                    bool alpha_mode = false, uint64_t max_resident_bytes = 0, kmg_batch_apply_report *apply_report = nullptr) const
    {
        std::vector<Indexed> out;
        std::vector<const uint8_t *> src;
        std::vector<void *> dst;
        std::vector<uint32_t> ws, hs;
        for (const Image &im : images) out.push_back(indexed_for(im, (uint32_t)colors.size(), alpha_mode));
        for (size_t i = 0; i < images.size(); ++i) {
            src.push_back(bytes(images[i])); dst.push_back(index_data(out[i]));
            ws.push_back(images[i].dims.first); hs.push_back(images[i].dims.second);
        }
        const int format = images.empty() ? KMG_FORMAT_INDEX8 : out[0].format;
        check(kmg_find_batch(single(), (uint32_t)images.size(), src.data(), ws.data(), hs.data(), reinterpret_cast<const uint8_t *>(colors.data()),
                             (uint32_t)colors.size(), (int)reduce_mode, format, max_resident_bytes, dst.data(), apply_report));
        return out;
    }

    std::vector<Indexed> reduce_indexed_batch(uint32_t color_count, const std::vector<Image> &images, Algorithm algo, ReduceMode reduce_mode,
                                              bool alpha_mode = false, uint64_t max_resident_bytes = 0, kmg_batch_report *batch_report = nullptr,
                                              kmg_batch_apply_report *apply_report = nullptr) const
    {
        std::vector<Indexed> out;
        std::vector<const uint8_t *> src;
        std::vector<void *> dst;
        std::vector<uint8_t *> pals;
        std::vector<uint32_t> ws, hs, counts(images.size() ? images.size() : 1);
        for (const Image &im : images) {
            out.push_back(indexed_for(im, color_count, alpha_mode));
            out.back().palette.resize(color_count ? color_count : 1);
        }
        for (size_t i = 0; i < images.size(); ++i) {
            src.push_back(bytes(images[i])); dst.push_back(index_data(out[i]));
            pals.push_back(reinterpret_cast<uint8_t *>(out[i].palette.data()));
            ws.push_back(images[i].dims.first); hs.push_back(images[i].dims.second);
        }
        const int format = images.empty() ? KMG_FORMAT_INDEX8 : out[0].format;
        check(kmg_reduce_indexed_batch(single(), (uint32_t)images.size(), src.data(), ws.data(), hs.data(), color_count, (int)algo, (int)reduce_mode,
                                       format, max_resident_bytes, pals.data(), counts.data(), dst.data(), batch_report, apply_report));
        for (size_t i = 0; i < images.size(); ++i) out[i].palette.resize(counts[i]);
        return out;
    }

    // kmg_reduce_quality_batch (include/kmeans_hip.h): reduce_quality() of many small images on a single-device processor, every
    // round of their searches one launch chain -- image by image what reduce_quality gives.  report: what the call did.  The batch
    // must not be empty.
    std::vector<Quality> reduce_quality_batch(const std::vector<Image> &images, double max_delta_e, uint32_t k_min, uint32_t k_max,
                                              ReduceMode reduce_mode, bool alpha_mode = false, uint64_t max_resident_bytes = 0,
                                              kmg_batch_quality_report *report = nullptr) const
    {
        std::vector<Quality> out(images.size());
        std::vector<const uint8_t *> src;
        std::vector<void *> dst;
        std::vector<uint8_t *> pals;
        std::vector<uint32_t> ws, hs, counts(images.size() ? images.size() : 1);
        std::vector<kmg_error_stats> achieved(images.size() ? images.size() : 1);
        std::vector<int> reached(images.size() ? images.size() : 1, 0);
        for (size_t i = 0; i < images.size(); ++i) {
            out[i].indexed = indexed_for(images[i], k_max, alpha_mode);
            out[i].indexed.palette.resize(k_max ? k_max : 1);
            src.push_back(bytes(images[i])); dst.push_back(index_data(out[i].indexed));
            pals.push_back(reinterpret_cast<uint8_t *>(out[i].indexed.palette.data()));
            ws.push_back(images[i].dims.first); hs.push_back(images[i].dims.second);
        }
        const double t = std::floor(4096.0 * max_delta_e * max_delta_e);
        const uint32_t target = t >= 4294967295.0 ? 0xFFFFFFFFu : (t > 0.0 ? (uint32_t)t : 0u);
        const int format = images.empty() ? KMG_FORMAT_INDEX8 : out[0].indexed.format;
        check(kmg_reduce_quality_batch(single(), (uint32_t)images.size(), src.data(), ws.data(), hs.data(), k_min, k_max, target, (int)reduce_mode,
                                       format, max_resident_bytes, pals.data(), counts.data(), dst.data(), achieved.data(), reached.data(), report));
        for (size_t i = 0; i < images.size(); ++i) {
            out[i].indexed.palette.resize(counts[i]);
            out[i].achieved = achieved[i];
            out[i].reached = reached[i] != 0;
        }
        return out;
    }

    // kmg_options.alpha_cutoff of a single-device processor (0 = alpha ignored, 1..255 = alpha mode; include/kmeans_hip.h).  Set
    // it at creation through create(opt) or here; a processor over several devices has no alpha mode.
    void set_alpha_cutoff(uint32_t alpha_cutoff) const
    {
        if (g_) throw Error(KMG_ERR_INVALID_ARGUMENT, "a processor over several devices has no alpha mode");
        check(kmg_processor_set_alpha_cutoff(p_, alpha_cutoff));
    }

    // kmg_processor_set_diffusion (include/kmeans_hip.h at kmg_diffusion): the error-diffusion filter of ReduceMode::Diffuse for the
    // outputs made from now on (KMG_DIFFUSION_FLOYD_STEINBERG is the default); the other modes ignore it.  A processor over
    // several devices has no such mode.
    void set_diffusion(int filter) const
    {
        if (g_) throw Error(KMG_ERR_INVALID_ARGUMENT, "a processor over several devices has no diffusion mode");
        check(kmg_processor_set_diffusion(p_, filter));
    }

    // kmg_processor_set_dither (include/kmeans_hip.h at kmg_dither_map): a built-in threshold map (KMG_DITHER_*) and the strength
    // (0 .. 4) of ReduceMode::Dither for the outputs made from now on; KMG_DITHER_BAYER4 at 1, the reference's dither, is the
    // default, and the other modes ignore both.  A processor over several devices dithers with the default only.
    void set_dither(int map, float strength = 1.0f) const
    {
        if (g_) throw Error(KMG_ERR_INVALID_ARGUMENT, "a processor over several devices has no dither maps");
        check(kmg_processor_set_dither(p_, map, strength));
    }

    // kmg_processor_set_dither_custom: the same with the caller's own map -- width x height levels below n_levels, row-major, each
    // side a power of two up to 64
    void set_dither(const std::vector<uint16_t> &levels, uint32_t width, uint32_t height, uint32_t n_levels, float strength = 1.0f) const
    {
        if (g_) throw Error(KMG_ERR_INVALID_ARGUMENT, "a processor over several devices has no dither maps");
        if (levels.size() != (size_t)width * height) throw Error(KMG_ERR_INVALID_ARGUMENT, "the dither map's levels do not match its sides");
        check(kmg_processor_set_dither_custom(p_, levels.data(), width, height, n_levels, strength));
    }

    // kmg_dither_map_values: the table of a built-in map (no device needed), row-major; the sides and n_levels through the pointers
    static std::vector<uint16_t> dither_map_values(int map, uint32_t *width, uint32_t *height, uint32_t *n_levels)
    {
        std::vector<uint16_t> levels(4096);
        uint32_t w = 0, h = 0, n = 0;
        check(kmg_dither_map_values(map, &w, &h, &n, levels.data()));
        levels.resize((size_t)w * h);
        if (width) *width = w;
        if (height) *height = h;
        if (n_levels) *n_levels = n;
        return levels;
    }

    // kmg_processor_set_fixed_colors (include/kmeans_hip.h): colours every k-means palette of the calls that start from now on keeps
    // exactly (alpha ignored), as entries 0 .. colors.size() - 1 in index order; an empty list clears them.  A color_count below
    // their number and Algorithm::Octree are then errors.  A processor over several devices has no fixed colours.
    void set_fixed_colors(const std::vector<RGBA8> &colors) const
    {
        if (g_) throw Error(KMG_ERR_INVALID_ARGUMENT, "a processor over several devices has no fixed colours");
        check(kmg_processor_set_fixed_colors(p_, colors.empty() ? nullptr : reinterpret_cast<const uint8_t *>(colors.data()),
                                             (uint32_t)colors.size()));
    }

    // kmg_processor_set_weighting (include/kmeans_hip.h): on = the k-means palette steps of the calls that start from now on weigh every
    // pixel by its alpha byte (KMG_WEIGHT_ALPHA) and keep the pixels with alpha >= max(alpha_cutoff, 1); Algorithm::Octree is then an
    // error.  off = every kept pixel weighs 1 (KMG_WEIGHT_NONE, the default).  A processor over several devices has no weighting.
    void set_alpha_weight(bool on) const
    {
        if (g_) throw Error(KMG_ERR_INVALID_ARGUMENT, "a processor over several devices has no alpha weighting");
        check(kmg_processor_set_weighting(p_, on ? KMG_WEIGHT_ALPHA : KMG_WEIGHT_NONE));
    }

    kmg_processor *handle() const { return g_ ? kmg_group_processor(g_, 0) : p_; }
    kmg_group *group() const { return g_; }

private:
    ImageProcessor() : p_(nullptr), g_(nullptr) {}
    explicit ImageProcessor(const kmg_options *opt) : p_(nullptr), g_(nullptr)
    {
        check(opt ? kmg_processor_create_ex(opt, &p_) : kmg_processor_create(&p_));
    }
    void release()
    {
        if (g_) kmg_group_destroy(g_);
        kmg_processor_destroy(p_);
        g_ = nullptr; p_ = nullptr;
    }
    static const uint8_t *bytes(const Image &im) { return reinterpret_cast<const uint8_t *>(im.rgba.data()); }
    kmg_processor *single() const
    {
        if (g_) throw Error(KMG_ERR_INVALID_ARGUMENT, "index output and error statistics need a single-device processor");
        return p_;
    }
    static Indexed indexed_for(const Image &image, uint32_t k, bool alpha_mode)
    {
        Indexed out;
        out.dims = image.dims;
        out.format = k + (alpha_mode ? 1u : 0u) <= 256u ? KMG_FORMAT_INDEX8 : KMG_FORMAT_INDEX16;
        if (out.format == KMG_FORMAT_INDEX8) out.index8.resize(image.rgba.size());
        else out.index16.resize(image.rgba.size());
        return out;
    }
    static void *index_data(Indexed &o)
    {
        return o.format == KMG_FORMAT_INDEX8 ? static_cast<void *>(o.index8.data()) : static_cast<void *>(o.index16.data());
    }
    static void check(int rc)
    {
        if (rc != KMG_OK) throw Error(rc, kmg_last_error());
    }
    kmg_processor *p_;
    kmg_group *g_;
};

// Frame sequences (include/kmeans_hip.h kmg_sequence; single-device processors only, which outlive their sequences): one palette for
// all frames added, then every frame as an INDEX8 map (k <= 255; index k is the transparent slot) -- a delta map against what is
// shown, or the full map when a shown pixel turns transparent.  frame_lossy: a pixel whose source stays within max_delta_e (dE76) of
// the source it was last written for keeps what it shows (kmg_sequence_output_frame_lossy, tolerance = rint(4096 max_delta_e^2)); exact
// and lossy frames may alternate.  Not re-entrant: one thread at a time per sequence.
class Sequence {
public:
    struct Frame {
        std::vector<uint8_t> map;     // width x height indices: the delta map, or -- is_full -- the full map
        kmg_frame_hold info;          // an exact frame leaves held = held_sse = 0
        bool is_full = false;
    };
    explicit Sequence(const ImageProcessor &processor) : s_(nullptr)
    {
        if (processor.group()) throw Error(KMG_ERR_INVALID_ARGUMENT, "a sequence needs a single-device processor");
        check(kmg_sequence_create(processor.handle(), &s_));
    }
    ~Sequence() { kmg_sequence_destroy(s_); }
    Sequence(const Sequence &) = delete;
    Sequence &operator=(const Sequence &) = delete;

    void add(const Image &image) { check(kmg_sequence_add(s_, reinterpret_cast<const uint8_t *>(image.rgba.data()), image.dims.first, image.dims.second)); }
    // opens the frame output; returns the palette in index order
    std::vector<RGBA8> output(uint32_t color_count, ReduceMode reduce_mode, uint32_t width, uint32_t height)
    {
        std::vector<RGBA8> palette(color_count ? color_count : 1);
        uint32_t n = 0;
        check(kmg_sequence_output_begin(s_, color_count, (int)reduce_mode, KMG_FORMAT_INDEX8, width, height,
                                        reinterpret_cast<uint8_t *>(palette.data()), &n));
        palette.resize(n);
        pixels_ = (size_t)width * height;
        return palette;
    }
    Frame frame(const Image &image, bool delta = true)
    {
        Frame f = start(image);
        kmg_frame_delta rec = {0, 0, 0xFFFFFFFFu, 0xFFFFFFFFu, 0, 0};
        int full = 1;
        check(kmg_sequence_output_frame(s_, reinterpret_cast<const uint8_t *>(image.rgba.data()), delta ? KMG_FRAME_DELTA : 0u, f.map.data(), &rec, &full));
        f.info = kmg_frame_hold{rec.changed, rec.cleared, rec.x0, rec.y0, rec.x1, rec.y1, 0, 0};
        f.is_full = full != 0;
        return f;
    }
    Frame frame_lossy(const Image &image, double max_delta_e)
    {
        const double t = std::nearbyint(4096.0 * max_delta_e * max_delta_e);
        if (!(max_delta_e >= 0.0) || t > 4294967295.0) throw Error(KMG_ERR_INVALID_ARGUMENT, "frame_lossy: the tolerance does not fit 32 bits");
        Frame f = start(image);
        int full = 0;
        check(kmg_sequence_output_frame_lossy(s_, reinterpret_cast<const uint8_t *>(image.rgba.data()), KMG_FRAME_DELTA, (uint32_t)t, f.map.data(),
                                              &f.info, &full));
        f.is_full = full != 0;
        return f;
    }
    // A whole clip in one launch chain (kmg_sequence_output_frames): frame by frame what frame() (max_delta_e empty) or frame_lossy()
    // (one tolerance for all frames, or one per frame) return for the images one after another, and the same state afterwards.
    std::vector<Frame> frames(const std::vector<Image> &images, bool delta = true, const std::vector<double> &max_delta_e = {},
                              uint64_t max_resident_bytes = 0, kmg_clip_report *report = nullptr)
    {
        const size_t n = images.size();
        if (!max_delta_e.empty() && max_delta_e.size() != 1 && max_delta_e.size() != n)
            throw Error(KMG_ERR_INVALID_ARGUMENT, "frames: one tolerance, or one per frame");
        std::vector<uint32_t> tol;
        for (size_t t = 0; !max_delta_e.empty() && t < n; ++t) {
            const double e = max_delta_e[max_delta_e.size() == 1 ? 0 : t], q = std::nearbyint(4096.0 * e * e);
            if (!(e >= 0.0) || q > 4294967295.0) throw Error(KMG_ERR_INVALID_ARGUMENT, "frames: the tolerance does not fit 32 bits");
            tol.push_back((uint32_t)q);
        }
        std::vector<Frame> out;
        std::vector<const uint8_t *> src;
        std::vector<void *> dst;
        for (const Image &image : images) {
            out.push_back(start(image));
            src.push_back(reinterpret_cast<const uint8_t *>(image.rgba.data()));
        }
        for (Frame &f : out) dst.push_back(f.map.data());
        std::vector<kmg_frame_hold> info(n ? n : 1, kmg_frame_hold{0, 0, 0xFFFFFFFFu, 0xFFFFFFFFu, 0, 0, 0, 0});
        std::vector<int> full(n ? n : 1, 1);
        check(kmg_sequence_output_frames(s_, (uint32_t)n, src.data(), delta ? KMG_FRAME_DELTA : 0u, max_delta_e.empty() ? nullptr : tol.data(),
                                         max_resident_bytes, dst.data(), info.data(), full.data(), report));
        for (size_t t = 0; t < n; ++t) {
            out[t].info = info[t];
            out[t].is_full = full[t] != 0;
        }
        return out;
    }
    // Per-frame palettes (kmg_sequence_output_begin_local): no frame needs to be added.  warm: the k-means of every frame after the
    // first starts from the previous frame's centroids.  frame_local: the frame's own palette in index order and its map -- a delta
    // map against what is shown (exact, or lossy within max_delta_e when that is >= 0), or the full map.
    struct LocalFrame : Frame {
        std::vector<RGBA8> palette;
    };
    void begin_local(uint32_t color_count, ReduceMode reduce_mode, uint32_t width, uint32_t height, bool warm = false)
    {
        pixels_ = 0;
        check(kmg_sequence_output_begin_local(s_, color_count, (int)reduce_mode, KMG_FORMAT_INDEX8, width, height, warm ? KMG_LOCAL_WARM : 0u));
        pixels_ = (size_t)width * height;
        colors_ = color_count;
    }
    LocalFrame frame_local(const Image &image, bool delta = true, double max_delta_e = -1.0)
    {
        const bool lossy = max_delta_e >= 0.0;
        const double t = lossy ? std::nearbyint(4096.0 * max_delta_e * max_delta_e) : 0.0;
        if (max_delta_e != max_delta_e || t > 4294967295.0) throw Error(KMG_ERR_INVALID_ARGUMENT, "frame_local: the tolerance does not fit 32 bits");
        LocalFrame f;
        static_cast<Frame &>(f) = start(image);
        f.palette.resize(colors_);
        const uint32_t tol = (uint32_t)t;
        uint32_t n = 0;
        int full = 1;
        check(kmg_sequence_output_frame_local(s_, reinterpret_cast<const uint8_t *>(image.rgba.data()), delta ? KMG_FRAME_DELTA : 0u,
                                              lossy ? &tol : nullptr, f.map.data(), reinterpret_cast<uint8_t *>(f.palette.data()), &n, &f.info, &full));
        f.palette.resize(n);
        f.is_full = full != 0;
        return f;
    }
    void end_output() { pixels_ = 0; check(kmg_sequence_output_end(s_)); }
    kmg_sequence *handle() const { return s_; }

private:
    Frame start(const Image &image) const
    {
        if (!pixels_) throw Error(KMG_ERR_INVALID_ARGUMENT, "no output is open (Sequence::output)");
        if (image.rgba.size() != pixels_) throw Error(KMG_ERR_INVALID_ARGUMENT, "the frame does not have the size the output was opened for");
        Frame f;
        f.map.resize(pixels_);
        return f;
    }
    static void check(int rc)
    {
        if (rc != KMG_OK) throw Error(rc, kmg_last_error());
    }
    kmg_sequence *s_;
    size_t pixels_ = 0;
    uint32_t colors_ = 0;
};

}  // namespace kmeans_color_gpu
