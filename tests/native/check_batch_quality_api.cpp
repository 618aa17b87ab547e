// Exercises the batched quality call of kmeans-gpu_amd/host/kmeans_color_gpu.hpp (ImageProcessor::reduce_quality_batch).
//   check_batch_quality_api nogpu   expects ImageProcessor::create() to fail loudly; with a device: a batch of three small images
//                                   must give what reduce_quality() gives image by image
#include <cstring>
#include <iostream>

#include "kmeans_color_gpu.hpp"

using namespace kmeans_color_gpu;

static Image synthetic(uint32_t w, uint32_t h, uint32_t seed, uint32_t levels)
{
    std::vector<RGBA8> px((size_t)w * h);
    uint32_t s = seed;
    for (RGBA8 &p : px) {
        s = s * 1664525u + 1013904223u;
        p.r = (uint8_t)(((s >> 24) % levels) * 255u / levels); p.g = (uint8_t)(((s >> 16) % levels) * 255u / levels);
        p.b = (uint8_t)(((s >> 8) % levels) * 255u / levels); p.a = 255;
    }
    return Image({w, h}, px);
}

static bool same(const ImageProcessor::Quality &a, const ImageProcessor::Quality &b)
{
    return a.indexed.dims == b.indexed.dims && a.indexed.format == b.indexed.format && a.indexed.index8 == b.indexed.index8 &&
           a.indexed.index16 == b.indexed.index16 && a.indexed.palette.size() == b.indexed.palette.size() &&
           (a.indexed.palette.empty() || !memcmp(a.indexed.palette.data(), b.indexed.palette.data(), a.indexed.palette.size() * 4)) &&
           !memcmp(&a.achieved, &b.achieved, sizeof a.achieved) && a.reached == b.reached;
}

int main(int argc, char **argv)
{
    if (argc < 2 || strcmp(argv[1], "nogpu")) { std::cerr << "usage\n"; return 2; }
    try {
        ImageProcessor p = ImageProcessor::create();
        const std::vector<Image> images = {synthetic(40, 30, 1, 2), synthetic(17, 90, 2, 3), synthetic(300, 20, 3, 256)};
        kmg_batch_quality_report report;
        const std::vector<ImageProcessor::Quality> got = p.reduce_quality_batch(images, 3.0, 2, 24, ReduceMode::Dither, false, 0, &report);
        for (size_t i = 0; i < images.size(); ++i) {
            if (!same(got[i], p.reduce_quality(images[i], 3.0, 2, 24, ReduceMode::Dither))) {
                std::cout << "mismatch " << i << "\n";
                return 1;
            }
        }
        if (report.batched + report.per_image != images.size() || report.rounds == 0 || report.sub_batches != 1) {
            std::cout << "report " << report.rounds << " " << report.batched << " " << report.per_image << "\n";
            return 1;
        }
        std::cout << "batch quality ok " << report.rounds << " rounds " << report.launches << " launches\n";
        return 0;
    } catch (const Error &e) {
        std::cout << "error " << e.status << " " << e.what() << "\n";
        return (e.status != KMG_OK && strlen(e.what()) > 0) ? 0 : 1;
    }
}
