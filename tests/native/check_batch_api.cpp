// Exercises the batch calls of kmeans-gpu_amd/host/kmeans_color_gpu.hpp (ImageProcessor::palette_batch / reduce_batch).
//   check_batch_api nogpu     expects ImageProcessor::create() to fail loudly; with a device: a batch of three small images must
//                             give what palette() / reduce() give image by image
#include <cstring>
#include <iostream>

#include "kmeans_color_gpu.hpp"

using namespace kmeans_color_gpu;

static Image synthetic(uint32_t w, uint32_t h, uint32_t seed)
{
    std::vector<RGBA8> px((size_t)w * h);
    uint32_t s = seed;
    for (RGBA8 &p : px) {
        s = s * 1664525u + 1013904223u;
        p.r = (uint8_t)(s >> 24); p.g = (uint8_t)(s >> 16); p.b = (uint8_t)(s >> 8); p.a = 255;
    }
    return Image({w, h}, px);
}

int main(int argc, char **argv)
{
    if (argc < 2 || strcmp(argv[1], "nogpu")) { std::cerr << "usage\n"; return 2; }
    try {
        ImageProcessor p = ImageProcessor::create();
        const std::vector<Image> images = {synthetic(40, 30, 1), synthetic(17, 90, 2), synthetic(300, 20, 3)};
        kmg_batch_report report;
        const std::vector<std::vector<RGBA8>> palettes = p.palette_batch(6, images, Algorithm::Kmeans, 0, &report);
        const std::vector<Image> reduced = p.reduce_batch(6, images, Algorithm::Kmeans, ReduceMode::Dither, 0);
        for (size_t i = 0; i < images.size(); ++i) {
            const std::vector<RGBA8> one = p.palette(6, images[i], Algorithm::Kmeans);
            const Image red = p.reduce(6, images[i], Algorithm::Kmeans, ReduceMode::Dither);
            if (one.size() != palettes[i].size() || memcmp(one.data(), palettes[i].data(), one.size() * 4) ||
                memcmp(red.rgba.data(), reduced[i].rgba.data(), red.rgba.size() * 4)) {
                std::cout << "mismatch " << i << "\n";
                return 1;
            }
        }
        std::cout << "batch ok " << report.launches << " launches\n";
        return 0;
    } catch (const Error &e) {
        std::cout << "error " << e.status << " " << e.what() << "\n";
        return (e.status != KMG_OK && strlen(e.what()) > 0) ? 0 : 1;
    }
}
