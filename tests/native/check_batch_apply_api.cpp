// Exercises the batched output calls of kmeans-gpu_amd/host/kmeans_color_gpu.hpp (ImageProcessor::find_batch /
// reduce_indexed_batch).
//   check_batch_apply_api nogpu   expects ImageProcessor::create() to fail loudly; with a device: a batch of three small images
//                                 must give what find_indexed() / reduce_indexed() give image by image
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

static bool same(const ImageProcessor::Indexed &a, const ImageProcessor::Indexed &b)
{
    return a.dims == b.dims && a.format == b.format && a.index8 == b.index8 && a.index16 == b.index16 && a.palette.size() == b.palette.size() &&
           (a.palette.empty() || !memcmp(a.palette.data(), b.palette.data(), a.palette.size() * 4));
}

int main(int argc, char **argv)
{
    if (argc < 2 || strcmp(argv[1], "nogpu")) { std::cerr << "usage\n"; return 2; }
    try {
        ImageProcessor p = ImageProcessor::create();
        const std::vector<Image> images = {synthetic(40, 30, 1), synthetic(17, 90, 2), synthetic(300, 20, 3)};
        const std::vector<RGBA8> colors = synthetic(6, 1, 4).rgba;
        kmg_batch_apply_report found, reduced;
        kmg_batch_report palettes;
        const std::vector<ImageProcessor::Indexed> maps = p.find_batch(images, colors, ReduceMode::Dither, false, 0, &found);
        const std::vector<ImageProcessor::Indexed> pairs =
            p.reduce_indexed_batch(6, images, Algorithm::Kmeans, ReduceMode::Dither, false, 0, &palettes, &reduced);
        for (size_t i = 0; i < images.size(); ++i) {
            if (!same(maps[i], p.find_indexed(images[i], colors, ReduceMode::Dither)) ||
                !same(pairs[i], p.reduce_indexed(6, images[i], Algorithm::Kmeans, ReduceMode::Dither))) {
                std::cout << "mismatch " << i << "\n";
                return 1;
            }
        }
        if (found.batched != images.size() || reduced.batched != images.size() || found.per_image || reduced.per_image) {
            std::cout << "reports " << found.batched << " " << reduced.batched << "\n";
            return 1;
        }
        std::cout << "batch apply ok " << found.launches + reduced.launches << " launches\n";
        return 0;
    } catch (const Error &e) {
        std::cout << "error " << e.status << " " << e.what() << "\n";
        return (e.status != KMG_OK && strlen(e.what()) > 0) ? 0 : 1;
    }
}
