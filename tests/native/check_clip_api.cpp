// Exercises Sequence::frames of kmeans-gpu_amd/host/kmeans_color_gpu.hpp (kmg_sequence_output_frames).
//   check_clip_api nogpu   expects ImageProcessor::create() to fail loudly; with a device: a clip of nine frames, exact and lossy,
//                          cut into pieces and not, must give what frame() / frame_lossy() give one frame at a time on a twin
//                          sequence of a second processor, and leave the same state
#include <cstring>
#include <iostream>

#include "kmeans_color_gpu.hpp"

using namespace kmeans_color_gpu;

static Image synthetic(uint32_t w, uint32_t h, uint32_t t)
{
    std::vector<RGBA8> px((size_t)w * h);
    uint32_t s = 12345u;
    for (size_t i = 0; i < px.size(); ++i) {
        s = s * 1664525u + 1013904223u;
        RGBA8 &p = px[i];
        // a still scene with a little noise and a block that moves with t
        const uint32_t x = (uint32_t)(i % w), y = (uint32_t)(i / w), noise = (s >> 24) & 1u;
        p.r = (uint8_t)(40 + 5 * (x / 4) + noise); p.g = (uint8_t)(60 + 7 * (y / 4)); p.b = (uint8_t)(90 + noise * ((t + x) & 1u)); p.a = 255;
        if (x >= 3 * t && x < 3 * t + 6 && y >= 2 && y < 9) { p.r = 250; p.g = 20; p.b = 30; }
    }
    return Image({w, h}, px);
}

static bool same(const Sequence::Frame &a, const Sequence::Frame &b)
{
    return a.map == b.map && a.is_full == b.is_full && !memcmp(&a.info, &b.info, sizeof a.info);
}

int main(int argc, char **argv)
{
    if (argc < 2 || strcmp(argv[1], "nogpu")) { std::cerr << "usage\n"; return 2; }
    try {
        ImageProcessor p = ImageProcessor::create(), q = ImageProcessor::create();
        const uint32_t w = 31, h = 17, k = 9;
        std::vector<Image> clip;
        for (uint32_t t = 0; t < 9; ++t) clip.push_back(synthetic(w, h, t));
        uint32_t launches = 0;
        for (int lossy = 0; lossy < 2; ++lossy) {
            for (uint64_t bound : {(uint64_t)0, (uint64_t)3 * w * h * 6}) {
                Sequence seq(p), twin(q);
                for (const Image &f : clip) { seq.add(f); twin.add(f); }
                seq.output(k, ReduceMode::Dither, w, h);
                twin.output(k, ReduceMode::Dither, w, h);
                kmg_clip_report rep;
                const std::vector<Sequence::Frame> got = seq.frames(clip, true, lossy ? std::vector<double>{3.0} : std::vector<double>{}, bound, &rep);
                for (size_t t = 0; t < clip.size(); ++t)
                    if (!same(got[t], lossy ? twin.frame_lossy(clip[t], 3.0) : twin.frame(clip[t]))) {
                        std::cout << "mismatch " << lossy << " " << bound << " " << t << "\n";
                        return 1;
                    }
                if (!same(seq.frame_lossy(clip[1], 2.0), twin.frame_lossy(clip[1], 2.0))) { std::cout << "state " << lossy << "\n"; return 1; }
                if (rep.batched + rep.per_image != clip.size() || rep.sub_clips != (bound ? 3u : 1u)) {
                    std::cout << "report " << rep.batched << " " << rep.per_image << " " << rep.sub_clips << "\n";
                    return 1;
                }
                launches += rep.launches;
            }
        }
        std::cout << "clip ok " << launches << " launches\n";
        return 0;
    } catch (const Error &e) {
        std::cout << "error " << e.status << " " << e.what() << "\n";
        return (e.status != KMG_OK && strlen(e.what()) > 0) ? 0 : 1;
    }
}
