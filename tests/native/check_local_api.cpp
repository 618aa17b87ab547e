// A three-frame sequence with a palette per frame through the C++ mirror (kmeans_color_gpu.hpp Sequence::begin_local / frame_local):
//   check_local_api <frames.rgba> <width> <height> <k> <out.bin>
// frames.rgba holds three frames of width x height RGBA8.  Frame 0 and 1 are exact delta frames, frame 2 is lossy at dE76 2.0; the
// output is warm.  out.bin: per frame u32 n, n x 4 palette bytes, width x height indices, the 48-byte record, one byte is_full.
#include <cstdio>
#include <vector>

#include "kmeans_color_gpu.hpp"

using namespace kmeans_color_gpu;

int main(int argc, char **argv)
{
    if (argc != 6) return 2;
    const uint32_t w = (uint32_t)atoi(argv[2]), h = (uint32_t)atoi(argv[3]), k = (uint32_t)atoi(argv[4]);
    const size_t n = (size_t)w * h;
    std::vector<uint8_t> raw(3 * n * 4);
    FILE *f = fopen(argv[1], "rb");
    if (!f || fread(raw.data(), 1, raw.size(), f) != raw.size()) return 3;
    fclose(f);
    try {
        ImageProcessor proc = ImageProcessor::create();
        Sequence seq(proc);
        seq.begin_local(k, ReduceMode::Dither, w, h, true);
        FILE *o = fopen(argv[5], "wb");
        if (!o) return 4;
        for (int t = 0; t < 3; ++t) {
            const Image img = copied_pixel({w, h}, raw.data() + t * n * 4);
            const Sequence::LocalFrame fr = t < 2 ? seq.frame_local(img) : seq.frame_local(img, true, 2.0);
            const uint32_t np = (uint32_t)fr.palette.size();
            const uint8_t full = fr.is_full ? 1 : 0;
            fwrite(&np, 4, 1, o);
            fwrite(fr.palette.data(), 4, np, o);
            fwrite(fr.map.data(), 1, n, o);
            fwrite(&fr.info, sizeof fr.info, 1, o);
            fwrite(&full, 1, 1, o);
        }
        fclose(o);
        // the two kinds of output stay apart
        int refused = 0;
        try { seq.frame(copied_pixel({w, h}, raw.data())); } catch (const Error &e) { refused += e.status == KMG_ERR_INVALID_ARGUMENT; }
        seq.end_output();
        printf("ok refused %d\n", refused);
    } catch (const Error &e) {
        printf("error %d %s\n", e.status, e.what());
        return 1;
    }
    return 0;
}
