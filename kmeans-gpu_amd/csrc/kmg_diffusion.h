// kmg_diffusion.h -- the error-diffusion filters of KMG_MODE_DIFFUSE (kmg_diffusion in include/kmeans_hip.h), plain C++ with no
// device in it: kmg_diffusion_weights returns this table, and the kernels' arguments are derived from it (diffuse_filter).
#pragma once

#include <cstdint>

namespace kmg {

constexpr int kDiffusionCount = 8;

// weights[12]: [0..1] row 0 (dx = +1, +2), [2..6] row 1 (dx = -2 .. +2), [7..11] row 2 (dx = -2 .. +2); returns the divisor
// (0: no such filter, weights untouched)
inline int32_t diffusion_table(int filter, int32_t weights[12])
{
    static const int32_t table[kDiffusionCount][13] = {
        {16, 7, 0, 0, 3, 5, 1, 0, 0, 0, 0, 0, 0},                   // Floyd-Steinberg
        {4, 2, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0},                    // Sierra Lite (Sierra-2-4A)
        {8, 1, 1, 0, 1, 1, 1, 0, 0, 0, 1, 0, 0},                    // Atkinson (passes on 6/8 of the error)
        {32, 8, 4, 2, 4, 8, 4, 2, 0, 0, 0, 0, 0},                   // Burkes
        {16, 4, 3, 1, 2, 3, 2, 1, 0, 0, 0, 0, 0},                   // Sierra-2 (two-row Sierra)
        {32, 5, 3, 2, 4, 5, 4, 2, 0, 2, 3, 2, 0},                   // Sierra-3
        {48, 7, 5, 3, 5, 7, 5, 3, 1, 3, 5, 3, 1},                   // Jarvis, Judice and Ninke
        {42, 8, 4, 2, 4, 8, 4, 2, 1, 2, 4, 2, 1},                   // Stucki
    };
    if (filter < 0 || filter >= kDiffusionCount) return 0;
    for (int i = 0; i < 12; ++i) weights[i] = table[filter][1 + i];
    return table[filter][0];
}

}  // namespace kmg
