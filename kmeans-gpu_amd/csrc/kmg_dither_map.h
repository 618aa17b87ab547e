// kmg_dither_map.h -- the threshold maps of KMG_MODE_DITHER (include/kmeans_hip.h at kmg_dither_map): the limits
// and checks of a map and the choice a processor and a plan keep (the built-in tables: kmg_processor.hip).  Host only, no device.
#pragma once

#include <stdint.h>

#include <cmath>
#include <memory>
#include <vector>

#include "../../include/kmeans_hip.h"

namespace kmg {

constexpr uint32_t kDitherMapMaxSide = 64, kDitherMapMaxLevels = 65536;

// A map and a strength as a processor keeps them and a plan copies them.  A null DitherPtr is the default choice -- the reference's
// matrix at strength 1 through the kernels that carry it in their code; any other choice (a custom copy of that matrix included)
// goes through the map kernels.
struct DitherChoice {
    int map = KMG_DITHER_BAYER4;
    uint32_t mw = 4, mh = 4, n_levels = 16;
    float strength = 1.0f;
    std::vector<uint16_t> levels;   // mw x mh, row-major
    std::vector<float> v;           // (float)level / (float)n_levels - 0.5f
    float vmin = 0.0f, vmax = 0.0f; // the smallest and largest v
};
using DitherPtr = std::shared_ptr<const DitherChoice>;

inline bool dither_side_ok(uint32_t s) { return s >= 1u && s <= kDitherMapMaxSide && (s & (s - 1u)) == 0u; }
inline bool dither_strength_ok(float s) { return std::isfinite(s) && s >= 0.0f && s <= 4.0f; }

// the table of a built-in map (KMG_DITHER_BAYER4 .. KMG_DITHER_BLUE64; kmg_processor.hip); levels: room for 4096.  false: no such map
bool dither_builtin(int map, uint32_t *w, uint32_t *h, uint32_t *n_levels, uint16_t *levels);

// a checked map and strength as a choice: v in IEEE fp32, one division, one subtraction
inline DitherPtr dither_choice(int map, const uint16_t *levels, uint32_t w, uint32_t h, uint32_t n_levels, float strength)
{
    auto c = std::make_shared<DitherChoice>();
    c->map = map; c->mw = w; c->mh = h; c->n_levels = n_levels; c->strength = strength;
    c->levels.assign(levels, levels + (size_t)w * h);
    c->v.resize((size_t)w * h);
    for (size_t i = 0; i < c->v.size(); ++i) {
        volatile float q = (float)levels[i] / (float)n_levels;        // (volatile: the quotient is rounded to fp32 before the subtraction)
        c->v[i] = q - 0.5f;
    }
    c->vmin = c->vmax = c->v[0];
    for (const float x : c->v) { c->vmin = x < c->vmin ? x : c->vmin; c->vmax = x > c->vmax ? x : c->vmax; }
    return c;
}

}  // namespace kmg
