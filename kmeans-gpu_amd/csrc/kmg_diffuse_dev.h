// kmg_diffuse_dev.h -- what the two schedules of KMG_MODE_DIFFUSE share (kmg_diffuse.hip: Floyd-Steinberg; kmg_diffuse_wide.hip:
// the filters that reach two columns or two rows): the per-call control block, the heartbeat, the bounded wait on the chunk above,
// the nearest colour of a quantised value by route, and the packed error word.  The text is the one kmg_diffuse.hip had; it stays
// in an unnamed namespace, so each translation unit keeps its own copy and k_diffuse keeps its code.
#pragma once

#include "../../include/kmeans_hip.h"
#include "kmg_device.h"
#include "kmg_table.h"

namespace kmg {

// a filter of kmg_diffuse_wide.hip as its kernel takes it
struct DiffuseFilter {
    int32_t w[12];                 // kmg_diffusion_weights' order
    uint32_t bias, magic;          // floor((S + D/2) / D) = umulhi(S + bias, magic) - 4096: bias = D/2 + 4096 D, magic = ceil(2^32 / D)
    int skew;                      // columns a row lags the row above: 3 when the filter takes e(x + 2, .) of a row above, else 2
};
// launch_diffuse (kmg_kernels.h) for the filters other than Floyd-Steinberg; it calls this
hipError_t launch_diffuse_wide(int route, int filter, const uint32_t *rgba, uint32_t w, uint32_t rows, void *out, int format, void *erow,
                               uint32_t parity, void *ctl, uint32_t *sticky, const Centroid *cent, uint32_t k, const float *lut,
                               const uint32_t *pal, const void *colour_labels, const uint16_t *sub_table, hipStream_t st, uint32_t alpha_cutoff);

namespace {

constexpr int kBody = 16;                          // columns per unrolled body: source block, output block, publish batch
constexpr uint64_t kSpinTicks = 50000000ull;       // 0.5 s at the 100 MHz s_memrealtime clock, measured from the last progress
constexpr uint32_t kPairsLds = kCells + 128 + 256;         // pair table, direction words, palette (u32)
constexpr uint32_t kCellsLds = kCells / 2 + 3072;          // 8x8x8 summaries (u16 pairs), palette (u32)

struct DiffCtl {
    uint32_t ticket;
    uint32_t timeout;
    uint32_t pad[2];
    unsigned long long prog[kDiffuseRing];         // slot t % ring: (t + 1) << 32 | columns of chunk t's last row published
    unsigned long long beat[kDiffuseRing];         // slot t % ring: (t + 1) << 32 | heartbeat count of chunk t
};

__device__ __forceinline__ void heartbeat(DiffCtl *ctl, uint32_t t, uint32_t &beats)
{
    beats += 1u;
    if (threadIdx.x == 0)
        __hip_atomic_store(&ctl->beat[t % kDiffuseRing], ((unsigned long long)(t + 1u) << 32) | beats, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ uint2 pack_err(int r, int g, int b)
{
    return make_uint2(((uint32_t)r & 0xFFFFu) | ((uint32_t)g << 16), (uint32_t)b);
}

// nearest palette entry of an opaque colour px = r | g << 8 | b << 16: the replace pass's label
template <int ROUTE>
__device__ __forceinline__ uint32_t diffuse_label(uint32_t px, const uint32_t *s_lds, const float4 *s_cent, const float *s_lut,
                                                  uint32_t k, const void *colour_labels, const uint16_t *sub_table, bool active)
{
    if (ROUTE == kDiffusePairs) {
        // k <= 256: k_labels_pairs (kmg_table.hip) -- the cell's pair entry in LDS, the per-colour byte where the plane says "fine"
        const uint32_t *s_pair = s_lds, *s_dir = s_lds + kCells;
        const uint32_t ci = colour_index(px);
        const uint32_t xyz = (px & 0x00070707u) | 0x01000000u;
        const uint32_t e = s_pair[ci >> 9];
        const uint32_t dirw = s_dir[(e >> 16) & 127u];
        const int proj = __builtin_amdgcn_sdot4((int)xyz, (int)dirw, 0, false);
        const int tlo = (int)((e >> 23) & 63u), w = (int)(e >> 29);
        const bool inA = proj < tlo, inB = proj >= tlo + w + (w == 7 ? 64 : 0);
        uint32_t lab = inA ? (e & 0xFFu) : ((e >> 8) & 0xFFu);
        if (active && !(inA || inB)) lab = (uint32_t)static_cast<const uint8_t *>(colour_labels)[ci];
        return lab;
    } else if (ROUTE == kDiffuseCells) {
        // k > 256: k_labels (kmg_table.hip) -- 8x8x8 summary in LDS, 4x4x4 summary, per-colour label
        const uint16_t *s_cell = reinterpret_cast<const uint16_t *>(s_lds);
        const uint32_t ci = colour_index(px);
        uint32_t lab = s_cell[ci >> 9];
        if (active && lab == kSubMixed) lab = sub_table[ci >> 6];
        if (active && lab == kSubMixed) lab = static_cast<const uint16_t *>(colour_labels)[ci];
        return active ? lab : 0u;
    } else {
        // per-lane scan: the key arg-min with the near-tie repair of argmin_scan (kmg_kernels.hip), i.e. find_centroid.wgsl's
        // first minimum of the literal distance
        float L, a, b;
        px_to_lab(s_lut, px, L, a, b);
        const PixelTerms pt = pixel_terms(L, a, b);
        float best = 3.0e38f, second = 3.0e38f;
        uint32_t idx = 0;
        for (uint32_t j = 0; j < k; ++j) {
            const float4 c = s_cent[j];
            const float d = cie94_key(pt, c.x, c.y, c.z, c.w);
            const bool lt = d < best;
            second = __builtin_amdgcn_fmed3f(d, best, second);
            best = lt ? d : best;
            idx = lt ? j : idx;
        }
        const float thr = tie_threshold(best);
        if (active && second <= thr) {
            float bd = 3.0e38f;
            uint32_t bj = 0;
            for (uint32_t j = 0; j < k; ++j) {
                const float4 c = s_cent[j];
                if (cie94_key(pt, c.x, c.y, c.z, c.w) <= thr) {
                    const float d = cie94_c(pt.L, pt.a, pt.b, pt.C, c.x, c.y, c.z, c.w);
                    if (d < bd) { bd = d; bj = j; }
                }
            }
            idx = bd < 100000.0f ? bj : 0u;                  // find_centroid.wgsl:29-30
        }
        return idx;
    }
}

__device__ __forceinline__ bool timed_out(const DiffCtl *ctl)
{
    return __hip_atomic_load(&ctl->timeout, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u;
}

// Wait until chunk t - 1 has published `need` columns of its last row.  Relaxed polls, one acquire after; the clock restarts
// whenever the predecessor's progress or heartbeat changes, and each such change is passed on as a beat of this chunk.  false:
// the pass is abandoned (this wave timed out, or another one did).
__device__ bool wait_progress(DiffCtl *ctl, uint32_t *sticky, uint32_t t, uint32_t need, uint32_t &known, uint32_t &beats)
{
    const unsigned long long *slot = &ctl->prog[(t - 1u) % kDiffuseRing];
    const unsigned long long *bslot = &ctl->beat[(t - 1u) % kDiffuseRing];
    uint64_t since = __builtin_amdgcn_s_memrealtime();
    unsigned long long seen = 0;
    for (;;) {
        const unsigned long long v = __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const uint32_t cols = (uint32_t)(v >> 32) == t ? (uint32_t)v : 0u;   // (another tag: an older chunk's word, nothing yet)
        if (cols >= need) { known = cols; break; }
        const unsigned long long b = __hip_atomic_load(bslot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned long long beat = (uint32_t)(b >> 32) == t ? b : 0ull;
        const uint64_t now = __builtin_amdgcn_s_memrealtime();
        if (cols > known || beat != seen) {                            // the pass moves: restart the clock, tell the next chunk
            known = cols > known ? cols : known;
            seen = beat;
            since = now;
            heartbeat(ctl, t, beats);
        }
        if (timed_out(ctl)) return false;
        if (now - since > kSpinTicks) {
            __hip_atomic_store(&ctl->timeout, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(sticky, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            return false;
        }
        __builtin_amdgcn_s_sleep(2);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    return true;
}

}  // namespace

}  // namespace kmg
