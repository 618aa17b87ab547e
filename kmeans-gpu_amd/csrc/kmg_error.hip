// kmg_error.hip -- quantisation error statistics (kmg_error_stats, include/kmeans_hip.h): how far an output is
// from its source, as exact integer sums and maxima.
//
//   k_error_palette  the q triples of a palette, (rint(64 L), rint(64 a), rint(64 b)) of the device's own rgb_to_lab, once per call:
//                    entry i = (palette word, qL, qa, qb), 16 bytes
//   k_error_stats    one template over the output's form (RGBA8 words; u8 / u16 indices; u32 labels, the quality search's own) and
//                    over `what` (the Lab arithmetic is not compiled into the RGB-only instantiations), on the skeleton of
//                    kmg_pass.h.  A lane takes four consecutive pixels per tile: one 16-byte source load and one 16- / 4- / 8- /
//                    16-byte output load.  Index forms: the palette (and its q triples) are staged once per workgroup in LDS.
//                    Accumulators are 32-bit where a run cannot overflow them (see kErrLanePixels) and leave the workgroup as
//                    64-bit atomics: at most 14 x 2048 per launch.
// A pixel that is not counted (out of range, alpha below the cutoff, invalid index) is compared with itself: it adds zero to
// every sum and maximum without a branch per field.

#include "kmg_internal.h"
#include "kmg_pass.h"

namespace kmg {

namespace {

constexpr uint32_t kErrFields = 14;                     // kmg_error_stats as 14 x u64
// n < 2^32 pixels are at most 2^22 tiles; a full grid gives a workgroup at most 2^22 / 2048 = 2048 of them, a lane 8192 pixels:
// its 32-bit sums reach 8192 x 255^2 = 5.3e8 < 2^32.  (The Lab sum, up to 2^29 per pixel, is 64-bit.)
constexpr uint64_t kErrLanePixels = 8192;
static_assert(kErrLanePixels * 255u * 255u < 0xFFFFFFFFull, "per-lane 32-bit sums");

enum { fPixels = 0, fChanged = 1, fInvalid = 2, fSse = 3, fSad = 6, fMax = 9, fLabSse = 12, fLabMax = 13 };

__host__ __device__ constexpr bool field_is_max(uint32_t f) { return (f >= fMax && f < fMax + 3) || f == fLabMax; }

__global__ __launch_bounds__(kPassBlock) void k_error_palette(const uint32_t *__restrict__ pal, uint32_t k, const float *__restrict__ lut,
                                                            int4 *__restrict__ entries)
{
    __shared__ float s_lut[256];
    s_lut[threadIdx.x] = lut[threadIdx.x];
    __syncthreads();
    const uint32_t i = blockIdx.x * kPassBlock + threadIdx.x;
    if (i >= k) return;
    const uint32_t px = pal[i];
    int32_t q[3];
    px_to_q(s_lut, px, q);
    entries[i] = make_int4((int)px, q[0], q[1], q[2]);
}

// four consecutive output elements as words: RGBA8 words / u32 labels (16-byte load), u8 (4-byte) or u16 (8-byte) indices
template <int FORM>
__device__ __forceinline__ void load4_out(const void *out, uint64_t i0, uint64_t n, bool aligned, uint32_t v[4])
{
    if (FORM == kErrorIndex8) load4_index<uint8_t, true>(static_cast<const uint8_t *>(out), i0, n, aligned, v);
    else if (FORM == kErrorIndex16) load4_index<uint16_t, true>(static_cast<const uint16_t *>(out), i0, n, aligned, v);
    else load4_stream(static_cast<const uint32_t *>(out), i0, n, aligned, v);
}

template <int FORM, uint32_t WHAT>
__global__ __launch_bounds__(kPassBlock) void k_error_stats(const uint32_t *__restrict__ src, const void *__restrict__ out, uint64_t n,
                                                          const uint32_t *__restrict__ pal, const int4 *__restrict__ entries, uint32_t k,
                                                          uint32_t cutoff, const float *__restrict__ lut,
                                                          unsigned long long *__restrict__ stats, int aligned)
{
    constexpr bool RGB = (WHAT & KMG_ERROR_RGB) != 0, LAB = (WHAT & KMG_ERROR_LAB) != 0, INDEXED = FORM != kErrorRgba8;
    extern __shared__ uint4 s_dyn[];                            // index forms: k words, or -- LAB -- k (word, qL, qa, qb) entries
    __shared__ float s_lut[LAB ? 256 : 1];
    __shared__ unsigned long long s_part[kPassWaves][kErrFields];
    const uint32_t *s_pal = reinterpret_cast<const uint32_t *>(s_dyn);
    const int4 *s_ent = reinterpret_cast<const int4 *>(s_dyn);
    if (LAB) s_lut[threadIdx.x] = lut[threadIdx.x];
    if (INDEXED) {
        if (LAB) for (uint32_t i = threadIdx.x; i < k; i += kPassBlock) reinterpret_cast<int4 *>(s_dyn)[i] = entries[i];
        else for (uint32_t i = threadIdx.x; i < k; i += kPassBlock) reinterpret_cast<uint32_t *>(s_dyn)[i] = pal[i];
    }
    if (LAB || INDEXED) __syncthreads();

    uint32_t pixels = 0, changed = 0, invalid = 0, lab_max = 0;
    uint32_t sse[3] = {0u, 0u, 0u}, sad[3] = {0u, 0u, 0u}, mx[3] = {0u, 0u, 0u};
    unsigned long long lab_sse = 0;

    uint64_t t0, t1;
    tile_run((n + kPassTile - 1) / kPassTile, t0, t1);
    uint32_t ns[4] = {0u, 0u, 0u, 0u}, no[4] = {0u, 0u, 0u, 0u};
    if (t0 < t1) {
        const uint64_t i0 = t0 * kPassTile + (uint64_t)threadIdx.x * 4u;
        load4_stream(src, i0, n, aligned != 0, ns);
        load4_out<FORM>(out, i0, n, aligned != 0, no);
    }
    for (uint64_t t = t0; t < t1; ++t) {
        const uint64_t i0 = t * kPassTile + (uint64_t)threadIdx.x * 4u;
        const uint32_t ps[4] = {ns[0], ns[1], ns[2], ns[3]}, po[4] = {no[0], no[1], no[2], no[3]};
        if (t + 1 < t1) {                                       // the next tile, in flight meanwhile
            load4_stream(src, i0 + kPassTile, n, aligned != 0, ns);
            load4_out<FORM>(out, i0 + kPassTile, n, aligned != 0, no);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint32_t s = ps[q];
            const bool counted = i0 + (uint64_t)q < n && (s >> 24) >= cutoff;
            bool valid = true;
            uint32_t o = po[q];
            int4 e = make_int4(0, 0, 0, 0);
            if (INDEXED) {
                valid = o < k;
                const uint32_t idx = valid ? o : 0u;
                if (LAB) { e = s_ent[idx]; o = (uint32_t)e.x; }
                else o = s_pal[idx];
            }
            const bool use = counted && valid;
            pixels += use ? 1u : 0u;
            invalid += (counted && !valid) ? 1u : 0u;
            o = use ? o : s;                                    // a pixel that does not count is compared with itself
            const bool differs = ((s ^ o) & 0x00FFFFFFu) != 0u;
            changed += differs ? 1u : 0u;
            if (RGB) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const int d = (int)((s >> (8 * c)) & 255u) - (int)((o >> (8 * c)) & 255u);
                    const uint32_t ad = (uint32_t)(d < 0 ? -d : d);
                    sse[c] += ad * ad;
                    sad[c] += ad;
                    mx[c] = max(mx[c], ad);
                }
            }
            if (LAB) {
                if (differs) {                                  // equal colours have equal q: the term is 0
                    int32_t qs[3], qo[3];
                    px_to_q(s_lut, s, qs);
                    if (INDEXED) { qo[0] = e.y; qo[1] = e.z; qo[2] = e.w; }
                    else px_to_q(s_lut, o, qo);
                    const int32_t dL = qs[0] - qo[0], da = qs[1] - qo[1], db = qs[2] - qo[2];
                    const uint32_t term = (uint32_t)(dL * dL) + (uint32_t)(da * da) + (uint32_t)(db * db);   // < 2^29
                    lab_sse += term;
                    lab_max = max(lab_max, term);
                }
            }
        }
    }

    unsigned long long v[kErrFields];
    v[fPixels] = pixels; v[fChanged] = changed; v[fInvalid] = invalid;
#pragma unroll
    for (int c = 0; c < 3; ++c) { v[fSse + c] = sse[c]; v[fSad + c] = sad[c]; v[fMax + c] = mx[c]; }
    v[fLabSse] = lab_sse; v[fLabMax] = lab_max;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
    for (uint32_t f = 0; f < kErrFields; ++f) {
        const bool wanted = f < fSse || (f < fLabSse ? RGB : LAB);
        if (!wanted) continue;
        unsigned long long x = v[f];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long y = __shfl_xor(x, o);
            x = field_is_max(f) ? max(x, y) : x + y;
        }
        if (lane == 0) s_part[wave][f] = x;
    }
    __syncthreads();
    if (threadIdx.x < kErrFields) {
        const uint32_t f = threadIdx.x;
        const bool wanted = f < fSse || (f < fLabSse ? RGB : LAB);
        if (wanted) {
            unsigned long long x = 0;
#pragma unroll
            for (uint32_t w = 0; w < kPassWaves; ++w) x = field_is_max(f) ? max(x, s_part[w][f]) : x + s_part[w][f];
            if (x != 0) {                                       // (adding 0 or maxing with 0 changes nothing)
                if (field_is_max(f)) atomicMax(stats + f, x);
                else atomicAdd(stats + f, x);
            }
        }
    }
}

}  // namespace

size_t error_palette_bytes(uint32_t k) { return sizeof(int4) * (size_t)k; }

hipError_t launch_error_palette(const uint32_t *pal, uint32_t k, const float *lut, void *entries, hipStream_t st)
{
    hipLaunchKernelGGL(k_error_palette, dim3((k + kPassBlock - 1) / kPassBlock), dim3(kPassBlock), 0, st, pal, k, lut, static_cast<int4 *>(entries));
    return hipGetLastError();
}

hipError_t launch_error_stats(int form, uint32_t what, const uint32_t *src, const void *out, uint64_t n, const uint32_t *pal,
                              const void *entries, uint32_t k, uint32_t cutoff, const float *lut, unsigned long long *stats, hipStream_t st)
{
    const uint32_t grid = pass_grid((n + kPassTile - 1) / kPassTile);
    // the vector loads: the source 16-byte aligned, the output for its own (RGBA8 words and u32 labels 16, u8 4, u16 8 bytes)
    const uintptr_t out_mask = form == kErrorIndex8 ? 3u : (form == kErrorIndex16 ? 7u : 15u);
    const int aligned = ((reinterpret_cast<uintptr_t>(src) & 15u) == 0 && (reinterpret_cast<uintptr_t>(out) & out_mask) == 0) ? 1 : 0;
    const bool lab = (what & KMG_ERROR_LAB) != 0;
    const size_t lds = form == kErrorRgba8 ? 0 : (size_t)k * (lab ? sizeof(int4) : sizeof(uint32_t));
    bool launched = false;                                            // (stays false for a form or `what` that does not exist)
    with_value<kErrorRgba8, kErrorIndex8, kErrorIndex16, kErrorLabel32>(form, [&](auto F) {
        with_value<KMG_ERROR_RGB, KMG_ERROR_LAB, KMG_ERROR_RGB | KMG_ERROR_LAB>((int)what, [&](auto W) {
            hipLaunchKernelGGL((k_error_stats<F(), W()>), dim3(grid), dim3(kPassBlock), lds, st, src, out, n, pal,
                               static_cast<const int4 *>(entries), k, cutoff, lut, stats, aligned);
            launched = true;
        });
    });
    return launched ? hipGetLastError() : hipErrorInvalidValue;
}

}  // namespace kmg
