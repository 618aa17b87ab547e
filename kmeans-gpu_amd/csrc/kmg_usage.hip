// kmg_usage.hip -- index-map optimisation (kmg_dev_index_usage, kmg_index_plan, kmg_dev_index_remap and their host-buffer calls,
// include/kmeans_hip.h): which palette entries a map uses, a new order without the unused ones, and the map
// rewritten for it at 1, 2, 4, 8 or 16 bits per pixel.  All integers.
//
//   k_index_usage    one template over the index type (u8 / u16), on the skeleton of kmg_pass.h.  A lane takes four consecutive
//                    indices per tile (one 4- / 8-byte non-temporal load, the next tile's in flight).  k + 2 bins of u32 live in LDS;
//                    an index above k goes to bin k + 1.  Real maps are long runs of one value, and 64 lanes adding to one LDS
//                    address serialise, so equal values are combined before the atomic: a lane merges its own consecutive equal
//                    indices; a wave whose 256 indices all agree adds nothing at all but extends a run it keeps in registers; up
//                    to two further values that whole lanes agree on leave the wave as one add of 4 x the population count each.
//                    The workgroup ends with one u64 vector atomic per NON-ZERO bin: at most (k + 2) x 2048 per launch.
//   k_index_remap    one template over the input type and the output's bits.  The table (k + 1 u16) is staged in LDS.  8 / 16 bits:
//                    four pixels per lane, one load and one store each.  1 / 2 / 4 bits: a lane owns four consecutive output
//                    bytes of ONE row (32 / 16 / 8 pixels) and writes them as one dword where the address allows, byte by byte
//                    with bounds at a row's tail or a misaligned address; no output byte has two writers.  Bad pixels are counted
//                    per lane and leave the workgroup as one atomic when there are any.
// The plan between the two passes is host arithmetic (kmg_index_plan.h).

#include <string.h>

#include <type_traits>
#include <vector>

#include "kmg_index_plan.h"
#include "kmg_pass.h"
#include "kmg_state.h"

namespace kmg {

namespace {

// n < 2^32 pixels are at most 2^22 tiles; a full grid gives a workgroup at most 2^22 / 2048 = 2048 of them, 2^21 pixels: a
// workgroup's u32 bins, a wave's run counter and a lane's count of bad pixels cannot overflow.
constexpr uint64_t kUsageGroupPixels = (uint64_t)kPassTile * 2048u;
static_assert(kUsageGroupPixels < 0xFFFFFFFFull, "per-workgroup 32-bit bins");
constexpr unsigned long long kWholeWave = ~0ull;

template <typename T>
__global__ __launch_bounds__(kPassBlock) void k_index_usage(const T *__restrict__ index, uint64_t n, uint32_t k, int aligned,
                                                           unsigned long long *__restrict__ usage)
{
    extern __shared__ uint4 s_dyn[];                            // k + 2 bins
    uint32_t *s_bins = reinterpret_cast<uint32_t *>(s_dyn);
    const uint32_t n_bins = k + 2u;
    for (uint32_t i = threadIdx.x; i < n_bins; i += kPassBlock) s_bins[i] = 0u;
    __syncthreads();

    uint64_t t0, t1;
    tile_run((n + kPassTile - 1) / kPassTile, t0, t1);
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t run_bin = 0u, run_cnt = 0u;                        // the same in every lane of a wave: pixels of a run not yet in LDS
    uint32_t nx[4] = {0u, 0u, 0u, 0u};
    if (t0 < t1) load4_index<T, true>(index, t0 * kPassTile + (uint64_t)threadIdx.x * 4u, n, aligned != 0, nx);
    for (uint64_t t = t0; t < t1; ++t) {
        const uint64_t i0 = t * kPassTile + (uint64_t)threadIdx.x * 4u;
        uint32_t b[4], c[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            b[j] = min(nx[j], k + 1u);
            c[j] = i0 + (uint64_t)j < n ? 1u : 0u;              // (an element outside the map reads as 0 and counts nothing)
        }
        if (t + 1 < t1) load4_index<T, true>(index, i0 + kPassTile, n, aligned != 0, nx);   // the next tile, in flight meanwhile
        // the lane's own four: a count moves on to the next pixel while the index stays the same
#pragma unroll
        for (int j = 1; j < 4; ++j)
            if (b[j] == b[j - 1]) { c[j] += c[j - 1]; c[j - 1] = 0u; }
        const bool flat = c[3] == 4u;                           // four pixels of the map, one index
        bool pend = flat;
        unsigned long long todo = __ballot(pend);
        if (todo == kWholeWave) {
            const uint32_t first = __builtin_amdgcn_readfirstlane(b[3]);
            if (__ballot(b[3] == first) == kWholeWave) {        // the whole wave agrees: no LDS traffic, the run grows
                if (first != run_bin) {
                    if (run_cnt != 0u && lane == 0u) atomicAdd(&s_bins[run_bin], run_cnt);
                    run_bin = first;
                    run_cnt = 0u;
                }
                run_cnt += 256u;
                pend = false;
                todo = 0ull;
            }
        }
        // two values that whole lanes agree on: one add of the population count each
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            if (todo == 0ull) break;
            const uint32_t lead = (uint32_t)__ffsll((long long)todo) - 1u;
            const uint32_t first = __builtin_amdgcn_readlane(b[3], __builtin_amdgcn_readfirstlane(lead));
            const bool mine = pend && b[3] == first;
            const unsigned long long m = __ballot(mine);
            if (lane == lead) atomicAdd(&s_bins[first], 4u * (uint32_t)__popcll(m));
            pend = pend && !mine;
            todo &= ~m;
        }
        if (pend) atomicAdd(&s_bins[b[3]], 4u);
        else if (!flat) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (c[j] != 0u) atomicAdd(&s_bins[b[j]], c[j]);
        }
    }
    if (run_cnt != 0u && lane == 0u) atomicAdd(&s_bins[run_bin], run_cnt);
    __syncthreads();
    // adding 0 changes nothing: only the bins that counted something leave the workgroup
    for (uint32_t i = threadIdx.x; i < n_bins; i += kPassBlock) {
        const uint32_t v = s_bins[i];
        if (v != 0u) atomicAdd(usage + i, (unsigned long long)v);
    }
}

// the new index of one pixel, 0 for a bad one (index above k, dropped entry, or a new index that does not fit BITS); a pixel
// outside the row (counted = false) is 0 and not bad
template <uint32_t BITS>
__device__ __forceinline__ uint32_t remap_one(const uint16_t *s_map, uint32_t v, uint32_t k, bool counted, uint32_t &bad)
{
    const uint32_t m = s_map[min(v, k)];
    const bool ok = v <= k && m != (uint32_t)kIndexDropped && (BITS >= 16u || m < (1u << (BITS & 15u)));
    bad += (counted && !ok) ? 1u : 0u;
    return (counted && ok) ? m : 0u;
}

// the PPU pixels behind four output bytes of a row: unit u = (row, four-byte column) in row-major order
template <typename TIn, uint32_t PPU>
__device__ __forceinline__ void remap_load_unit(const TIn *in, uint32_t u, uint32_t units, uint32_t upr, uint32_t width, uint32_t v[PPU])
{
    if (u >= units) return;
    const uint32_t row = u / upr, x0 = (u - row * upr) * PPU;
    const uint64_t base = (uint64_t)row * width, i0 = base + x0;
    const bool al = (reinterpret_cast<uintptr_t>(in + i0) & (4u * sizeof(TIn) - 1u)) == 0;
#pragma unroll
    for (uint32_t g = 0; g < PPU / 4u; ++g) load4_index<TIn, true>(in, i0 + 4u * g, base + width, al, v + 4u * g);   // 0 past the row's end
}

template <typename TIn, uint32_t BITS>
__global__ __launch_bounds__(kPassBlock) void k_index_remap(const TIn *in, void *out_v, uint32_t width, uint32_t rows, uint32_t k,
                                                           const uint16_t *__restrict__ map, int aligned_in, int aligned_out,
                                                           unsigned long long *__restrict__ bad_out)
{
    extern __shared__ uint4 s_dyn[];                            // k + 1 entries of u16
    __shared__ unsigned long long s_part[kPassWaves];
    uint16_t *s_map = reinterpret_cast<uint16_t *>(s_dyn);
    for (uint32_t i = threadIdx.x; i <= k; i += kPassBlock) s_map[i] = map[i];
    __syncthreads();

    uint32_t bad = 0u;
    if constexpr (BITS >= 8u) {
        // one element per pixel: the map as one run of n pixels.  In place (out == in, same width) a lane reads its four pixels
        // of a tile, this one and the next, before it writes them, and no other lane touches them.
        using TOut = typename std::conditional<BITS == 8u, uint8_t, uint16_t>::type;
        TOut *out = static_cast<TOut *>(out_v);
        const uint64_t n = (uint64_t)width * rows;
        uint64_t t0, t1;
        tile_run((n + kPassTile - 1) / kPassTile, t0, t1);
        uint32_t nx[4] = {0u, 0u, 0u, 0u};
        if (t0 < t1) load4_index<TIn, true>(in, t0 * kPassTile + (uint64_t)threadIdx.x * 4u, n, aligned_in != 0, nx);
        for (uint64_t t = t0; t < t1; ++t) {
            const uint64_t i0 = t * kPassTile + (uint64_t)threadIdx.x * 4u;
            const uint32_t v[4] = {nx[0], nx[1], nx[2], nx[3]};
            if (t + 1 < t1) load4_index<TIn, true>(in, i0 + kPassTile, n, aligned_in != 0, nx);   // the next tile, in flight meanwhile
            uint32_t o[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = remap_one<BITS>(s_map, v[j], k, i0 + (uint64_t)j < n, bad);
            store4_index<TOut, true>(out, i0, n, aligned_out != 0, o);
        }
    } else {
        // packed rows: every row starts on a byte, the leftmost pixel in the high bits, the padding bits of its last byte zero
        constexpr uint32_t PPB = 8u / BITS, PPU = 4u * PPB;     // pixels per output byte, per unit of four bytes
        uint8_t *out = static_cast<uint8_t *>(out_v);
        const uint32_t stride = (uint32_t)(((uint64_t)width * BITS + 7u) / 8u), upr = (stride + 3u) / 4u;
        const uint32_t units = rows * upr;                      // <= width * rows < 2^32
        uint64_t t0, t1;
        tile_run(((uint64_t)units + kPassBlock - 1) / kPassBlock, t0, t1);
        uint32_t nx[PPU];
#pragma unroll
        for (uint32_t j = 0; j < PPU; ++j) nx[j] = 0u;
        if (t0 < t1) remap_load_unit<TIn, PPU>(in, (uint32_t)(t0 * kPassBlock) + threadIdx.x, units, upr, width, nx);
        for (uint64_t t = t0; t < t1; ++t) {
            const uint64_t u64 = t * kPassBlock + threadIdx.x;  // (the last tile may end above `units`)
            const uint32_t u = (uint32_t)u64;
            uint32_t v[PPU];
#pragma unroll
            for (uint32_t j = 0; j < PPU; ++j) v[j] = nx[j];
            if (t + 1 < t1 && u64 + kPassBlock < units) remap_load_unit<TIn, PPU>(in, u + kPassBlock, units, upr, width, nx);   // the next tile
            if (u64 >= units) continue;
            const uint32_t row = u / upr, b0 = (u - row * upr) * 4u, x0 = b0 * PPB;
            uint32_t word = 0u;
#pragma unroll
            for (uint32_t j = 0; j < PPU; ++j) {
                const uint32_t m = remap_one<BITS>(s_map, v[j], k, (uint64_t)x0 + j < width, bad);
                word |= m << (8u * (j / PPB) + (8u - BITS * (j % PPB + 1u)));
            }
            uint8_t *o = out + (uint64_t)row * stride + b0;
            if (b0 + 4u <= stride && (reinterpret_cast<uintptr_t>(o) & 3u) == 0) {
                __builtin_nontemporal_store(word, reinterpret_cast<uint32_t *>(o));
            } else {
#pragma unroll
                for (uint32_t q = 0; q < 4u; ++q)
                    if (b0 + q < stride) o[q] = (uint8_t)(word >> (8u * q));
            }
        }
    }
    const unsigned long long total = block_sum((unsigned long long)bad, s_part);
    if (threadIdx.x == 0 && total != 0ull) atomicAdd(bad_out, total);
}

template <typename T>
hipError_t usage_typed(const void *index, uint64_t n, uint32_t k, unsigned long long *usage, hipStream_t st)
{
    const uint32_t grid = pass_grid((n + kPassTile - 1) / kPassTile);
    const int aligned = (reinterpret_cast<uintptr_t>(index) & (4u * sizeof(T) - 1u)) == 0 ? 1 : 0;
    const size_t lds = (((size_t)k + 2u) * sizeof(uint32_t) + 15u) & ~(size_t)15u;
    hipLaunchKernelGGL((k_index_usage<T>), dim3(grid), dim3(kPassBlock), lds, st, static_cast<const T *>(index), n, k, aligned, usage);
    return hipGetLastError();
}

template <typename TIn, uint32_t BITS>
hipError_t remap_typed(const void *in, void *out, uint32_t width, uint32_t rows, uint32_t k, const uint16_t *map, unsigned long long *bad,
                       hipStream_t st)
{
    const uint64_t n = (uint64_t)width * rows;
    uint64_t tiles;
    if (BITS >= 8u) tiles = (n + kPassTile - 1) / kPassTile;
    else {
        const uint64_t stride = ((uint64_t)width * BITS + 7u) / 8u, units = (uint64_t)rows * ((stride + 3u) / 4u);
        tiles = (units + kPassBlock - 1) / kPassBlock;
    }
    // the vector accesses of the 8- / 16-bit forms: four elements of the input, four of the output (the packed forms look at
    // each unit's own addresses)
    const int aligned_in = (reinterpret_cast<uintptr_t>(in) & (4u * sizeof(TIn) - 1u)) == 0 ? 1 : 0;
    const int aligned_out = (reinterpret_cast<uintptr_t>(out) & (BITS == 16u ? 7u : 3u)) == 0 ? 1 : 0;
    const size_t lds = (((size_t)k + 1u) * sizeof(uint16_t) + 15u) & ~(size_t)15u;
    hipLaunchKernelGGL((k_index_remap<TIn, BITS>), dim3(pass_grid(tiles)), dim3(kPassBlock), lds, st, static_cast<const TIn *>(in), out, width,
                       rows, k, map, aligned_in, aligned_out, bad);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_index_usage(const void *index, bool wide, uint64_t n, uint32_t k, unsigned long long *usage, hipStream_t st)
{
    hipError_t e = hipErrorInvalidValue;
    with_index_type(wide, [&](auto t) { e = usage_typed<typename decltype(t)::type>(index, n, k, usage, st); });
    return e;
}

hipError_t launch_index_remap(const void *in, bool wide, uint32_t width, uint32_t rows, uint32_t k, const uint16_t *map, uint32_t out_bits,
                              void *out, unsigned long long *bad, hipStream_t st)
{
    hipError_t e = hipErrorInvalidValue;                              // (stays for out_bits outside 1 / 2 / 4 / 8 / 16)
    with_index_type(wide, [&](auto t) { with_value<1, 2, 4, 8, 16>((int)out_bits, [&](auto B) {
        e = remap_typed<typename decltype(t)::type, B()>(in, out, width, rows, k, map, bad, st);
    }); });
    return e;
}

namespace {

bool bits_ok(uint32_t bits) { return bits == 1u || bits == 2u || bits == 4u || bits == 8u || bits == 16u; }

// what both passes ask of a map: an index format, a colour count it can hold, an aligned pointer
int check_index_map(const char *name, const void *map, int format, uint32_t k)
{
    if (format != KMG_FORMAT_INDEX8 && format != KMG_FORMAT_INDEX16)
        return fail(KMG_ERR_INVALID_ARGUMENT, "%s: format %d is not an index format", name, format);
    if (k == 0 || k > KMG_MAX_K) return fail(KMG_ERR_INVALID_ARGUMENT, "%s: k = %u is outside 1 .. %u", name, k, KMG_MAX_K);
    if (format == KMG_FORMAT_INDEX8 && k > 256u) return fail(KMG_ERR_INVALID_ARGUMENT, "%s: INDEX8 holds 256 indices; k = %u needs INDEX16", name, k);
    if (!map) return fail(KMG_ERR_INVALID_ARGUMENT, "%s: the index map is NULL", name);
    if (format == KMG_FORMAT_INDEX16 && (reinterpret_cast<uintptr_t>(map) & 1u))
        return fail(KMG_ERR_INVALID_ARGUMENT, "%s: an INDEX16 map is not 2-byte aligned", name);
    return KMG_OK;
}

int check_usage_args(const kmg_processor *p, const void *index, uint64_t n, int format, uint32_t k, const uint64_t *usage)
{
    KMG_TRY(check_index_map("index_usage", index, format, k));
    if (!p || !usage) return fail(KMG_ERR_INVALID_ARGUMENT, "index_usage: the processor or the record is NULL");
    if (n == 0) return fail(KMG_ERR_INVALID_ARGUMENT, "index_usage: no pixels");
    if (n > 0xFFFFFFFFull) return fail(KMG_ERR_UNSUPPORTED, "index_usage: more than 2^32-1 pixels");
    if (reinterpret_cast<uintptr_t>(usage) & 7u) return fail(KMG_ERR_INVALID_ARGUMENT, "index_usage: the record is not 8-byte aligned");
    return KMG_OK;
}

int check_remap_args(const kmg_processor *p, const void *in, int format, uint32_t width, uint32_t rows, uint32_t k, const uint16_t *remap,
                     uint32_t out_bits, const void *out)
{
    KMG_TRY(check_index_map("index_remap", in, format, k));
    if (!bits_ok(out_bits)) return fail(KMG_ERR_INVALID_ARGUMENT, "index_remap: out_bits = %u is not 1, 2, 4, 8 or 16", out_bits);
    if (!p || !remap || !out) return fail(KMG_ERR_INVALID_ARGUMENT, "index_remap: the processor, the table or the output is NULL");
    if (width == 0 || rows == 0) return fail(KMG_ERR_INVALID_ARGUMENT, "index_remap: zero width or rows");
    if ((uint64_t)width * rows > 0xFFFFFFFFull) return fail(KMG_ERR_UNSUPPORTED, "index_remap: more than 2^32-1 pixels");
    if (out_bits == 16u && (reinterpret_cast<uintptr_t>(out) & 1u)) return fail(KMG_ERR_INVALID_ARGUMENT, "index_remap: a 16-bit output is not 2-byte aligned");
    return KMG_OK;
}

int dev_usage(kmg_processor *p, const void *d_index, uint64_t n, int format, uint32_t k, uint64_t *d_usage, hipStream_t st)
{
    KMG_TRY(check_usage_args(p, d_index, n, format, k, d_usage));
    HIP_TRY(hipSetDevice(p->device));
    unsigned long long *usage = reinterpret_cast<unsigned long long *>(d_usage);
    HIP_TRY(launch_index_usage(d_index, format == KMG_FORMAT_INDEX16, n, k, usage, st));
    return KMG_OK;
}

// Enqueues on st: the table's upload from a heap copy of the caller's entries (released by the stream once the copy has run)
// and the launch; the device copy of the table goes back to the pool in stream order.
int dev_remap(kmg_processor *p, const void *d_in, int format, uint32_t width, uint32_t rows, uint32_t k, const uint16_t *remap,
              uint32_t out_bits, void *d_out, uint64_t *d_bad, hipStream_t st)
{
    KMG_TRY(check_remap_args(p, d_in, format, width, rows, k, remap, out_bits, d_out));
    if (!d_bad || (reinterpret_cast<uintptr_t>(d_bad) & 7u)) return fail(KMG_ERR_INVALID_ARGUMENT, "index_remap: the bad-pixel count is NULL or not 8-byte aligned");
    HIP_TRY(hipSetDevice(p->device));
    const size_t bytes = ((size_t)k + 1u) * sizeof(uint16_t);
    StreamBuf tab;
    HIP_TRY(tab.alloc(p, bytes, st));
    HIP_TRY(upload_host_copy(tab.ptr, remap, bytes, st));
    unsigned long long *bad = reinterpret_cast<unsigned long long *>(d_bad);
    const uint16_t *map = static_cast<const uint16_t *>(tab.ptr);
    HIP_TRY(launch_index_remap(d_in, format == KMG_FORMAT_INDEX16, width, rows, k, map, out_bits, d_out, bad, st));
    return KMG_OK;
}

size_t map_bytes(int format, uint64_t n) { return (size_t)n * (format == KMG_FORMAT_INDEX16 ? 2u : 1u); }

size_t packed_bytes(uint32_t width, uint32_t rows, uint32_t bits)
{
    return bits >= 8u ? (size_t)width * rows * (bits / 8u) : (size_t)(((uint64_t)width * bits + 7u) / 8u) * rows;
}

int plan_of(const uint64_t *usage, const uint8_t *palette_rgba, uint32_t k, uint32_t flags, uint16_t *remap, uint8_t *out_palette_rgba,
            kmg_index_plan_info *info)
{
    static_assert(sizeof(kmg_index_plan_info) == sizeof(IndexPlanInfo) && sizeof(kmg_index_plan_info) == 16, "kmg_index_plan_info is 16 bytes");
    static_assert(KMG_MAX_K == kIndexPlanMaxK, "kmg_index_plan.h knows KMG_MAX_K");
    static_assert(KMG_INDEX_ORDER_KEEP == kIndexOrderKeep && KMG_INDEX_ORDER_USAGE == kIndexOrderUsage && KMG_INDEX_ORDER_LUMA == kIndexOrderLuma &&
                      KMG_INDEX_KEEP_UNUSED == kIndexKeepUnused && KMG_INDEX_KEEP_TRANSPARENT == kIndexKeepTransparent &&
                      KMG_INDEX_TRANSPARENT_FIRST == kIndexTransparentFirst,
                  "kmg_index_plan.h knows the flags");
    IndexPlanInfo pi;
    const char *why = index_plan(usage, palette_rgba, k, flags, remap, out_palette_rgba, info ? &pi : nullptr);
    if (why) return fail(KMG_ERR_INVALID_ARGUMENT, "index_plan: %s", why);
    info->n_colors = pi.n_colors;
    info->n_slots = pi.n_slots;
    info->transparent = pi.transparent;
    info->bits = pi.bits;
    return KMG_OK;
}

}  // namespace

}  // namespace kmg

extern "C" int kmg_dev_index_usage(kmg_processor *p, const void *d_index, uint64_t n_pixels, int format, uint32_t k, uint64_t *d_usage,
                                   void *stream)
try {
    return dev_usage(p, d_index, n_pixels, format, k, d_usage, S(stream));
}
KMG_ABI_CATCH

extern "C" int kmg_index_plan(const uint64_t *usage, const uint8_t *palette_rgba, uint32_t k, uint32_t flags, uint16_t *remap,
                              uint8_t *out_palette_rgba, kmg_index_plan_info *info)
try {
    return plan_of(usage, palette_rgba, k, flags, remap, out_palette_rgba, info);
}
KMG_ABI_CATCH

extern "C" int kmg_dev_index_remap(kmg_processor *p, const void *d_in, int in_format, uint32_t width, uint32_t rows, uint32_t k,
                                   const uint16_t *remap, uint32_t out_bits, void *d_out, uint64_t *d_bad, void *stream)
try {
    return dev_remap(p, d_in, in_format, width, rows, k, remap, out_bits, d_out, d_bad, S(stream));
}
KMG_ABI_CATCH

extern "C" int kmg_index_usage(kmg_processor *p, const void *index, int format, uint64_t n_pixels, uint32_t k, uint64_t *usage)
try {
    // (the refusals that need no device come first)
    KMG_TRY(check_usage_args(p, index, n_pixels, format, k, usage));
    HIP_TRY(hipSetDevice(p->device));
    StreamGuard sg;
    HIP_TRY(sg.acquire(p));
    const size_t bytes = map_bytes(format, n_pixels), rec_bytes = ((size_t)k + 2u) * sizeof(uint64_t);
    StreamBuf map, rec;
    HIP_TRY(map.alloc(p, bytes, sg.st));
    HIP_TRY(copy_host_image(p, map.ptr, index, bytes, hipMemcpyHostToDevice, sg.st));
    HIP_TRY(rec.alloc(p, rec_bytes, sg.st));
    HIP_TRY(hipMemsetAsync(rec.ptr, 0, rec_bytes, sg.st));
    KMG_TRY_DRAIN(sg.st, dev_usage(p, map.ptr, n_pixels, format, k, static_cast<uint64_t *>(rec.ptr), sg.st));
    std::vector<uint64_t> got((size_t)k + 2u);
    HIP_TRY(hipMemcpyAsync(got.data(), rec.ptr, rec_bytes, hipMemcpyDeviceToHost, sg.st));
    HIP_TRY(hipStreamSynchronize(sg.st));
    for (size_t i = 0; i < got.size(); ++i) usage[i] += got[i];
    return KMG_OK;
}
KMG_ABI_CATCH

extern "C" int kmg_index_remap(kmg_processor *p, const void *in, int in_format, uint32_t width, uint32_t height, uint32_t k,
                               const uint16_t *remap, uint32_t out_bits, void *out, uint64_t *bad)
try {
    // (the refusals that need no device come first)
    KMG_TRY(check_remap_args(p, in, in_format, width, height, k, remap, out_bits, out));
    HIP_TRY(hipSetDevice(p->device));
    StreamGuard sg;
    HIP_TRY(sg.acquire(p));
    const size_t in_bytes = map_bytes(in_format, (uint64_t)width * height), out_bytes = packed_bytes(width, height, out_bits);
    StreamBuf src, dst, cnt;
    HIP_TRY(src.alloc(p, in_bytes, sg.st));
    HIP_TRY(copy_host_image(p, src.ptr, in, in_bytes, hipMemcpyHostToDevice, sg.st));
    HIP_TRY(dst.alloc(p, out_bytes, sg.st));
    HIP_TRY(cnt.alloc(p, sizeof(uint64_t), sg.st));
    HIP_TRY(hipMemsetAsync(cnt.ptr, 0, sizeof(uint64_t), sg.st));
    KMG_TRY_DRAIN(sg.st, dev_remap(p, src.ptr, in_format, width, height, k, remap, out_bits, dst.ptr, static_cast<uint64_t *>(cnt.ptr), sg.st));
    uint64_t n_bad = 0;
    HIP_TRY(copy_host_image(p, out, dst.ptr, out_bytes, hipMemcpyDeviceToHost, sg.st));
    HIP_TRY(hipMemcpyAsync(&n_bad, cnt.ptr, sizeof(uint64_t), hipMemcpyDeviceToHost, sg.st));
    HIP_TRY(hipStreamSynchronize(sg.st));
    if (bad) *bad = n_bad;
    return KMG_OK;
}
KMG_ABI_CATCH

extern "C" int kmg_index_optimize(kmg_processor *p, const void *index, int format, uint32_t width, uint32_t height,
                                  const uint8_t *palette_rgba, uint32_t k, uint32_t flags, uint32_t out_bits, uint8_t *out_palette_rgba,
                                  kmg_index_plan_info *info, void *out_map)
try {
    // (the refusals that need no device come first)
    KMG_TRY(check_index_map("index_optimize", index, format, k));
    if (!p || !palette_rgba || !out_palette_rgba || !info || !out_map) return fail(KMG_ERR_INVALID_ARGUMENT, "index_optimize: a pointer is NULL");
    if (width == 0 || height == 0) return fail(KMG_ERR_INVALID_ARGUMENT, "index_optimize: zero width or height");
    const uint64_t n = (uint64_t)width * height;
    if (n > 0xFFFFFFFFull) return fail(KMG_ERR_UNSUPPORTED, "index_optimize: more than 2^32-1 pixels");
    const uint32_t in_bits = format == KMG_FORMAT_INDEX16 ? 16u : 8u;
    if (out_bits != 0u && !bits_ok(out_bits)) return fail(KMG_ERR_INVALID_ARGUMENT, "index_optimize: out_bits = %u is not 0, 1, 2, 4, 8 or 16", out_bits);
    if (out_bits > in_bits) return fail(KMG_ERR_INVALID_ARGUMENT, "index_optimize: out_bits = %u is wider than the input map's %u", out_bits, in_bits);
    if ((flags & ~kIndexFlagsAll) || (flags & kIndexOrderMask) == 3u) return fail(KMG_ERR_INVALID_ARGUMENT, "index_optimize: unknown flag bits or order");
    HIP_TRY(hipSetDevice(p->device));
    StreamGuard sg;
    HIP_TRY(sg.acquire(p));
    const size_t in_bytes = map_bytes(format, n), rec_bytes = ((size_t)k + 2u) * sizeof(uint64_t);
    StreamBuf src, dst, rec;                                           // rec: the k + 2 counts, then the bad-pixel count
    HIP_TRY(src.alloc(p, in_bytes, sg.st));
    HIP_TRY(copy_host_image(p, src.ptr, index, in_bytes, hipMemcpyHostToDevice, sg.st));
    HIP_TRY(rec.alloc(p, rec_bytes + sizeof(uint64_t), sg.st));
    HIP_TRY(hipMemsetAsync(rec.ptr, 0, rec_bytes + sizeof(uint64_t), sg.st));
    KMG_TRY_DRAIN(sg.st, dev_usage(p, src.ptr, n, format, k, static_cast<uint64_t *>(rec.ptr), sg.st));
    std::vector<uint64_t> usage((size_t)k + 2u);
    HIP_TRY(hipMemcpyAsync(usage.data(), rec.ptr, rec_bytes, hipMemcpyDeviceToHost, sg.st));
    HIP_TRY(hipStreamSynchronize(sg.st));                              // (the plan is host arithmetic on the counts)
    std::vector<uint16_t> remap((size_t)k + 1u);
    std::vector<uint8_t> pal(((size_t)k + 1u) * 4u);
    kmg_index_plan_info pi;
    KMG_TRY(plan_of(usage.data(), palette_rgba, k, flags, remap.data(), pal.data(), &pi));
    const uint32_t bits = out_bits ? out_bits : pi.bits;
    if (bits < pi.bits) return fail(KMG_ERR_INVALID_ARGUMENT, "index_optimize: %u slots need %u bits, out_bits = %u", pi.n_slots, pi.bits, out_bits);
    if (bits > in_bits) return fail(KMG_ERR_INVALID_ARGUMENT, "index_optimize: %u slots need %u bits, more than the input map's %u", pi.n_slots, bits, in_bits);
    const size_t out_bytes = packed_bytes(width, height, bits);
    HIP_TRY(dst.alloc(p, out_bytes, sg.st));
    uint64_t *d_bad = static_cast<uint64_t *>(rec.ptr) + (k + 2u);
    KMG_TRY_DRAIN(sg.st, dev_remap(p, src.ptr, format, width, height, k, remap.data(), bits, dst.ptr, d_bad, sg.st));
    uint64_t n_bad = 0;
    HIP_TRY(copy_host_image(p, out_map, dst.ptr, out_bytes, hipMemcpyDeviceToHost, sg.st));
    HIP_TRY(hipMemcpyAsync(&n_bad, d_bad, sizeof(uint64_t), hipMemcpyDeviceToHost, sg.st));
    HIP_TRY(hipStreamSynchronize(sg.st));
    if (n_bad != 0) return fail(KMG_ERR_HIP, "index_optimize: %llu pixels fell outside the plan made from their own counts", (unsigned long long)n_bad);
    memcpy(out_palette_rgba, pal.data(), (size_t)pi.n_slots * 4u);
    *info = pi;
    return KMG_OK;
}
KMG_ABI_CATCH
