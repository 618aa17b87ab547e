// kmg_seed.hip -- the seed pass of a seeded initialisation over the colours of a bound image (kmg_lloyd_init_centroids_seeded;
// its counterpart over pixels, k_init_seed, is in kmg_kernels.hip).  It writes what the passes of kmg_table.hip (k_init_fused) read
// next -- the per-colour distance map, the cell records, the workgroups' slots -- so the layouts below restate that file's, and
// tests/test_gpu_fixed.py compares the centroids the two files produce together with the model, bit for bit.
// Compile with -ffp-contract=off.

#include "kmg_internal.h"
#include "kmg_kernels.h"
#include "kmg_table_dev.h"

namespace kmg {

// ---- the hand-over of kmg_table.hip's initialisation passes, restated (same names, same layout) ------------------------------
constexpr uint32_t kInitGrid = 256, kInitBlock = 1024;
static_assert(kInitGrid * (kInitBlock / 64) * 8 == kCells, "one test slot per cell");
constexpr uint32_t kNoCell = 0xFFFFFFFFu;

struct alignas(16) InitSlot { unsigned long long key; uint32_t pad[2]; float4 lab; };
struct alignas(16) InitRecord {
    unsigned long long key;        // largest key of the cell's colours
    uint32_t cell;                 // kNoCell: past the end of the work list
    uint32_t pad;
    float4 lab;                    // Lab of the colour that holds it
    CellBounds cb;
};
static_assert(sizeof(InitSlot) == 32 && sizeof(InitRecord) == 32 + sizeof(CellBounds), "init record layout");

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v)
{
    const uint32_t hi = (uint32_t)(v >> 32), lo = (uint32_t)v;
    const uint32_t mhi = wave_max_u32_dpp(hi);
    const uint32_t mlo = wave_max_u32_dpp(hi == mhi ? lo : 0u);
    return ((unsigned long long)mhi << 32) | mlo;
}

__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) { return wave_max_u32_dpp(v); }

// test slot q (0..127) of workgroup g (0..255) -> index into the work list
__device__ __forceinline__ uint32_t slot_work_index(uint32_t g, uint32_t q)
{
    const uint32_t b = (g & 7u) | ((q & 3u) << 3), gg = ((g >> 3) & 7u) | (((q >> 2) & 3u) << 3), r = (g >> 6) | ((q >> 4) << 2);
    return (r << 10) | (gg << 5) | b;
}

// Seeded initialisation over the colours (kmg_lloyd_init_centroids_seeded): centroids 0 .. f - 1 are given, so launches 1 .. f have
// nothing to pick and collapse into ONE sweep over every occupied cell -- no cell can be skipped, no record holds a distance yet --
// that leaves dist = fminf over 1e6 and cie94(colour, cent[0 .. f - 1]) in that order, every cell's record and the workgroups'
// slots exactly as launch f leaves them: launch f + 1 of k_init_fused<true> picks centroid f and goes on unchanged.  Wave wv visits
// the eight cells it would test (slot_work_index), 64 lanes x 8 colours each; the f seeds sit in LDS (16 bytes each, dynamic).
__global__ __launch_bounds__(kInitBlock) void k_init_seed_cells(const uint32_t *__restrict__ tie, const uint8_t *__restrict__ occ_bits,
                                                                const float4 *__restrict__ lab_table, const Centroid *__restrict__ cent,
                                                                uint32_t f, float *__restrict__ dist, InitRecord *__restrict__ records,
                                                                InitSlot *__restrict__ slots)
{
    extern __shared__ float4 s_seed_cells[];
    __shared__ unsigned long long s_key[kInitBlock / 64];
    __shared__ float4 s_lab[kInitBlock / 64];
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (uint32_t q = threadIdx.x; q < f; q += kInitBlock) { const Centroid c = cent[q]; s_seed_cells[q] = make_float4(c.L, c.a, c.b, c.C); }
    __syncthreads();

    unsigned long long run_key = 0ull;                             // the largest record this lane has met
    float4 run_lab = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    for (uint32_t e = 0; e < 8u; ++e) {
        const uint32_t wi = slot_work_index(blockIdx.x, wv * 8u + e);
        const uint32_t cell = records[wi].cell;                    // (the same for the whole wave)
        if (cell == kNoCell) continue;
        const uint32_t base = cell * kCellColours + lane * 8u;
        const uint32_t occ = occ_bits[(uint64_t)cell * 64u + lane];
        float4 v[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = lab_table[base + q];
        const uint4 t0 = *reinterpret_cast<const uint4 *>(tie + base), t1 = *reinterpret_cast<const uint4 *>(tie + base + 4);
        float m[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) m[q] = 1000000.0f;             // kmeans++_calc_diff.wgsl:26-30
        for (uint32_t s = 0; s < f; ++s) {
            const float4 c = s_seed_cells[s];
#pragma unroll
            for (int q = 0; q < 8; ++q)
                if ((occ >> q) & 1u) m[q] = fminf(m[q], cie94(v[q].x, v[q].y, v[q].z, c.x, c.y, c.z));
        }
        uint32_t md = 0u;                                          // largest distance (bits) among this lane's colours
#pragma unroll
        for (int q = 0; q < 8; ++q)
            if ((occ >> q) & 1u) md = max(md, float_to_bits(m[q]));
        *reinterpret_cast<float4 *>(dist + base) = make_float4(m[0], m[1], m[2], m[3]);
        *reinterpret_cast<float4 *>(dist + base + 4) = make_float4(m[4], m[5], m[6], m[7]);
        // the cell's key = (largest distance, largest low half among the colours that hold it), as in k_init_fused (kmg_table.hip)
        const uint32_t wmd = wave_max_u32(md);
        uint32_t low1 = 0u;
        float4 best_lab = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (occ && md == wmd) {
            const uint32_t t[8] = {t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w};
#pragma unroll
            for (int q = 0; q < 8; ++q)
                if (((occ >> q) & 1u) && float_to_bits(m[q]) == wmd && t[q] > low1) { low1 = t[q]; best_lab = v[q]; }
        }
        const uint32_t wlow1 = wave_max_u32(low1);
        if (low1 == wlow1 && low1 != 0u) {
            const unsigned long long key = ((unsigned long long)wmd << 32) | (unsigned long long)(wlow1 - 1u);
            InitRecord *r = records + wi;
            r->key = key;
            r->lab = best_lab;
            if (key >= run_key) { run_key = key; run_lab = best_lab; }
        }
    }
    // the largest record of the workgroup, into the slot set of launch f
    const unsigned long long wbest = wave_max_u64(run_key);
    if (lane == (uint32_t)__builtin_ctzll(__ballot(run_key == wbest))) { s_key[wv] = wbest; s_lab[wv] = run_lab; }
    __syncthreads();
    if (wv == 0u) {
        const unsigned long long k16 = lane < kInitBlock / 64u ? s_key[lane] : 0ull;
        const float4 el = s_lab[lane < kInitBlock / 64u ? lane : 0u];
        const unsigned long long best = wave_max_u64(k16);
        if (lane == (uint32_t)__builtin_ctzll(__ballot(k16 == best))) {
            InitSlot o; o.key = best; o.pad[0] = 0u; o.pad[1] = 0u; o.lab = el;
            slots[(f & 1u) * kInitGrid + blockIdx.x] = o;
        }
    }
}

hipError_t launch_init_seed_cells(const uint32_t *tie, const uint8_t *occ_bits, const float4 *lab_table, const Centroid *cent,
                                  uint32_t n_seeds, float *dist, void *init_scratch, hipStream_t st)
{
    InitRecord *records = (InitRecord *)init_scratch;
    InitSlot *slots = (InitSlot *)(records + kCells);
    hipLaunchKernelGGL(k_init_seed_cells, dim3(kInitGrid), dim3(kInitBlock), sizeof(float4) * n_seeds, st, tie, occ_bits, lab_table, cent,
                       n_seeds, dist, records, slots);
    return hipGetLastError();
}

}  // namespace kmg
