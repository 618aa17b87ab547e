// kmg_batch.hip -- many small images per launch on one device: the segmented versions of the small-image route (single-pick
// initialisation k_init_first / k_init_pass<PICK> / k_init_pick_slots and the one-launch Lloyd step k_assign<1, true, CHUNKED, LOOP>
// of kmg_kernels.hip) and kmg_dev_palette_batch / kmg_dev_palette_batch_counts on top of them (include/kmeans_hip.h; DESIGN.md 4.16,
// and 4.18 for the colour count per image).
//
// A batch is a table of BatchImage records in device memory, one per image.  The grid of a pass is the sum of the images' tiles
// (256 pixels each, at most 2048 per image: the batch takes working images below 2^19 pixels); a workgroup finds its image by a
// binary search over the records' first-workgroup column and then runs the arithmetic of the per-image kernel, operation for
// operation, on that image's own buffers.  Images are independent problems and their sums are integers, so every image gets the
// bits the per-image calls give it.
//
// Synchronisation: the launch boundary, nothing else.  No kernel here waits for another workgroup, and every loop has a bound
// known at launch.  When an image's loop stops is decided by the HOST, from the convergence counts it reads back where
// kmg_lloyd_run reads them (one copy for the whole batch); it then sets the image's word in `stop`, which the kernels only
// read: the workgroups of a stopped image return at once and leave its centroids, sums and count as they are.
//
// Compile with -ffp-contract=off: arithmetic must match kmg_math.h operation for operation.

#include "kmg_state.h"

#include "kmg_batch_layout.h"    // kBatchMaxGrid
#include "kmg_device.h"
#include "kmg_lloyd_dev.h"       // argmin_scan, init_key_index, init_max_slot

namespace kmg {

// One image of a batch.  All pointers are device memory carved from one block of the processor (batch_run).
struct alignas(16) BatchImage {
    const uint32_t *rgba;          // n pixels
    float *dist;                   // n running distances of the initialisation
    unsigned long long *slots;     // 2 x tiles keys: the workgroups' keys of the initialisation's passes, by pass parity
    Centroid *cent;                // 2 x k: the two centroid buffers; launch l of the loop reads buffer (l - 1) & 1, writes l & 1
    int64_t *acc;                  // 3 x k x 4: the three sum buffers; launch l adds to l % 3, clears (l + 1) % 3, reads (l + 2) % 3
    uint32_t *state;               // kStateWords: [0] the convergence count, [kFixedWord] = 0 (no frozen centroid)
    uint32_t n;                    // pixels, < 2^19
    uint32_t first_wg;             // index of the image's first workgroup in the grid
    uint32_t first_pixel;          // plus_plus_init.wgsl:161-168 `initial` of this image's width and height
    uint32_t k;                    // the image's own colour count: the size of its cent / acc tables, what its loop converges to
};
static_assert(sizeof(BatchImage) == 64, "BatchImage layout");

// (the image a workgroup belongs to: batch_image_of, kmg_device.h)

__device__ __forceinline__ Centroid centroid_of_pixel(const float *__restrict__ lut, uint32_t px)
{
    // plus_plus_init.wgsl:161-168 `initial` / :172-181 `pick`
    float L, a, b;
    linear100_to_lab(lut[px & 255u], lut[(px >> 8) & 255u], lut[(px >> 16) & 255u], L, a, b);
    Centroid o; o.L = L; o.a = a; o.b = b; o.C = chroma(a, b);
    return o;
}

// ------------------------------------------------------------------------------------------
// Batched initialisation: pass j (1 <= j < the largest k of the piece) of EVERY image with j < its own k in one launch --
// k_init_pass<true> per image with one tile per workgroup.  The workgroups of an image whose k is reached return at once: its slot
// set of parity (k - 1) & 1 -- the one its last pass wrote -- then stays as it is until k_batch_init_pick reads it.  Every workgroup first derives centroid j - 1 of its image itself: the image's first pixel (j = 1: k_init_first) or the
// pixel named by the largest slot of pass j - 1; the image's first workgroup also writes it to the table.  Then the pass: the
// running distances against that centroid, the workgroup's largest key into the slot set of parity j & 1.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_batch_init_pass(const BatchImage *__restrict__ img, uint32_t n_images,
                                                            const float *__restrict__ lut, uint32_t j)
{
    __shared__ float s_lut[256];
    __shared__ unsigned long long s_key[kBlock / 64];
    __shared__ Centroid s_c;
    const BatchImage im = img[batch_image_of(img, n_images, blockIdx.x)];
    if (j >= im.k) return;                                           // (the whole workgroup: the image is uniform)
    const uint32_t wg = blockIdx.x - im.first_wg, tiles = (im.n + kBlock - 1u) / kBlock;
    s_lut[threadIdx.x] = lut[threadIdx.x];
    // (this thread's pixel and its running distance do not depend on the new centroid: requested before the pick)
    const uint32_t i = wg * kBlock + threadIdx.x;
    uint32_t px = 0u;
    float before = 1000000.0f;                                      // kmeans++_calc_diff.wgsl:26-30
    if (i < im.n) {
        px = im.rgba[i];
        if (j != 1u) before = im.dist[i];
    }
    unsigned long long kk = 0ull;
    if (j >= 2u) kk = init_max_slot(im.slots + ((j - 1u) & 1u) * tiles, tiles, s_key);   // (a barrier inside)
    if (threadIdx.x == 0) {
        const Centroid o = centroid_of_pixel(lut, im.rgba[j >= 2u ? init_key_index(kk) : im.first_pixel]);
        s_c = o;
        if (wg == 0u) im.cent[j - 1u] = o;
    }
    __syncthreads();
    const Centroid c = s_c;
    unsigned long long best = 0ull;
    if (i < im.n) {
        float L, a, b;
        px_to_lab(s_lut, px, L, a, b);
        const float d = cie94(L, a, b, c.L, c.a, c.b);
        const float m = fminf(before, d);
        im.dist[i] = m;
        best = ((unsigned long long)float_to_bits(m) << 32) | (unsigned long long)(((i >> 4) << 4) | (15u - (i & 15u)));
    }
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_down(best, off, 64);
        best = o > best ? o : best;
    }
    if ((threadIdx.x & 63) == 0) s_key[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kBlock / 64; ++w) best = s_key[w] > best ? s_key[w] : best;
        im.slots[(j & 1u) * tiles + wg] = best;
    }
}

// The last centroid of every image, one workgroup per image: centroid j = k - 1 of the image's own k from the slots of its pass j
// (k_init_pick_slots), or -- j = 0, an image with k = 1 -- the image's first pixel (k_init_first).
__global__ __launch_bounds__(kBlock) void k_batch_init_pick(const BatchImage *__restrict__ img, const float *__restrict__ lut)
{
    __shared__ unsigned long long s_key[kBlock / 64];
    const BatchImage im = img[blockIdx.x];
    const uint32_t j = im.k - 1u;
    const uint32_t tiles = (im.n + kBlock - 1u) / kBlock;
    unsigned long long kk = 0ull;
    if (j >= 1u) kk = init_max_slot(im.slots + (j & 1u) * tiles, tiles, s_key);
    if (threadIdx.x == 0) im.cent[j] = centroid_of_pixel(lut, im.rgba[j >= 1u ? init_key_index(kk) : im.first_pixel]);
}

// ------------------------------------------------------------------------------------------
// Batched Lloyd step: launch `launch` of EVERY image that is still running -- k_assign<1, true, CHUNKED, LOOP> per image, one tile
// per workgroup.  launch >= 1: every workgroup does the update on its LDS copy of its image's centroids, from the sums the
// previous launch left (the image's first workgroup writes the centroids to the other buffer and the convergence count to the
// image's state); then the assign, and the workgroup's bins are added to the image's sum buffer of this launch.  The buffers
// rotate with the launch number, the same for every image; stop[i] != 0 (host-written between launches): image i has stopped.
// LDS: [centroids kpad x 16 B][bins k x 32 B][sRGB table 1 KiB], laid out by the image's own k; the launch is sized for the
// largest k of the piece.
// SCAN: the form of argmin_scan (kmg_lloyd_dev.h) -- kScanPlain / kScanChunked: the one form for every image of the piece (all k
// below 32 / all from 32 on); kScanByImage: a piece with counts on both sides, each workgroup takes the form of its image's k by
// a branch that is uniform over the workgroup.  Either way an image is scanned by the form k_assign takes at its k.
// ------------------------------------------------------------------------------------------
enum { kScanPlain = 0, kScanChunked = 1, kScanByImage = 2 };

template <int SCAN>
__global__ __launch_bounds__(kBlock) void k_batch_assign(const BatchImage *__restrict__ img, uint32_t n_images,
                                                         const uint32_t *__restrict__ stop,
                                                         const float *__restrict__ lut, uint32_t launch, float convergence)
{
    extern __shared__ float4 smem4[];
    const uint32_t which = batch_image_of(img, n_images, blockIdx.x);
    if (stop[which]) return;                                         // (the whole workgroup: `which` is uniform)
    const BatchImage im = img[which];
    const uint32_t wg = blockIdx.x - im.first_wg, k = im.k;
    const uint32_t kpad = (k + 3u) & ~3u;
    float4 *s_cent = smem4;
    unsigned long long *bins = reinterpret_cast<unsigned long long *>(smem4 + kpad);
    float *s_lut = reinterpret_cast<float *>(bins + 4ull * k);
    const Centroid *cent = im.cent + (size_t)(launch ? (launch - 1u) & 1u : 0u) * k;
    Centroid *cent_out = im.cent + (size_t)(launch & 1u) * k;
    const int64_t *acc_in = im.acc + (size_t)((launch + 2u) % 3u) * 4u * k;
    int64_t *acc_out = im.acc + (size_t)(launch % 3u) * 4u * k;
    int64_t *acc_clear = im.acc + (size_t)((launch + 1u) % 3u) * 4u * k;

    s_lut[threadIdx.x] = lut[threadIdx.x];
    stage_centroids(s_cent, cent, k, kpad);
    if (launch) {
        __shared__ uint32_t s_conv;
        const long long *sums = reinterpret_cast<const long long *>(bins);
        for (uint32_t i = threadIdx.x; i < 4 * k; i += kBlock) bins[i] = (unsigned long long)acc_in[i];
        const uint32_t n_fixed = im.state[kFixedWord];                // (0: a batch has no frozen centroid)
        if (threadIdx.x == 0) s_conv = n_fixed;
        __syncthreads();
        // (update_centroids of kmg_device.h, operation for operation, on the LDS copy)
        uint32_t mine = 0;
        for (uint32_t c = threadIdx.x; c < k; c += kBlock) {
            const float4 prev = s_cent[c];
            float4 now = prev;
            const long long count = sums[4ull * c + 3];
            if (count > 0 && c >= n_fixed) {                            // choose_centroid.wgsl:185
                float nw[3];
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    double mean = ((double)sums[4ull * c + q] / (double)count) * (1.0 / 1048576.0);
                    nw[q] = (float)mean;                             // :186
                }
                now = make_float4(nw[0], nw[1], nw[2], chroma(nw[1], nw[2]));
                if (cie94(nw[0], nw[1], nw[2], prev.x, prev.y, prev.z) < convergence) mine += 1;   // :191
            }                                                        // :192-194 empty: unchanged, 0
            s_cent[c] = now;
            if (wg == 0u) { Centroid o; o.L = now.x; o.a = now.y; o.b = now.z; o.C = now.w; cent_out[c] = o; }
        }
        if (mine) atomicAdd(&s_conv, mine);
        __syncthreads();
        if (wg == 0u && threadIdx.x == 0) im.state[0] = s_conv;       // :196-202
    }
    if (wg == 0u)
        for (uint32_t i = threadIdx.x; i < 4 * k; i += kBlock) acc_clear[i] = 0;
    for (uint32_t i = threadIdx.x; i < 4 * k; i += kBlock) bins[i] = 0ull;
    __syncthreads();

    // (every thread scans, a thread past the image's end with pixel 0 as in k_assign: the near-tie repair works wave-wide)
    const uint32_t i = wg * kBlock + threadIdx.x;
    float L[1], A[1], B[1];
    PixelTerms pt[1];
    px_to_lab(s_lut, i < im.n ? im.rgba[i] : 0u, L[0], A[0], B[0]);
    pt[0] = pixel_terms(L[0], A[0], B[0]);
    // find_centroid.wgsl:29-41: min_distance = 100000.0 (squared here), found_index = 0, strict '<': the first minimum wins
    float best[1] = {1.0e10f};
    uint32_t idx[1] = {0u};
    if (SCAN == kScanChunked || (SCAN == kScanByImage && k >= 32u)) argmin_scan<1, true, false>(pt, best, idx, s_cent, k, kpad);
    else argmin_scan<1, false, false>(pt, best, idx, s_cent, k, kpad);
    if (i < im.n) {
        unsigned long long *bin = bins + 4ull * idx[0];
        atomicAdd(bin + 0, (unsigned long long)(long long)lab_fix(L[0]));
        atomicAdd(bin + 1, (unsigned long long)(long long)lab_fix(A[0]));
        atomicAdd(bin + 2, (unsigned long long)(long long)lab_fix(B[0]));
        atomicAdd(bin + 3, 1ull);
    }
    __syncthreads();
    unsigned long long *to = reinterpret_cast<unsigned long long *>(acc_out);
    for (uint32_t q = threadIdx.x; q < 4 * k; q += kBlock) {
        const unsigned long long v = bins[q];
        if (v) atomicAdd(to + q, v);                                 // (only the clusters this workgroup met)
    }
}

// The images' final centroids, concatenated: the buffer an image's last launch wrote, stop[image] - 1 being that launch.  cent0:
// the first image's centroid buffers -- the images' pairs of buffers lie one behind the other, so an image whose pair starts 2 s
// centroids behind cent0 has s centroids of earlier images before its own in `out`.
__global__ __launch_bounds__(kBlock) void k_batch_gather(const BatchImage *__restrict__ img, const uint32_t *__restrict__ stop,
                                                         const Centroid *__restrict__ cent0, Centroid *__restrict__ out)
{
    const BatchImage im = img[blockIdx.x];
    const uint32_t k = im.k;
    const Centroid *from = im.cent + (size_t)((stop[blockIdx.x] - 1u) & 1u) * k;
    Centroid *to = out + (size_t)(im.cent - cent0) / 2u;
    for (uint32_t c = threadIdx.x; c < k; c += kBlock) to[c] = from[c];
}

}  // namespace kmg

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
namespace {

// the batch takes working images below this many pixels: the PPT = 1 tiling of the small-image route (kmg_kernels.hip assign_ppt)
constexpr uint64_t kBatchMaxPixels = 1ull << 19;
// (workgroups of one batched launch at most: kBatchMaxGrid, kmg_batch_layout.h)

// plus_plus_init.wgsl:161-168 `initial`: the pixel that kmg_init_first_key(w, h) names
uint32_t first_pixel_of(uint32_t w, uint32_t h)
{
    const uint32_t low = (uint32_t)kmg_init_first_key(w, h);
    return (low & ~15u) | (15u - (low & 15u));
}

// One piece of a batch through the batched kernels: images idx[0 .. m) of the caller's arrays, each below kBatchMaxPixels; image
// i has ks[i] colours and its table starts at centroids4[at[i]].  Returns with the stream drained and the piece's state back with
// the processor.
int batch_run(kmg_processor *p, const uint32_t *idx, uint32_t m, const uint8_t *const *d_rgba, const uint32_t *widths, const uint32_t *heights,
              const uint32_t *ks, const size_t *at, float *centroids4, uint32_t *iterations, uint32_t *launches, hipStream_t st)
{
    const kmg_options &o = p->opt;
    // the piece's counts: before[q] = the colours of its images before q; k = the largest, k_low = the smallest
    std::vector<size_t> before(m + 1u, 0);
    uint32_t k = 0, k_low = 0xFFFFFFFFu;
    for (uint32_t q = 0; q < m; ++q) {
        const uint32_t kq = ks[idx[q]];
        before[q + 1u] = before[q] + kq;
        k = std::max(k, kq); k_low = std::min(k_low, kq);
    }
    const size_t k_sum = before[m];
    // the layout of the piece's block
    std::vector<BatchImage> rec(m);
    size_t off = 0;
    auto room = [&](size_t bytes) { const size_t at = off; off += pad256(bytes); return at; };
    const size_t at_rec = room(sizeof(BatchImage) * m);
    const size_t at_stop = room(sizeof(uint32_t) * m);               // stop, state and sums: one memset
    const size_t at_state = room(sizeof(uint32_t) * kStateWords * m);
    const size_t at_acc = room(sizeof(int64_t) * 12ull * k_sum);
    const size_t zero_bytes = off - at_stop;
    const size_t at_cent = room(sizeof(Centroid) * 2ull * k_sum);
    const size_t at_out = room(sizeof(Centroid) * k_sum);
    std::vector<size_t> at_slots(m), at_dist(m);
    uint64_t grid = 0;
    for (uint32_t q = 0; q < m; ++q) {
        const uint64_t n = (uint64_t)widths[idx[q]] * heights[idx[q]], tiles = (n + kBlock - 1) / kBlock;
        at_slots[q] = room(sizeof(unsigned long long) * 2ull * tiles);
        at_dist[q] = room(sizeof(float) * n);
        rec[q].n = (uint32_t)n;
        rec[q].first_wg = (uint32_t)grid;
        rec[q].first_pixel = first_pixel_of(widths[idx[q]], heights[idx[q]]);
        rec[q].k = ks[idx[q]];
        grid += tiles;
    }
    ArenaGuard blk;
    {
        const hipError_t e = blk.acquire(p, off);
        if (e != hipSuccess) { blk.base = nullptr; return fail_hip(e, "batch state allocation"); }
    }
    uint8_t *base = (uint8_t *)blk.base;
    for (uint32_t q = 0; q < m; ++q) {
        rec[q].rgba = (const uint32_t *)d_rgba[idx[q]];
        rec[q].dist = (float *)(base + at_dist[q]);
        rec[q].slots = (unsigned long long *)(base + at_slots[q]);
        rec[q].cent = (Centroid *)(base + at_cent) + 2ull * before[q];
        rec[q].acc = (int64_t *)(base + at_acc) + 12ull * before[q];
        rec[q].state = (uint32_t *)(base + at_state) + (size_t)kStateWords * q;
    }
    const BatchImage *d_rec = (const BatchImage *)(base + at_rec);
    uint32_t *d_stop = (uint32_t *)(base + at_stop);
    const uint32_t *d_state = (const uint32_t *)(base + at_state);
    Centroid *d_out = (Centroid *)(base + at_out);
    // (from here on the stream has work on the block: every early return drains it before the guard gives the block back)
    HIP_TRY_DRAIN(st, upload_host_copy(base + at_rec, rec.data(), sizeof(BatchImage) * m, st));
    HIP_TRY_DRAIN(st, hipMemsetAsync(d_stop, 0, zero_bytes, st));

    // initialisation: passes 1 .. k - 1 of every image that has them, then the last centroid -- k launches whatever m is
    uint32_t n_launches = 0;
    for (uint32_t j = 1; j < k; ++j, ++n_launches) {
        hipLaunchKernelGGL(k_batch_init_pass, dim3((uint32_t)grid), dim3(kBlock), 0, st, d_rec, m, p->d_lut, j);
        HIP_TRY_DRAIN(st, hipGetLastError());
    }
    hipLaunchKernelGGL(k_batch_init_pick, dim3(m), dim3(kBlock), 0, st, d_rec, p->d_lut);
    HIP_TRY_DRAIN(st, hipGetLastError());
    ++n_launches;

    // the loop of kmg_lloyd_run's small-image route (operations.rs:75-83, modules.rs:769-836), for all images at once
    const uint32_t kpad = (k + 3u) & ~3u;
    const size_t lds = sizeof(float4) * kpad + 256 * sizeof(float) + sizeof(unsigned long long) * 4ull * k;
    auto step = [&](uint32_t l) {
        with_value<kScanChunked, kScanPlain, kScanByImage>(k_low >= 32u ? kScanChunked : k < 32u ? kScanPlain : kScanByImage, [&](auto SCAN) {
            hipLaunchKernelGGL((k_batch_assign<SCAN()>), dim3((uint32_t)grid), dim3(kBlock), lds, st, d_rec, m, d_stop, p->d_lut, l, o.convergence);
        });
        ++n_launches;
        return hipGetLastError();
    };
    std::vector<uint32_t> stop(m, 0u), its(m, 0u), state((size_t)kStateWords * m);
    uint32_t running = m;
    HIP_TRY_DRAIN(st, step(0u));                                      // the initial assignment
    for (uint32_t it = 0; it < o.max_iterations && running; ++it) {  // modules.rs:769: update (:773-788), re-assign (:793-800)
        const uint32_t l = it + 1u;
        HIP_TRY_DRAIN(st, step(l));
        if (!(it > 0 && it % o.check_period == 0)) continue;         // :802
        HIP_TRY_DRAIN(st, hipMemcpyAsync(state.data(), d_state, sizeof(uint32_t) * state.size(), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        bool stopped = false;
        for (uint32_t q = 0; q < m; ++q)
            if (!stop[q] && state[(size_t)kStateWords * q] >= rec[q].k) {   // :826-831
                stop[q] = l + 1u;
                its[q] = it;
                --running;
                stopped = true;
            }
        if (stopped && running) HIP_TRY_DRAIN(st, upload_host_copy(d_stop, stop.data(), sizeof(uint32_t) * m, st));
    }
    // the images that ran to max_iterations: their last launch is that one's
    for (uint32_t q = 0; q < m; ++q)
        if (!stop[q]) {
            stop[q] = o.max_iterations + 1u;
            its[q] = o.max_iterations - 1u;
        }
    std::vector<Centroid> cent(k_sum);
    HIP_TRY_DRAIN(st, upload_host_copy(d_stop, stop.data(), sizeof(uint32_t) * m, st));
    hipLaunchKernelGGL(k_batch_gather, dim3(m), dim3(kBlock), 0, st, d_rec, d_stop, (const Centroid *)(base + at_cent), d_out);
    HIP_TRY_DRAIN(st, hipGetLastError());
    HIP_TRY_DRAIN(st, hipMemcpyAsync(cent.data(), d_out, sizeof(Centroid) * cent.size(), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (uint32_t q = 0; q < m; ++q) {
        float *c4 = centroids4 + at[idx[q]];
        for (uint32_t c = 0; c < rec[q].k; ++c) {
            const Centroid &v = cent[before[q] + c];
            c4[4 * c] = v.L; c4[4 * c + 1] = v.a; c4[4 * c + 2] = v.b; c4[4 * c + 3] = 1.0f;
        }
        if (iterations) iterations[idx[q]] = its[q];
    }
    *launches += n_launches;
    return KMG_OK;
}

}  // namespace

int kmg::dev_palette_batch_counts(kmg_processor *p, uint32_t n_images, const uint8_t *const *d_rgba, const uint32_t *widths,
                                  const uint32_t *heights, const uint32_t *ks, float *centroids4, uint32_t *iterations,
                                  kmg_batch_report *report, hipStream_t st)
{
    HIP_TRY(hipSetDevice(p->device));
    kmg_batch_report rep = {0u, 0u, 1u, 0u};
    std::vector<uint32_t> its(n_images, 0u), piece;
    std::vector<size_t> at(n_images, 0);
    for (uint32_t i = 1; i < n_images; ++i) at[i] = at[i - 1] + 4ull * ks[i - 1];
    uint64_t grid = 0;
    auto flush = [&]() -> int {
        if (piece.empty()) return KMG_OK;
        KMG_TRY(batch_run(p, piece.data(), (uint32_t)piece.size(), d_rgba, widths, heights, ks, at.data(), centroids4, its.data(), &rep.launches, st));
        piece.clear();
        grid = 0;
        return KMG_OK;
    };
    for (uint32_t i = 0; i < n_images; ++i) {
        const uint64_t n = (uint64_t)widths[i] * heights[i];
        if (n >= kBatchMaxPixels) {
            // a large working image: the per-image path (its own choice of route; the same results by the library's guarantee)
            LloydGuard g;
            KMG_TRY(lloyd_create_impl(p, ks[i], &g.s, st));
            KMG_TRY(kmg_lloyd_init_centroids(g.s, d_rgba[i], widths[i], heights[i], st));
            KMG_TRY(kmg_lloyd_run(g.s, d_rgba[i], n, nullptr, &its[i], st));
            KMG_TRY(kmg_lloyd_get_centroids(g.s, centroids4 + at[i], st));
            ++rep.fallback;
            continue;
        }
        const uint64_t tiles = (n + kBlock - 1) / kBlock;
        if (grid + tiles > kBatchMaxGrid) KMG_TRY(flush());
        piece.push_back(i);
        grid += tiles;
    }
    KMG_TRY(flush());
    for (uint32_t i = 0; i < n_images; ++i) {
        rep.iterations = std::max(rep.iterations, its[i]);
        if (iterations) iterations[i] = its[i];
    }
    if (report) *report = rep;
    return KMG_OK;
}

// (the case where every image has k colours)
int kmg::dev_palette_batch(kmg_processor *p, uint32_t n_images, const uint8_t *const *d_rgba, const uint32_t *widths, const uint32_t *heights,
                           uint32_t k, float *centroids4, uint32_t *iterations, kmg_batch_report *report, hipStream_t st)
{
    KMG_TRY(check_batch_prefix(p, n_images, !d_rgba || !widths || !heights || !centroids4, "bad palette_batch arguments", d_rgba, widths, heights));
    KMG_TRY(check_k(k));
    const std::vector<uint32_t> ks(n_images, k);
    return dev_palette_batch_counts(p, n_images, d_rgba, widths, heights, ks.data(), centroids4, iterations, report, st);
}

extern "C" int kmg_dev_palette_batch(kmg_processor *p, uint32_t n_images, const uint8_t *const *d_rgba, const uint32_t *widths,
                                     const uint32_t *heights, uint32_t k, float *centroids4, uint32_t *iterations,
                                     kmg_batch_report *report, void *stream)
try {
    return dev_palette_batch(p, n_images, d_rgba, widths, heights, k, centroids4, iterations, report, S(stream));
}
KMG_ABI_CATCH

extern "C" int kmg_dev_palette_batch_counts(kmg_processor *p, uint32_t n_images, const uint8_t *const *d_rgba, const uint32_t *widths,
                                            const uint32_t *heights, const uint32_t *ks, float *centroids4, uint32_t *iterations,
                                            kmg_batch_report *report, void *stream)
try {
    KMG_TRY(check_batch_prefix(p, n_images, !d_rgba || !widths || !heights || !ks || !centroids4, "bad palette_batch arguments", d_rgba, widths, heights));
    for (uint32_t i = 0; i < n_images; ++i) KMG_TRY(check_k(ks[i]));
    return dev_palette_batch_counts(p, n_images, d_rgba, widths, heights, ks, centroids4, iterations, report, S(stream));
}
KMG_ABI_CATCH
