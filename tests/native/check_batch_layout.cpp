// check_batch_layout.cpp -- the host arithmetic of the batches: the packed blocks, the grid and its cuts into launches, the cuts of a
// batch into sub-batches (csrc/kmg_batch_layout.h) and the rule for which images join the launch (csrc/kmg_apply_route.h batch_apply_joins), the latter over
// the grid of (mode, k, n, forced, mask_words) of apply_route_table.txt, which check_apply_route.cpp walks.  Stops at the first
// difference.  Host code only: built plain and with -fsanitize=address,undefined by tests/test_batch_layout.py.
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "kmg_apply_route.h"
#include "kmg_batch_layout.h"

#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) { printf("line %d: %s\n", __LINE__, #cond); return 1; }          \
    } while (0)

static int check_layout()
{
    using namespace kmg;
    // pixel counts 1 .. 40 in mixed order, every format: aligned offsets, no overlap, the total
    std::vector<uint64_t> pixels;
    for (uint64_t i = 0; i < 40; ++i) pixels.push_back(1 + (i * 17) % 40);
    for (const uint32_t bpp : {1u, 2u, 4u}) {
        std::vector<uint64_t> off;
        uint64_t total = 0;
        CHECK(batch_offsets(pixels.data(), (uint32_t)pixels.size(), bpp, off, &total));
        CHECK(off.size() == pixels.size() && off[0] == 0);
        for (size_t i = 0; i < off.size(); ++i) {
            CHECK(off[i] % 16 == 0);
            const uint64_t end = off[i] + pixels[i] * bpp;
            CHECK(end <= (i + 1 < off.size() ? off[i + 1] : total));
            CHECK((i + 1 < off.size() ? off[i + 1] : total) - end < 16);      // (packed: less than one alignment step of padding)
        }
        CHECK(total % 16 == 0);
    }
    // the grid: first workgroups in order, their sum, for the tiles of 1024 and 2048 pixels
    const std::vector<uint64_t> sizes = {1, 2047, 2048, 2049, 1023, 1024, 1025, 43776, 5, 4096};
    for (const uint64_t tile : std::vector<uint64_t>{1024, 2048}) {
        std::vector<uint32_t> first;
        uint64_t grid = 0, sum = 0;
        CHECK(batch_grid(sizes.data(), (uint32_t)sizes.size(), tile, first, &grid));
        for (size_t i = 0; i < sizes.size(); ++i) {
            CHECK(first[i] == sum);
            sum += (sizes[i] + tile - 1) / tile;
        }
        CHECK(grid == sum);
        CHECK(grid == first.back() + (sizes.back() + tile - 1) / tile);
    }
    // the cuts into launches at the piece bound: in order, each at most the bound, covering the grid once
    for (const uint64_t grid : std::vector<uint64_t>{1, kBatchMaxGrid - 1, kBatchMaxGrid, kBatchMaxGrid + 1, 2 * kBatchMaxGrid, 3 * kBatchMaxGrid + 7, 1049400}) {
        const std::vector<BatchLaunch> cuts = batch_launches(grid);
        CHECK(cuts.size() == (grid + kBatchMaxGrid - 1) / kBatchMaxGrid);
        uint64_t at = 0;
        for (const BatchLaunch &c : cuts) {
            CHECK(c.first == at && c.count >= 1 && c.count <= kBatchMaxGrid);
            at += c.count;
        }
        CHECK(at == grid);
    }
    CHECK(batch_launches(0).empty());
    CHECK(batch_launches(10, 4).size() == 3 && batch_launches(10, 4)[2].first == 8 && batch_launches(10, 4)[2].count == 2);
    // totals that do not fit are refused: a product beyond 64 bits, a sum beyond 64 bits, a block beyond the caller's limit, a grid
    // beyond the 32 bits of the first-workgroup column
    {
        std::vector<uint64_t> off;
        std::vector<uint32_t> first;
        uint64_t total = 0, grid = 0;
        const uint64_t huge[2] = {1ull << 62, 1ull << 62};
        CHECK(!batch_offsets(huge, 1, 4, off, &total));
        CHECK(batch_offsets(huge, 1, 2, off, &total) && total == 1ull << 63);
        CHECK(!batch_offsets(huge, 2, 2, off, &total));
        const uint64_t two[2] = {100, 100};
        CHECK(batch_offsets(two, 2, 1, off, &total, 224) && total == 224 && off[1] == 112);
        CHECK(!batch_offsets(two, 2, 1, off, &total, 223));
        const uint64_t wide[2] = {0xFFFFFFFFull * 2048, 2048};
        CHECK(batch_grid(wide, 1, 2048, first, &grid) && grid == 0xFFFFFFFFull);
        CHECK(!batch_grid(wide, 2, 2048, first, &grid));
    }
    return 0;
}

// the greedy rule of the sub-batches, written out once more (sums that cannot wrap here: the callers keep them small)
static std::vector<uint32_t> expected_cuts(const std::vector<uint64_t> &bytes, uint64_t bound)
{
    std::vector<uint32_t> cuts(1, 0u);
    uint64_t held = 0;
    for (uint32_t i = 0; i < bytes.size(); ++i) {
        if (i > cuts.back() && held + bytes[i] > bound) { cuts.push_back(i); held = 0; }
        held += bytes[i];
    }
    cuts.push_back((uint32_t)bytes.size());
    return cuts;
}

static int check_cuts()
{
    using namespace kmg;
    std::vector<uint64_t> bytes;
    uint64_t sum = 0;
    for (uint64_t i = 0; i < 40; ++i) { bytes.push_back(1 + (i * 17) % 40); sum += bytes.back(); }
    const uint32_t n = (uint32_t)bytes.size();
    // everything fits: one sub-batch; a bound below every image: one image each
    CHECK((batch_cuts(bytes.data(), n, sum) == std::vector<uint32_t>{0, n}));
    CHECK((batch_cuts(bytes.data(), n, UINT64_MAX) == std::vector<uint32_t>{0, n}));
    const std::vector<uint64_t> big(5, 7);
    const std::vector<uint32_t> each = batch_cuts(big.data(), 5, 6);
    CHECK((each == std::vector<uint32_t>{0, 1, 2, 3, 4, 5}));
    // pixel counts 1 .. 40 in mixed order over a range of bounds: the greedy loop; [0, n) once and in order; no sub-batch of two
    // images or more above the bound, and none that the next image would still have fitted
    for (uint64_t bound = 1; bound <= sum + 1; ++bound) {
        const std::vector<uint32_t> cuts = batch_cuts(bytes.data(), n, bound);
        CHECK(cuts == expected_cuts(bytes, bound));
        CHECK(cuts.size() >= 2 && cuts.front() == 0 && cuts.back() == n);
        for (size_t s = 0; s + 1 < cuts.size(); ++s) {
            CHECK(cuts[s] < cuts[s + 1]);
            uint64_t held = 0;
            for (uint32_t i = cuts[s]; i < cuts[s + 1]; ++i) held += bytes[i];
            CHECK(held <= bound || cuts[s + 1] - cuts[s] == 1);
            CHECK(cuts[s + 1] == n || held + bytes[cuts[s + 1]] > bound);
        }
    }
    // bound == 0 is 2^30
    const uint64_t gib[4] = {1ull << 29, 1ull << 29, 1, (1ull << 30) + 5};
    CHECK(kBatchDefaultResident == 1ull << 30);
    CHECK((batch_cuts(gib, 4, 0) == std::vector<uint32_t>{0, 2, 3, 4}));
    CHECK(batch_cuts(gib, 4, 0) == batch_cuts(gib, 4, 1ull << 30));
    CHECK((batch_cuts(gib, 2, 0) == std::vector<uint32_t>{0, 2}));
    // sizes of 2^63 and above: held + bytes would wrap to a small number and join what does not fit
    const uint64_t huge[5] = {1ull << 63, 1ull << 63, 3, UINT64_MAX, 2};
    CHECK((batch_cuts(huge, 5, UINT64_MAX) == std::vector<uint32_t>{0, 1, 3, 4, 5}));
    CHECK((batch_cuts(huge, 5, 1ull << 63) == std::vector<uint32_t>{0, 1, 2, 3, 4, 5}));
    CHECK((batch_cuts(huge, 5, 10) == std::vector<uint32_t>{0, 1, 2, 3, 4, 5}));
    const uint64_t tail[3] = {4, UINT64_MAX - 4, 1};
    CHECK((batch_cuts(tail, 3, UINT64_MAX) == std::vector<uint32_t>{0, 2, 3}));
    CHECK((batch_cuts(tail, 3, UINT64_MAX - 1) == std::vector<uint32_t>{0, 1, 3}));
    return 0;
}

// the rule, written out once more: what its own plan would scan joins, and -- a batch of two images or more, forced == 0,
// 128 <= k <= 512 -- a dither image that a plan prunes only for the latency of one image's scan (n (0.255 k - 0.3) <= 45e6 ps);
// never meld or diffusion
static bool expected_join(int mode, uint32_t k, uint64_t n, int forced, int route, uint32_t n_images)
{
    if (mode == kmg::kRouteModeMeld || mode == kmg::kRouteModeDiffuse) return false;
    if (route == (int)kmg::Route::kScan) return true;
    const bool pruned = route == (int)kmg::Route::kDitherLists || route == (int)kmg::Route::kDitherMasks;
    return n_images >= 2 && forced == 0 && pruned && k >= 128 && k <= 512 && !((double)n * (0.255 * k - 0.3) > 45.0e6);
}

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: check_batch_layout apply_route_table.txt\n"); return 2; }
    if (check_layout() || check_cuts()) return 1;
    FILE *f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 2; }
    static char line[1 << 16];
    unsigned long rows = 0, points = 0, joined = 0, scan = 0, widened = 0;
    while (fgets(line, sizeof line, f)) {
        if (line[0] == '#' || line[0] == '\n') continue;
        int mode, forced, mask_words, used = 0;
        uint32_t k;
        if (sscanf(line, "%d %" SCNu32 " %d %d%n", &mode, &k, &forced, &mask_words, &used) != 4) { fprintf(stderr, "bad line: %s", line); return 2; }
        ++rows;
        const char *s = line + used;
        uint64_t n;
        int route, step;
        while (sscanf(s, " %" SCNu64 " %d%n", &n, &route, &step) == 2) {
            s += step;
            ++points;
            // (a batch of one image: exactly what its own plan would scan)
            if (kmg::batch_apply_joins(mode, k, n, forced, mask_words != 0, 1u) != expected_join(mode, k, n, forced, route, 1u) ||
                kmg::batch_apply_joins(mode, k, n, forced, mask_words != 0, 1u) != (route == (int)kmg::Route::kScan && mode != kmg::kRouteModeMeld)) {
                printf("mode %d k %" PRIu32 " n %" PRIu64 " forced %d mask_words %d route %d: a batch of one\n", mode, k, n, forced, mask_words, route);
                return 1;
            }
            const bool got = kmg::batch_apply_joins(mode, k, n, forced, mask_words != 0, 2u);
            const bool is_scan = (int)kmg::apply_route(mode, k, n, forced, mask_words != 0) == (int)kmg::Route::kScan;
            const bool replace_or_dither = mode != kmg::kRouteModeMeld && mode != kmg::kRouteModeDiffuse;
            if (got != expected_join(mode, k, n, forced, route, 2u) || got != kmg::batch_apply_joins(mode, k, n, forced, mask_words != 0, 500u) || (is_scan && replace_or_dither && !got) || (!replace_or_dither && got) ||
                (forced > 0 && got && !is_scan)) {
                printf("mode %d k %" PRIu32 " n %" PRIu64 " forced %d mask_words %d route %d: joins %d\n", mode, k, n, forced, mask_words, route, (int)got);
                return 1;
            }
            joined += got;
            scan += is_scan && replace_or_dither;
            widened += got && !is_scan;
        }
    }
    fclose(f);
    printf("layout ok; cuts ok; rows %lu points %lu joined %lu scan %lu widened %lu join_mismatches 0\n", rows, points, joined, scan, widened);
    return rows == 4 * 11 * 3 * 2 && joined == scan + widened && scan > 0 ? 0 : 1;
}
