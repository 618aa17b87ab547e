// The lock-step schedule of kmg_reduce_quality_batch (kmeans-gpu_amd/csrc/kmg_quality_search.h) against the sequential bisection
// of kmg_reduce_quality, written out here a second time as that call has it.  No device.
//   every (k_min, k_max) with 1 <= k_min <= k_max <= 40 and every monotone acceptance "k >= t", t = k_min .. k_max + 1
//   (t = k_max + 1: never accepted): the same counts in the same order, the same k*, the same `reached`, the same evaluation kept,
//   within 1 + ceil(log2(k_max - k_min + 1)) evaluations, and -- monotone -- k* = the smallest accepted count;
//   non-monotone acceptance (E(k) need not fall with k): periodic patterns and a few hundred pseudo-random sets per range, again
//   against the sequential search -- the contract is the fixed search, not the optimum;
//   a batch in lock step: searches of different ranges and thresholds advanced round by round finish with the results they have alone.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <functional>
#include <vector>

#include "kmg_quality_search.h"

using kmg::QualitySearch;

struct Result {
    std::vector<uint32_t> asked;
    uint32_t k_star = 0, kept = 0;
    bool reached = false;
    bool operator==(const Result &o) const { return asked == o.asked && k_star == o.k_star && kept == o.kept && reached == o.reached; }
};

// kmg_reduce_quality's loop, statement for statement (kmg_api.hip quality_of_working)
static Result sequential(uint32_t k_min, uint32_t k_max, const std::function<bool(uint32_t)> &accepts)
{
    Result r;
    bool ok = false;
    auto evaluate = [&](uint32_t k) { r.asked.push_back(k); ok = accepts(k); };
    uint32_t k_star = k_max;
    evaluate(k_max);
    r.kept = k_max;
    r.reached = ok;
    if (ok) {
        uint32_t lo = k_min, hi = k_max;
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo) / 2;
            evaluate(mid);
            if (ok) { hi = mid; r.kept = mid; }
            else lo = mid + 1;
        }
        k_star = hi;
    }
    r.k_star = k_star;
    return r;
}

static Result stepped(uint32_t k_min, uint32_t k_max, const std::function<bool(uint32_t)> &accepts)
{
    Result r;
    QualitySearch s(k_min, k_max);
    while (!s.done()) {
        const uint32_t k = s.next();
        r.asked.push_back(k);
        if (s.take(accepts(k))) r.kept = k;
    }
    r.k_star = s.k_star();
    r.reached = s.reached;
    return r;
}

int main()
{
    uint64_t cases = 0, failures = 0;
    auto check = [&](uint32_t k_min, uint32_t k_max, const std::function<bool(uint32_t)> &accepts, const char *what, uint32_t tag, bool monotone) {
        const Result a = sequential(k_min, k_max, accepts), b = stepped(k_min, k_max, accepts);
        bool good = a == b && b.kept == b.k_star && b.asked.size() <= kmg::quality_search_max_rounds(k_min, k_max);
        if (monotone) {                                              // the smallest accepted count, or k_max unreached
            uint32_t want = k_max;
            for (uint32_t k = k_max; k >= k_min && accepts(k); --k) want = k;
            good = good && b.k_star == want && b.reached == accepts(k_max);
        }
        ++cases;
        if (!good && failures++ < 10) printf("MISMATCH %s [%u, %u] tag %u: k* %u / %u\n", what, k_min, k_max, tag, a.k_star, b.k_star);
    };
    for (uint32_t k_min = 1; k_min <= 40; ++k_min)
        for (uint32_t k_max = k_min; k_max <= 40; ++k_max) {
            for (uint32_t t = k_min; t <= k_max + 1; ++t)
                check(k_min, k_max, [t](uint32_t k) { return k >= t; }, "monotone", t, true);
            for (uint32_t period = 2; period <= 5; ++period)
                for (uint32_t phase = 0; phase < period; ++phase)
                    check(k_min, k_max, [=](uint32_t k) { return k == k_max || k % period == phase; }, "periodic", period * 8 + phase, false);
            uint64_t s = 0x9E3779B97F4A7C15ull * (k_min * 41u + k_max);
            for (uint32_t n = 0; n < 8; ++n) {
                s = s * 6364136223846793005ull + 1442695040888963407ull;
                const uint64_t set = s >> 20;                        // bit k % 41: count k is accepted
                check(k_min, k_max, [set](uint32_t k) { return ((set >> (k % 41u)) & 1u) != 0; }, "random", n, false);
            }
        }
    // quality_search_max_rounds is 1 + ceil(log2(span))
    for (uint32_t span = 1; span <= 300; ++span) {
        uint32_t lg = 0;
        while ((1u << lg) < span) ++lg;
        ++cases;
        if (kmg::quality_search_max_rounds(5, 5 + span - 1) != 1 + lg && failures++ < 10) printf("MISMATCH rounds span %u\n", span);
    }
    // lock step: many searches advanced together, a finished one left out of later rounds
    {
        struct One { uint32_t k_min, k_max, t; };
        std::vector<One> batch;
        for (uint32_t i = 0; i < 64; ++i) batch.push_back({1 + i % 7, 8 + (i * 5) % 33, 1 + (i * 11) % 44});
        std::vector<QualitySearch> search;
        for (const One &o : batch) search.emplace_back(o.k_min, o.k_max);
        uint32_t rounds = 0, bound = 0;
        for (;; ++rounds) {
            bool any = false;
            for (size_t i = 0; i < batch.size(); ++i) {
                if (search[i].done()) continue;
                any = true;
                search[i].take(search[i].next() >= batch[i].t);
            }
            if (!any) break;
        }
        for (size_t i = 0; i < batch.size(); ++i) {
            const One &o = batch[i];
            const Result a = sequential(o.k_min, o.k_max, [&](uint32_t k) { return k >= o.t; });
            bound = std::max(bound, (uint32_t)a.asked.size());
            ++cases;
            if ((a.k_star != search[i].k_star() || a.reached != search[i].reached) && failures++ < 10) printf("MISMATCH lock step %zu\n", i);
        }
        ++cases;
        if (rounds != bound && failures++ < 10) printf("MISMATCH lock step rounds %u / %u\n", rounds, bound);
    }
    printf("search cases %llu failures %llu\n", (unsigned long long)cases, (unsigned long long)failures);
    printf(failures ? "search FAILED\n" : "search ok\n");
    return failures ? 1 : 0;
}
