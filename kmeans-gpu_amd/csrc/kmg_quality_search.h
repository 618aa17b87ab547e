// kmg_quality_search.h -- the schedule of kmg_reduce_quality's search for the colour count, one image at a time, so that a batch
// can run many searches in lock step (kmg_reduce_quality_batch, kmg_api.hip).  Host only, no device, no
// processor: plain C++ that a host test can include (tests/native/check_quality_search.cpp).
//
// The search is the FIXED bisection of kmg_reduce_quality, not an optimum: k_max first -- not accepted: done, k* = k_max, not
// reached --, then lo = k_min, hi = k_max and, while lo < hi, mid = lo + (hi - lo) / 2: accepted -> hi = mid, else lo = mid + 1;
// k* = hi.  Every count the search asks for depends on the earlier answers alone, so an image's sequence of counts is the same
// whether its rounds run one after the other or beside other images' rounds.
#pragma once

#include <stdint.h>

namespace kmg {

struct QualitySearch {
    uint32_t lo, hi;
    bool first = true;           // the next count is k_max's
    bool reached = false;        // k_max was accepted
    QualitySearch(uint32_t k_min, uint32_t k_max) : lo(k_min), hi(k_max) {}
    // nothing more to evaluate: k_star() and reached are final
    bool done() const { return !first && (!reached || lo >= hi); }
    // the count of the next evaluation (!done())
    uint32_t next() const { return first ? hi : lo + (hi - lo) / 2; }
    // The answer for next().  true: that evaluation is the best so far -- its palette and record are the ones to keep (k_max's
    // whatever the answer, then every accepted count).
    bool take(bool accepted)
    {
        if (first) {
            first = false;
            reached = accepted;
            return true;
        }
        const uint32_t mid = next();
        if (accepted) hi = mid;
        else lo = mid + 1;
        return accepted;
    }
    uint32_t k_star() const { return hi; }
};

// evaluations of one search at most: 1 + ceil(log2(k_max - k_min + 1))
inline uint32_t quality_search_max_rounds(uint32_t k_min, uint32_t k_max)
{
    uint32_t rounds = 1;
    for (uint64_t span = 1; span < (uint64_t)k_max - k_min + 1; span *= 2) ++rounds;
    return rounds;
}

}  // namespace kmg
