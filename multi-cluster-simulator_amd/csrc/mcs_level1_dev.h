// mcs_level1_dev.h — device code the Level1 kernels share (mcs_level1.hip, mcs_stream.hip): the member
// test, the candidates' upper bound hi(t) and the small-node time over the list.  The definitions are
// those heading mcs_level1.hip; every function reads wait_prep_kernel's records
// {h, m, s, a} of one cluster, addressed from its row 0.
#pragma once
#include "mcs_internal.h"

namespace mcs {

constexpr uint32_t kLevel1None = 0xFFFFFFFFu;

__device__ __forceinline__ bool is_member(const uint4& r, uint32_t t) { return r.y <= t && t < r.z; }

// the first row in [lo, J) with m > t (m is non-decreasing): the candidates at t are [0, hi)
__device__ __forceinline__ uint32_t level1_hi(const uint4* __restrict__ rec, uint32_t lo, uint32_t J, uint32_t t) {
    uint32_t hi = J;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (rec[mid].y <= t) lo = mid + 1u;
        else hi = mid;
    }
    return lo;
}

// the same along a tile, from the previous sample's hi (hi only moves up): one row of 64 loads tells
// the rows a sample period lets in, which is nearly always all of them, and the bisection takes the
// rest (each wave finds the same hi; a bisection per sample is about 20 dependent loads, which was
// all the time of a run whose Level1 stays empty)
__device__ __forceinline__ uint32_t level1_hi_next(const uint4* __restrict__ rec, uint32_t hi, uint32_t J, uint32_t t,
                                                   uint32_t lane) {
    const uint64_t j = (uint64_t)hi + lane;
    uint32_t m = kLevel1None;  // past the stream's end: beyond every sample second
    if (j < J) m = rec[j].y;
    const uint32_t n = (uint32_t)__popcll(__ballot(m <= t));  // a prefix of the lanes: m is sorted
    if (n < (uint32_t)kWave) return hi + n;
    return level1_hi(rec, hi + (uint32_t)kWave, J, t);  // (hi + 64 <= J: all 64 rows exist)
}

// calculateSmallNodeSize's time over the list padded to a multiple of 20: the recurrence
// ct = ct < d ? d : 0.  A padding job resets it, so it is 0 unless len % 20 == 0 (the caller's test);
// then it is the last member's duration when the trailing run of falls (d_prev >= d_cur) has even
// length, else 0 (mcs_dtrade_dev.h states the same closed form over the live list).  One wave walks
// back from the last member over the rows down to the head, 64 at a time; rows that are no members
// are stepped over, batches that have left Level1 are skipped by their summary.
__device__ __forceinline__ uint32_t level1_small_time(const uint4* __restrict__ rec, const uint4* __restrict__ jobs,
                                                      const uint32_t* __restrict__ summ, uint32_t head,
                                                      uint32_t last, uint32_t t, uint32_t lane) {
    const uint32_t d_last = jobs[last].y;
    uint32_t cur = d_last, run = 0u, top = last;  // rows [head, top) are still to be walked
    bool done = false;
    while (!done && top > head) {
        const uint32_t b = (top - 1u) / kSeriesBatch;
        if (summ[b] <= t) {  // (never the head's batch: the head is a member)
            top = b * kSeriesBatch;
            continue;
        }
        uint32_t base = top > (uint32_t)kWave ? top - (uint32_t)kWave : 0u;
        if (base < head) base = head;
        const uint32_t j = base + lane;
        bool mem = false;
        uint32_t d = 0u;
        if (j < top) {
            mem = is_member(rec[j], t);
            if (mem) d = jobs[j].y;
        }
        unsigned long long mask = __ballot(mem);
        while (mask) {  // members of this row, last first
            const uint32_t bit = 63u - (uint32_t)__builtin_clzll(mask);
            mask &= ~(1ull << bit);
            const uint32_t dp = __shfl(d, (int)bit);
            if (dp >= cur) {
                ++run;
                cur = dp;
            } else {
                done = true;
                break;
            }
        }
        top = base;
    }
    return (run & 1u) == 0u ? d_last : 0u;
}

}  // namespace mcs
