// mcs_wait_dev.h — device code the wait-time kernels share (mcs_wait.hip, mcs_stream.hip): the clamp
// scan of d_j, the search for the entry a Level1 placement steps over (D6) and a job's additions to
// the sample accumulators.  The formulas are those heading mcs_wait.hip.
#pragma once
#include "mcs_internal.h"

namespace mcs {

constexpr uint32_t kWaitNone = 0xFFFFFFFFu;
constexpr long long kWaitInf = 1ll << 60;  // s of a job that is never placed; beyond every a + W + J

// x -> max(lo, min(hi, x + c)), lo <= hi
struct Clamp {
    long long lo, hi;
    uint32_t c;
};

__device__ __forceinline__ long long clamp_apply(const Clamp& e, long long x) {
    const long long y = x + (long long)e.c;
    const long long z = y < e.hi ? y : e.hi;
    return z > e.lo ? z : e.lo;
}

// `first`, then `second`: the bounds of `first`, shifted, clamped by `second`
__device__ __forceinline__ Clamp clamp_then(const Clamp& first, const Clamp& second) {
    Clamp r;
    r.lo = clamp_apply(second, first.lo);
    r.hi = clamp_apply(second, first.hi);
    r.c = first.c + second.c;
    return r;
}

__device__ __forceinline__ uint32_t sat32(long long x) {
    return x >= (long long)kWaitNone ? kWaitNone : (uint32_t)x;
}

// One round of the scan over the 256 jobs of a workgroup: thread i holds the clamp e of its job (the
// identity {-kWaitInf, kWaitInf, 0} for none), carry is d of the job before the round's first.
// Returns d of the thread's job and, in dprev, d of the job before it.  wave_tot: 4 LDS entries; the
// caller synchronises before the next round rewrites them.
__device__ __forceinline__ long long clamp_scan_round(const Clamp& e, long long carry, Clamp* wave_tot,
                                                      long long& dprev) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    Clamp inc = e;  // inclusive scan over the wave
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
        Clamp p;
        p.lo = __shfl_up(inc.lo, o);
        p.hi = __shfl_up(inc.hi, o);
        p.c = __shfl_up(inc.c, o);
        if (lane >= (uint32_t)o) inc = clamp_then(p, inc);
    }
    if (lane == 63u) wave_tot[wave] = inc;
    __syncthreads();
    long long x = carry;  // d of the job before this wave's first
    for (uint32_t w = 0; w < wave; ++w) x = clamp_apply(wave_tot[w], x);
    const long long d = clamp_apply(inc, x);
    dprev = __shfl_up(d, 1);
    if (lane == 0u) dprev = x;
    return d;
}

// The entry that the Level1 placement of job P steps over, and the length of that entry's run of
// skipped seconds: {k, run}, {kWaitNone, 0} when P is no Level1 placement or steps over nothing.
// rec: the cluster's records {h, m, s, a}, J of them.
__device__ __forceinline__ uint2 wait_skip_of(const uint4* __restrict__ rec, uint32_t P, uint32_t J) {
    uint2 res = make_uint2(kWaitNone, 0u);
    const uint4 rp = rec[P];
    const uint32_t u = rp.z;
    if (u != kWaitNone && u > rp.y) {  // placed by the Level1 pass at u
        // the entry behind P in Level1 at u: moved before u, not started before u; every job
        // from the first with h >= u on has not reached the head yet
        uint32_t k = kWaitNone, mk = 0u;
        for (uint32_t q = P + 1u; q < J; ++q) {
            const uint4 r = rec[q];
            if (r.x >= u) break;
            if (r.y < u && r.z >= u) {
                k = q;
                mk = r.y;
                break;
            }
        }
        if (k != kWaitNone) {
            // k was also stepped over at u - r iff it was in Level1 then (m_k < u - r) and an
            // entry between the placement that skipped it at u - r + 1 and k started at u - r:
            // the last such entry stood right before k
            uint32_t r = 1u, lo = P;
            while (r <= u) {
                const uint32_t tg = u - r;
                if (mk >= tg) break;
                uint32_t f = kWaitNone;
                for (uint32_t q = k - 1u; q > lo; --q) {
                    const uint4 x = rec[q];
                    if (x.z == tg && tg > x.y) {
                        f = q;
                        break;
                    }
                }
                if (f == kWaitNone) break;
                ++r;
                lo = f;
            }
            res = make_uint2(k, r);
        }
    }
    return res;
}

// a sample row as accumulators: [0] skip (pointwise), [1] A and [2] B (differences along the samples)
__device__ __forceinline__ unsigned long long* acc_of(mcs_wait_sample* s) {
    return reinterpret_cast<unsigned long long*>(s);
}

// One thread's additions to a cluster's row of n samples t_first + k * period.  Every job before the
// samples lands on sample 0: those differences are summed in registers and leave with one atomic per
// wave (flush, called by every lane of the wave).
struct WaitAcc {
    mcs_wait_sample* row;
    uint32_t n, period, t_first;
    unsigned long long pre_a = 0, pre_b = 0;

    // index of the first sample at or after x, n when there is none
    __device__ __forceinline__ uint32_t kt(uint32_t x) const {
        if (x <= t_first) return 0u;
        const uint32_t q = (x - t_first - 1u) / period;
        return q >= n ? n : q + 1u;
    }
    __device__ __forceinline__ void add(uint32_t k, unsigned long long da, unsigned long long db) {
        if (k == 0u) {
            pre_a += da;
            pre_b += db;
        } else {
            atomicAdd(acc_of(row + k) + 1, da);
            if (db) atomicAdd(acc_of(row + k) + 2, db);
        }
    }
    // the job with record r = {h, m, s, a}; ev() gives {k, run} of its Level1 placement (wait_skip_of)
    // and is called only when that placement falls on a sample
    template <class EV>
    __device__ __forceinline__ void job(const uint4& r, EV&& ev) {
        const uint32_t kh = kt(r.x);
        if (kh >= n) return;  // h <= s: neither falls on a sample
        const uint32_t ks = r.z != kWaitNone ? kt(r.z) : n;
        if (ks == kh) {  // reaches the head and starts within one sample: s - a for good
            add(kh, (unsigned long long)r.z - (unsigned long long)r.w, 0ull);
        } else {
            add(kh, 0ull - (unsigned long long)r.w, 1ull);
            if (ks < n) add(ks, (unsigned long long)r.z, ~0ull);
        }
        if (r.z != kWaitNone && r.z > r.y && r.z >= t_first) {  // a Level1 placement: its skip at u = s
            const uint32_t y = r.z - t_first, q = y / period;
            if (q < n && q * period == y) {
                const uint2 e = ev();
                if (e.x != kWaitNone) atomicAdd(acc_of(row + q), (unsigned long long)e.y);
            }
        }
    }
    __device__ __forceinline__ void flush() {
        for (int o = 32; o > 0; o >>= 1) {
            pre_a += __shfl_xor(pre_a, o);
            pre_b += __shfl_xor(pre_b, o);
        }
        if ((threadIdx.x & 63u) == 0u) {
            if (pre_a) atomicAdd(acc_of(row) + 1, pre_a);
            if (pre_b) atomicAdd(acc_of(row) + 2, pre_b);
        }
    }
};

}  // namespace mcs
