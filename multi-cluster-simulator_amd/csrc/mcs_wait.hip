// mcs_wait.hip — the average wait time series of a DELAY run (mcs_wait_time_series).
//
// WaitTime.TotalTime and WaitTime.JobsCount (scheduler.go:47-63) after the Delay iteration at every
// sample second t_k = t0 + k * period, rebuilt from the last DELAY run's placements: per job the
// arrival a and the start s (none: never placed), and W = MaxWaitTime.  Serialized semantics SDELAY
// (DESIGN.md §10).  Jobs of a cluster in stream order j = 0 .. J-1, d_-1 = -1:
//   h_j = max(a_j, d_{j-1} + 1)   the first iteration that examines j (as the Level0 head)
//   m_j = max(h_j, a_j + W)       the iteration at which a head that still fails moves to Level1
//   d_j = min(s_j, m_j)           the iteration at which j leaves the head (moved_j: s_j > m_j)
// A job adds nothing to TotalTime before h_j (JobsMap holds 0), t - a_j on h_j <= t < s_j (the head
// and every Level1 entry are examined each second) and s_j - a_j from s_j on (the delete at the
// placement subtracts nothing).  So, in seconds,
//   TotalTime(t) = A(t) + t * B(t) - skip(t),   A(t) = sum_{s_j <= t} s_j - sum_{h_j <= t} a_j,
//   B(t) = #{h_j <= t} - #{s_j <= t},           JobsCount(t) = #{a_j <= t}.
// skip(t) is deviation D6: a Level1 placement of job P at u = s_P removes its entry without i--, so
// the entry that slides into its slot — the first k > P with m_k < u <= s_k — is not examined at u
// and keeps its previous value: it is short by the number of consecutive seconds .., u-1, u at
// which k was stepped over.
//
// Four kernels, one 256-thread workgroup per cluster each:
//   wait_prep_kernel    d_j = min(s_j, max(a_j + W, d_{j-1} + 1)) is a clamp of d_{j-1} + 1, and
//                       clamps compose to clamps: a scan in rounds of 256 jobs with a carried d.
//                       Writes {h, m, s, a} per job (16 B), the times saturated at 0xFFFFFFFF (past
//                       every sample second).  launch_wait_rec runs it alone: the Level1 kernels
//                       (mcs_level1.hip) read the same records.
//   wait_skip_kernel    one lane per Level1 placement P finds the entry it steps over and the length
//                       of that entry's run of skipped seconds; writes {k, run} per job (8 B).
//   wait_accum_kernel   per chunk of samples: every job adds its differences of A and B at the first
//                       sample at or after h_j and s_j, and its skip at the sample u falls on, with
//                       64-bit integer atomics into the output rows themselves (the three 8 B fields
//                       of a sample serve as accumulators; jobs before the chunk land on sample 0
//                       and are summed in registers first, one atomic per wave).
//   wait_finish_kernel  prefix sums of A and B along the samples in rounds of 256 with a carried
//                       base, JobsCount by bisection of the sorted arrivals, and the three fields.
// Every loop is bounded by J or the sample count; no workgroup waits for another.
// Each kernel has a SEG instantiation for an online session (mcs_online_state_series): J is then the
// segment's job_cnt[c], not the distance to the next segment.
#include "mcs_internal.h"
#include "mcs_wait_dev.h"
#include "mcs_wave.h"

namespace mcs {

namespace {

constexpr int kWaitThreads = 256;
constexpr uint32_t kNone = kWaitNone;
constexpr long long kInf = kWaitInf;  // s of a job that is never placed (mcs_wait_dev.h)

// The rows of cluster c.  SEG: the first job_cnt[c] rows of the segment at job_off[c] (an online
// session, mcs_online_state_series); rec and ev are addressed by the same segment starts.  A job no
// horizon has decided yet reads MCS_NODE_UNPLACED / MCS_TIME_NONE, so its s is kInf below: d is then
// exact wherever it lies below the horizon and at or above it otherwise.
template <bool SEG>
__device__ __forceinline__ uint32_t wait_rows(const WaitArgs& a, uint32_t c) {
    if constexpr (SEG)
        return a.job_cnt[c];
    else
        return (uint32_t)(a.job_off[c + 1] - a.job_off[c]);
}

template <bool SEG>
__global__ __launch_bounds__(kWaitThreads) void wait_prep_kernel(WaitArgs a) {
    __shared__ Clamp wave_tot[kWaitThreads / kWave];
    __shared__ long long carry_s;
    const uint32_t c = blockIdx.x;
    const uint32_t tid = threadIdx.x;
    const uint64_t j0 = a.job_off[c];
    const uint32_t J = wait_rows<SEG>(a, c);
    const uint4* __restrict__ jobs = a.jobs + j0;
    const int32_t* __restrict__ node = a.out_node + j0;
    const uint32_t* __restrict__ start = a.out_start + j0;
    uint4* __restrict__ rec = a.rec + (j0 - a.rec_off);
    const long long W = (long long)a.max_wait;
    long long carry = -1;  // d_{-1}
    for (uint64_t base = 0; base < J; base += kWaitThreads) {  // 64-bit: base + 256 may pass 2^32
        const uint32_t i = (uint32_t)(base + tid);
        const bool live = base + tid < J;
        Clamp e{-kInf, kInf, 0u};              // the identity
        long long arr = 0, s = kInf;
        if (live) {
            arr = (long long)jobs[i].x;
            const int32_t k = node[i];
            const uint32_t st = start[i];
            if (k >= 0 && st != kNone) s = (long long)st;
            e.hi = s;
            e.lo = arr + W < s ? arr + W : s;
            e.c = 1u;
        }
        long long dprev;
        const long long d = clamp_scan_round(e, carry, wave_tot, dprev);
        if (live) {
            const long long h = arr > dprev + 1 ? arr : dprev + 1;
            const long long m = h > arr + W ? h : arr + W;
            rec[i] = make_uint4(sat32(h), sat32(m), sat32(s), (uint32_t)arr);
        }
        if (tid == kWaitThreads - 1) carry_s = d;
        __syncthreads();
        carry = carry_s;
    }
}

template <bool SEG>
__global__ __launch_bounds__(kWaitThreads) void wait_skip_kernel(WaitArgs a) {
    const uint32_t c = blockIdx.x;
    const uint64_t j0 = a.job_off[c];
    const uint32_t J = wait_rows<SEG>(a, c);
    const uint4* __restrict__ rec = a.rec + j0;
    uint2* __restrict__ ev = a.ev + j0;
    for (uint64_t base = 0; base < J; base += kWaitThreads) {
        if (base + threadIdx.x >= J) continue;
        const uint32_t P = (uint32_t)(base + threadIdx.x);
        ev[P] = wait_skip_of(rec, P, J);
    }
}

template <bool SEG>
__global__ __launch_bounds__(kWaitThreads) void wait_accum_kernel(WaitArgs a) {
    const uint32_t c = blockIdx.x;
    const uint64_t j0 = a.job_off[c];
    const uint32_t J = wait_rows<SEG>(a, c);
    const uint4* __restrict__ rec = a.rec + j0;
    const uint2* __restrict__ ev = a.ev + j0;
    WaitAcc acc;
    acc.n = a.n_samples;
    acc.period = a.period;
    acc.t_first = a.t0;
    acc.row = a.out + (size_t)c * a.n_samples;
    for (uint64_t base = 0; base < J; base += kWaitThreads) {
        if (base + threadIdx.x >= J) continue;
        const uint32_t i = (uint32_t)(base + threadIdx.x);
        acc.job(rec[i], [&]() { return ev[i]; });  // {h, m, s, a}
    }
    acc.flush();
}

template <bool SEG>
__global__ __launch_bounds__(kWaitThreads) void wait_finish_kernel(WaitArgs a) {
    __shared__ unsigned long long wave_tot[2][kWaitThreads / kWave];
    const uint32_t c = blockIdx.x;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint64_t j0 = a.job_off[c];
    const uint32_t J = wait_rows<SEG>(a, c);
    const uint4* __restrict__ rec = a.rec + j0;
    const uint32_t n = a.n_samples;
    mcs_wait_sample* const row = a.out + (size_t)c * n;
    unsigned long long base_a = 0, base_b = 0;  // A and B before this round's first sample
    for (uint64_t k0 = 0; k0 < n; k0 += kWaitThreads) {
        const uint32_t k = (uint32_t)(k0 + tid);
        const bool live = k0 + tid < n;
        unsigned long long sk = 0, va = 0, vb = 0;
        if (live) {
            const unsigned long long* p = acc_of(row + k);
            sk = p[0];
            va = p[1];
            vb = p[2];
        }
#pragma unroll
        for (int o = 1; o < kWave; o <<= 1) {
            const unsigned long long xa = __shfl_up(va, o), xb = __shfl_up(vb, o);
            if (lane >= (uint32_t)o) {
                va += xa;
                vb += xb;
            }
        }
        if (lane == 63u) {
            wave_tot[0][wave] = va;
            wave_tot[1][wave] = vb;
        }
        __syncthreads();
        unsigned long long all_a = 0, all_b = 0;
        for (uint32_t w = 0; w < kWaitThreads / kWave; ++w) {
            if (w == wave) {
                va += base_a + all_a;
                vb += base_b + all_b;
            }
            all_a += wave_tot[0][w];
            all_b += wave_tot[1][w];
        }
        base_a += all_a;
        base_b += all_b;
        __syncthreads();  // wave_tot is rewritten by the next round
        if (live) {
            const uint32_t t = a.t0 + k * a.period;  // fits: the last sample is at most 0xFFFFFFFE
            uint32_t lo = 0, hi = J;                 // JobsCount: arrivals <= t (sorted)
            while (lo < hi) {
                const uint32_t mid = lo + (hi - lo) / 2u;
                if (rec[mid].w <= t) lo = mid + 1u;
                else hi = mid;
            }
            // two's complement throughout: the true value fits wherever Go's int64 does
            const long long total = (long long)((va + (unsigned long long)t * vb - sk) * 1000ull);
            mcs_wait_sample out;
            out.average_wait_time = lo ? __ddiv_rn((double)total, (double)(long long)lo) : 0.0;
            out.total_wait_ms = total;
            out.jobs_count = (long long)lo;
            row[k] = out;
        }
    }
}

}  // namespace

hipError_t launch_wait_rec(const WaitArgs& a, hipStream_t s) {
    if (a.n_clusters == 0) return hipSuccess;
    if (a.job_cnt)
        hipLaunchKernelGGL(wait_prep_kernel<true>, dim3(a.n_clusters), dim3(kWaitThreads), 0, s, a);
    else
        hipLaunchKernelGGL(wait_prep_kernel<false>, dim3(a.n_clusters), dim3(kWaitThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_wait_prep(const WaitArgs& a, hipStream_t s) {
    if (a.n_clusters == 0) return hipSuccess;
    hipError_t st = launch_wait_rec(a, s);
    if (st != hipSuccess) return st;
    if (a.job_cnt)
        hipLaunchKernelGGL(wait_skip_kernel<true>, dim3(a.n_clusters), dim3(kWaitThreads), 0, s, a);
    else
        hipLaunchKernelGGL(wait_skip_kernel<false>, dim3(a.n_clusters), dim3(kWaitThreads), 0, s, a);
    return hipGetLastError();
}

// the last step alone, over accumulators the caller filled (mcs_stream.hip): an online session's segments
hipError_t launch_wait_finish(const WaitArgs& a, hipStream_t s) {
    if (a.n_clusters == 0 || a.n_samples == 0) return hipSuccess;
    if (!a.job_cnt) return hipErrorInvalidValue;
    hipLaunchKernelGGL(wait_finish_kernel<true>, dim3(a.n_clusters), dim3(kWaitThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_wait_series(const WaitArgs& a, hipStream_t s) {
    if (a.n_clusters == 0 || a.n_samples == 0) return hipSuccess;
    hipError_t st = hipMemsetAsync(a.out, 0, (size_t)a.n_clusters * a.n_samples * sizeof(mcs_wait_sample), s);
    if (st != hipSuccess) return st;
    if (a.job_cnt)
        hipLaunchKernelGGL(wait_accum_kernel<true>, dim3(a.n_clusters), dim3(kWaitThreads), 0, s, a);
    else
        hipLaunchKernelGGL(wait_accum_kernel<false>, dim3(a.n_clusters), dim3(kWaitThreads), 0, s, a);
    st = hipGetLastError();
    if (st != hipSuccess) return st;
    if (a.job_cnt)
        hipLaunchKernelGGL(wait_finish_kernel<true>, dim3(a.n_clusters), dim3(kWaitThreads), 0, s, a);
    else
        hipLaunchKernelGGL(wait_finish_kernel<false>, dim3(a.n_clusters), dim3(kWaitThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace mcs
