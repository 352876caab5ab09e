// mcs_level1.hip — the Level1 list of a DELAY run over time (mcs_level1_series, mcs_read_level1,
// mcs_online_level1_series): what ProvideJobs (trader_server.go:69-94, over GetLevel1,
// scheduler.go:204-214) hands the trader after the Delay iteration at a second t, and the two
// contract sizes the trader takes from it (scheduler_client.go:126-289).
//
// wait_prep_kernel (mcs_wait.hip) leaves {h, m, s, a} per job: m_j is the iteration at which a head
// that still fails moves to Level1, s_j the start (0xFFFFFFFF: never placed, undecided, or past every
// sample second).  After the iteration at t
//   Level1(t) = { j : m_j <= t < s_j }   in stream order
// (a head placed at m_j itself has s_j = m_j and is never a member; the D6 skips change which entries
// are examined, not the list's order).  m_j is non-decreasing in j over all jobs, so the candidates at
// t are the prefix [0, hi(t)), hi by bisection on m; the row of Level1[0] is non-decreasing in t, and
// once the list is empty at t no job below hi(t) enters it again, so the scan's lower bound only
// moves up along the samples.
//
// Three kernels, 256 threads each:
//   level1_summary_kernel  per batch of kSeriesBatch jobs the largest s among the jobs that move to
//                          Level1 (s_j > m_j; 0 when none does): a batch whose summary is <= t has
//                          wholly left Level1 by t and is skipped without reading its rows.
//   level1_series_kernel   one workgroup per (cluster, tile of kLevel1Tile samples): per sample hi(t),
//                          the scan of the batches between the carried lower bound and hi, a
//                          reduction of len, the two uint32 sums, the longest duration and the first
//                          and last member rows, and the small-node time where len is a positive
//                          multiple of 20.
//   level1_list_kernel     one workgroup for one cluster and one second: the member rows, compacted
//                          in order (ballot prefix per wave, wave counts through LDS).
// The member test, hi(t) and the small-node time are in mcs_level1_dev.h, which the cursor's Level1
// kernel (mcs_stream.hip) shares.
// Integer arithmetic only; every loop is bounded by J or the sample count; no workgroup waits for
// another.  The SEG instantiations read an online session's segments (J = job_cnt[c], rows addressed
// by the segment start job_off[c]), as the wait kernels do.
#include "mcs_internal.h"
#include "mcs_level1_dev.h"

namespace mcs {

namespace {

constexpr int kL1Threads = 256;
constexpr int kL1Waves = kL1Threads / kWave;
constexpr uint32_t kNone = 0xFFFFFFFFu;
static_assert(kSeriesBatch == (uint32_t)kL1Threads, "one row per thread and batch");

template <bool SEG>
__device__ __forceinline__ uint32_t level1_rows(const Level1Args& a, uint32_t c) {
    if constexpr (SEG)
        return a.job_cnt[c];
    else
        return (uint32_t)(a.job_off[c + 1] - a.job_off[c]);
}

// cluster c's summaries (series_summ_size: over segments with slack the same index serves)
__device__ __forceinline__ uint32_t* level1_summ(const Level1Args& a, uint32_t c, uint64_t j0) {
    return a.summ + (size_t)(j0 / kSeriesBatch) + c;
}

template <bool SEG>
__global__ __launch_bounds__(kL1Threads) void level1_summary_kernel(Level1Args a) {
    const uint32_t c = blockIdx.x;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t j0 = a.job_off[c];
    const uint32_t J = level1_rows<SEG>(a, c);
    const uint4* __restrict__ rec = a.rec + (j0 - a.rec_off);
    uint32_t* __restrict__ summ = level1_summ(a, c, j0);
    const uint64_t nb = ((uint64_t)J + kSeriesBatch - 1u) / kSeriesBatch;
    for (uint64_t b = wave; b < nb; b += kL1Waves) {  // one wave per batch, four rows per lane
        uint32_t v = 0u;
#pragma unroll
        for (uint32_t u = 0; u < kSeriesBatch / kWave; ++u) {
            const uint64_t j = b * kSeriesBatch + u * kWave + lane;
            if (j < J) {
                const uint4 r = rec[j];
                if (r.z > r.y && r.z > v) v = r.z;
            }
        }
        for (int o = 32; o > 0; o >>= 1) {
            const uint32_t w = __shfl_xor(v, o);
            v = w > v ? w : v;
        }
        if (lane == 0u) summ[b] = v;
    }
}

template <bool SEG>
__global__ __launch_bounds__(kL1Threads) void level1_series_kernel(Level1Args a) {
    __shared__ uint32_t part[kL1Waves][6];
    __shared__ uint32_t small_s;
    const uint32_t c = blockIdx.x / a.n_tiles, tile = blockIdx.x - c * a.n_tiles;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint64_t j0 = a.job_off[c];
    const uint32_t J = level1_rows<SEG>(a, c);
    const uint4* __restrict__ rec = a.rec + (j0 - a.rec_off);
    const uint4* __restrict__ jobs = a.jobs + j0;
    const uint32_t* __restrict__ summ = level1_summ(a, c, j0);
    mcs_level1_sample* const row = a.out + (size_t)c * a.n_samples;
    const uint32_t k0 = tile * kLevel1Tile;
    const uint32_t k1 = a.n_samples - k0 < kLevel1Tile ? a.n_samples : k0 + kLevel1Tile;
    uint32_t lo = 0u, hi = 0u;  // carried along the tile: both only move up
    for (uint32_t k = k0; k < k1; ++k) {
        const uint32_t t = a.t0 + k * a.period;  // fits: the last sample is at most 0xFFFFFFFE
        hi = k == k0 ? level1_hi(rec, 0u, J, t) : level1_hi_next(rec, hi, J, t, lane);
        uint32_t len = 0u, sc = 0u, sm = 0u, dmax = 0u, first = kNone, last = 0u;
        if (lo < hi) {
            const uint32_t b1 = (hi - 1u) / kSeriesBatch;
            for (uint32_t b = lo / kSeriesBatch; b <= b1; ++b) {
                if (summ[b] <= t) continue;  // the batch has wholly left Level1
                const uint32_t j = b * kSeriesBatch + tid;
                if (j >= lo && j < hi && is_member(rec[j], t)) {
                    const uint4 q = jobs[j];  // {arrival, dur, cores, mem}
                    ++len;
                    sc += q.z;
                    sm += q.w;
                    dmax = q.y > dmax ? q.y : dmax;
                    first = j < first ? j : first;
                    last = j;  // rows rise along the loop
                }
            }
        }
        for (int o = 32; o > 0; o >>= 1) {
            len += __shfl_xor(len, o);
            sc += __shfl_xor(sc, o);
            sm += __shfl_xor(sm, o);
            const uint32_t xd = __shfl_xor(dmax, o), xf = __shfl_xor(first, o), xl = __shfl_xor(last, o);
            dmax = xd > dmax ? xd : dmax;
            first = xf < first ? xf : first;
            last = xl > last ? xl : last;
        }
        if (lane == 0u) {
            part[wave][0] = len;
            part[wave][1] = sc;
            part[wave][2] = sm;
            part[wave][3] = dmax;
            part[wave][4] = first;
            part[wave][5] = last;
        }
        __syncthreads();
        len = sc = sm = dmax = last = 0u;
        first = kNone;
#pragma unroll
        for (int w = 0; w < kL1Waves; ++w) {
            len += part[w][0];
            sc += part[w][1];
            sm += part[w][2];
            dmax = part[w][3] > dmax ? part[w][3] : dmax;
            first = part[w][4] < first ? part[w][4] : first;
            last = part[w][5] > last ? part[w][5] : last;
        }
        const bool walk = len != 0u && len % 20u == 0u;  // uniform over the workgroup
        if (walk && wave == 0u) {
            const uint32_t st = level1_small_time(rec, jobs, summ, first, last, t, lane);
            if (lane == 0u) small_s = st;
        }
        __syncthreads();  // part is rewritten by the next sample (small_s by thread 0 itself)
        if (tid == 0u) {
            mcs_level1_sample s;
            s.len = len;
            s.cores = sc;
            s.mem = sm;
            s.fast_time_s = dmax;
            s.small_time_s = walk ? small_s : 0u;
            s.head = first;
            row[k] = s;
        }
        lo = len ? first : hi;  // no row below the head, and none below hi of an empty list, comes back
    }
}

__global__ __launch_bounds__(kL1Threads) void level1_list_kernel(Level1Args a) {
    __shared__ uint32_t wcnt[kL1Waves];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint64_t j0 = a.job_off[0];
    const uint32_t J = level1_rows<false>(a, 0u);
    const uint4* __restrict__ rec = a.rec + (j0 - a.rec_off);
    const uint32_t t = a.t0;
    const uint32_t hi = level1_hi(rec, 0u, J, t);
    uint32_t base = 0u;  // members before this round
    for (uint64_t b0 = 0; b0 < hi; b0 += kL1Threads) {  // 64-bit: b0 + 256 may pass 2^32
        const uint64_t j = b0 + tid;
        const bool mem = j < hi && is_member(rec[j], t);
        const unsigned long long mask = __ballot(mem);
        if (lane == 0u) wcnt[wave] = (uint32_t)__popcll(mask);
        __syncthreads();
        uint32_t before = base, all = 0u;
#pragma unroll
        for (uint32_t w = 0; w < (uint32_t)kL1Waves; ++w) {
            if (w < wave) before += wcnt[w];
            all += wcnt[w];
        }
        const uint32_t at = before + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
        if (mem && at < a.cap) a.rows[at] = (uint32_t)j;
        base += all;
        __syncthreads();  // wcnt is rewritten by the next round
    }
    if (tid == 0u) *a.n_out = base;
}

}  // namespace

hipError_t launch_level1_summary(const Level1Args& a, hipStream_t s) {
    if (a.n_clusters == 0) return hipSuccess;
    if (a.job_cnt)
        hipLaunchKernelGGL(level1_summary_kernel<true>, dim3(a.n_clusters), dim3(kL1Threads), 0, s, a);
    else
        hipLaunchKernelGGL(level1_summary_kernel<false>, dim3(a.n_clusters), dim3(kL1Threads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_level1_series(const Level1Args& a, hipStream_t s) {
    if (a.n_clusters == 0 || a.n_samples == 0) return hipSuccess;
    const uint64_t grid = (uint64_t)a.n_clusters * a.n_tiles;
    if (a.n_tiles != (a.n_samples + kLevel1Tile - 1u) / kLevel1Tile || grid > 0x7FFFFFFFull) return hipErrorInvalidValue;
    if (a.job_cnt)
        hipLaunchKernelGGL(level1_series_kernel<true>, dim3((uint32_t)grid), dim3(kL1Threads), 0, s, a);
    else
        hipLaunchKernelGGL(level1_series_kernel<false>, dim3((uint32_t)grid), dim3(kL1Threads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_level1_list(const Level1Args& a, hipStream_t s) {
    hipLaunchKernelGGL(level1_list_kernel, dim3(1), dim3(kL1Threads), 0, s, a);
    return hipGetLastError();
}

}  // namespace mcs
