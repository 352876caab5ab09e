// mcs_stream.hip — the start-stream cursor of an online session (mcs_stream_next).
//
// mcs_online_state_series rebuilds its scratch from the whole history at every call.  A stream keeps,
// per batch of kSeriesBatch rows, what no later horizon or append can change, and retires the batches
// no later sample can see:
//   final    a full batch whose rows are all decided (placed, start known).  Its summary
//            {arrival_min, end_max}, its wait records {h, m, s, a} and its sum of s - a are then exact
//            and stay: h_j <= s_j lies below the horizon, so h_j and with it m_j are exact (§14).
//   retired  a final batch with end_max < F, F the stream's next sample second.  At every t >= F none
//            of its jobs is queued or running, so series_kernel's own summary test passes it over
//            (end_max <= t_first), and both wait events of each job lie below F: it adds the constant
//            sum of s - a to A(t), 0 to B(t), and its Level1 placements fall on no sample (skip is
//            pointwise).  The constant is carried per cluster; no per-job loop reads the batch again.
// Retirement is per batch, not a prefix: a Level1 job that starves keeps its own batch live and no
// other.  The d carry of the clamp scan does advance as a prefix: d is strictly increasing and d_j is
// exact as soon as it lies below the horizon, whatever s_j is.
//
// Three kernels, one 256-thread workgroup per cluster each, one thread per row of a batch:
//   stream_prep_kernel    every batch that is not final: the summary, the records (rows from the d
//                         carry on: the clamp scan of wait_prep_kernel; rows before it: s alone), the
//                         final flag and the sum.
//   stream_accum_kernel   wait_accum_kernel over the batches that are not retired, the entry a Level1
//                         placement steps over searched when that placement falls on a sample
//                         (wait_skip_of), plus the carried constant on sample 0.  wait_finish_kernel
//                         and series_kernel then run as they are, over the kept records and summaries.
//   stream_retire_kernel  one thread per batch: retire against the new frontier, and count the rows
//                         the call loaded from the flags and the summaries (series_kernel reads the
//                         batches that its tiles hit: arrival_min <= t_last and end_max > t_first).
// stream_move_kernel carries the kept arrays over a segment relayout.
// A stream opened with Level1 (mcs_stream_open_level1) adds two kernels, stated where they stand below:
//   stream_level1_summ_kernel  after the prep kernel: the Level1 summary of every batch prep loaded.
//   stream_level1_kernel       the call's Level1 samples, one wave per cluster, from the carried bounds.
// A trading session's stream (mcs_trade_stream_next) runs the TRADE instantiations of the prep and the
// retire kernel, dt_series_kernel in place of series_kernel and, before them, dt_stream_foreign_kernel
// (mcs_state.hip): the two differences are stated at the templates.  The plain instantiations are the
// code they were.
// Every loop is bounded by a row, batch or sample count; no workgroup waits for another.
#include <type_traits>

#include "mcs_internal.h"
#include "mcs_level1_dev.h"
#include "mcs_wait_dev.h"
#include "mcs_wave.h"

namespace mcs {

namespace {

constexpr int kStreamThreads = 256;
static_assert(kStreamThreads == (int)kSeriesBatch, "one thread per row of a batch");
constexpr uint32_t kNone = 0xFFFFFFFFu;
template <bool TRADE>
using StreamArgsOf = std::conditional_t<TRADE, TradeStreamArgs, StreamArgs>;

// The batches base + i, i < 256, below nb whose flags hold none of `mask`, in stream order: list[] (LDS,
// 256 entries) receives their i, the count is returned.  The caller synchronises before the next call.
__device__ __forceinline__ uint32_t pick_batches(const uint32_t* __restrict__ flags, uint64_t base, uint64_t nb,
                                                 uint32_t mask, uint32_t* list, uint32_t* wcnt) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint64_t b = base + tid;
    const bool pred = b < nb && (flags[b] & mask) == 0u;
    const uint64_t bm = __ballot(pred);
    if (lane == 0u) wcnt[wave] = (uint32_t)__popcll(bm);
    __syncthreads();
    uint32_t before = 0, total = 0;
    for (uint32_t w = 0; w < kStreamThreads / kWave; ++w) {
        if (w < wave) before += wcnt[w];
        total += wcnt[w];
    }
    if (pred) list[before + (uint32_t)__popcll(bm & ((1ull << lane) - 1ull))] = tid;
    __syncthreads();
    return total;
}

// TRADE: a trading session's rows.  An own job runs on a physical node or on a virtual one (k >= N), so
// the summary's end is the TRADE summaries' rule (launch_dt_series_summary, `apply` in dt_series_kernel):
// the finish of every job with k >= 0.  With the plain test such a job would drop out of end_max and its
// batch would retire while the job still holds its row.
template <bool TRADE>
__global__ __launch_bounds__(kStreamThreads) void stream_prep_kernel(StreamArgs a) {
    __shared__ Clamp wave_tot[kStreamThreads / kWave];
    __shared__ long long carry_s, pd_s;
    __shared__ uint32_t list[kStreamThreads], wcnt[kStreamThreads / kWave];
    __shared__ uint32_t red_min[kStreamThreads / kWave], red_max[kStreamThreads / kWave];
    __shared__ unsigned long long red_sum[kStreamThreads / kWave];
    const uint32_t c = blockIdx.x;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t N = a.s.node_off[c + 1] - a.s.node_off[c];
    const uint64_t j0 = a.s.job_off[c];
    const uint64_t J = a.s.job_cnt[c];
    const uint64_t nb = (J + kSeriesBatch - 1) / kSeriesBatch;
    const uint64_t bi = j0 / kSeriesBatch + c;
    const int32_t* __restrict__ node = a.s.out_node + j0;
    const uint32_t* __restrict__ start = a.s.out_start + j0;
    const uint32_t* __restrict__ finish = a.s.out_finish + j0;
    const uint4* __restrict__ jobs = a.s.jobs + j0;
    uint32_t* __restrict__ flags = a.flags + bi;
    uint2* __restrict__ summ = a.summ + bi;
    unsigned long long* __restrict__ bsum = a.bsum + bi;
    uint4* __restrict__ rec = a.rec ? a.rec + j0 : nullptr;
    const bool wait = a.rec != nullptr;
    const long long W = (long long)a.max_wait, hor = (long long)a.hor;
    const StreamCluster st = a.cl[c];
    const uint64_t p0 = st.p;  // rows below have their final h and m
    uint64_t p = p0;           // grows while every row so far has d below the horizon
    bool adv = true;
    long long carry = st.d_carry;
    if (tid == 0) pd_s = st.d_carry;
    __syncthreads();
    for (uint64_t base = st.first_live; base < nb; base += kStreamThreads) {
        const uint32_t n_pick = pick_batches(flags, base, nb, kStreamFinal, list, wcnt);
        for (uint32_t x = 0; x < n_pick; ++x) {
            const uint64_t b = base + list[x];
            const uint64_t i = b * kSeriesBatch + tid;
            const bool live = i < J;
            uint32_t arr = 0, s32 = kNone, end = 0;
            bool placed_w = false, decided = false;
            if (live) {
                arr = jobs[i].x;
                const int32_t k = node[i];
                s32 = start[i];
                const uint32_t f = finish[i];
                placed_w = k >= 0 && s32 != kNone;                   // wait_prep_kernel's test
                bool placed_s;
                if constexpr (TRADE)
                    placed_s = k >= 0;                               // the TRADE summaries' (a DELAY run borrows nothing)
                else
                    placed_s = k >= 0 && (uint32_t)k < N;            // series_summary_kernel's
                end = placed_s ? f : kNone;                          // unplaced: queued for good
                decided = placed_w && placed_s && f != kNone;
            }
            uint32_t amin = live ? arr : kNone, emax = end;
            unsigned long long sum = placed_w ? (unsigned long long)s32 - (unsigned long long)arr : 0ull;
            for (int o = 32; o > 0; o >>= 1) {
                const uint32_t xa = (uint32_t)__shfl_xor((int)amin, o), xe = (uint32_t)__shfl_xor((int)emax, o);
                amin = xa < amin ? xa : amin;
                emax = xe > emax ? xe : emax;
                sum += __shfl_xor(sum, o);
            }
            if (lane == 0u) {
                red_min[wave] = amin;
                red_max[wave] = emax;
                red_sum[wave] = sum;
            }
            const uint32_t n_dec = (uint32_t)__syncthreads_count(decided);
            if (wait) {
                const long long s = placed_w ? (long long)s32 : kWaitInf;
                const long long la = (long long)arr;
                if ((b + 1) * kSeriesBatch > p0) {  // rows from the d carry on: the clamp scan
                    const bool scan = live && i >= p0;
                    Clamp e{-kWaitInf, kWaitInf, 0u};  // the identity
                    if (scan) {
                        e.hi = s;
                        e.lo = la + W < s ? la + W : s;
                        e.c = 1u;
                    }
                    long long dprev;
                    const long long d = clamp_scan_round(e, carry, wave_tot, dprev);
                    if (scan) {
                        const long long h = la > dprev + 1 ? la : dprev + 1;
                        const long long m = h > la + W ? h : la + W;
                        rec[i] = make_uint4(sat32(h), sat32(m), sat32(s), arr);
                    } else if (live) {
                        reinterpret_cast<uint32_t*>(rec + i)[2] = sat32(s);
                    }
                    if (tid == kStreamThreads - 1) carry_s = d;
                    const uint32_t n_ok = (uint32_t)__syncthreads_count(scan && d < hor);
                    carry = carry_s;
                    if (adv) {  // d ascends: the rows with d below the horizon are a prefix
                        const uint64_t first = b * kSeriesBatch > p0 ? b * kSeriesBatch : p0;
                        if (n_ok && i == first + n_ok - 1u) pd_s = d;
                        p = first + n_ok;
                        adv = p == (b + 1) * kSeriesBatch;
                    }
                } else if (live) {  // h and m are final: s alone may have been decided since
                    reinterpret_cast<uint32_t*>(rec + i)[2] = sat32(s);
                }
            }
            // final: full, all decided, and (with records) every d below the horizon, so that the
            // batches from the d carry on are never final and the scan passes through all of them
            const bool fin = n_dec == kSeriesBatch && (!wait || (b + 1) * kSeriesBatch <= p);
            if (tid == 0) {
                sum = 0ull;
                for (uint32_t w = 0; w < kStreamThreads / kWave; ++w) {
                    amin = red_min[w] < amin ? red_min[w] : amin;
                    emax = red_max[w] > emax ? red_max[w] : emax;
                    sum += red_sum[w];
                }
                summ[b] = make_uint2(amin, emax);
                if (fin) bsum[b] = sum;
                flags[b] = (fin ? kStreamFinal : 0u) | kStreamLoaded;
            }
            __syncthreads();  // the reduction words, wave_tot and carry_s are rewritten by the next batch
        }
        __syncthreads();  // list is rewritten by the next round
    }
    if (wait && tid == 0) {
        a.cl[c].p = (uint32_t)p;
        a.cl[c].d_carry = pd_s;
    }
}

__global__ __launch_bounds__(kStreamThreads) void stream_accum_kernel(StreamArgs a) {
    __shared__ uint32_t list[kStreamThreads], wcnt[kStreamThreads / kWave];
    const uint32_t c = blockIdx.x;
    const uint32_t tid = threadIdx.x;
    const uint64_t j0 = a.s.job_off[c];
    const uint32_t J = a.s.job_cnt[c];
    const uint64_t nb = ((uint64_t)J + kSeriesBatch - 1) / kSeriesBatch;
    const uint32_t* __restrict__ flags = a.flags + (j0 / kSeriesBatch + c);
    const uint4* __restrict__ rec = a.rec + j0;
    const StreamCluster st = a.cl[c];
    WaitAcc acc;
    acc.n = a.n_samples;
    acc.period = a.period;
    acc.t_first = a.t0;
    acc.row = a.wout + (size_t)c * a.n_samples;
    for (uint64_t base = st.first_live; base < nb; base += kStreamThreads) {
        const uint32_t n_pick = pick_batches(flags, base, nb, kStreamRetired, list, wcnt);
        for (uint32_t x = 0; x < n_pick; ++x) {
            const uint64_t i = (base + list[x]) * kSeriesBatch + tid;
            if (i < J) {
                const uint32_t P = (uint32_t)i;
                acc.job(rec[P], [&]() { return wait_skip_of(rec, P, J); });
            }
        }
        __syncthreads();  // list is rewritten by the next round
    }
    if (tid == 0) acc.pre_a += st.a_base;  // the retired batches: s - a for good, on sample 0
    acc.flush();
}

// TRADE: dt_series_kernel cuts the call into tiles of dt_series_tile(N + nv[c]) samples, nv[c] the
// cluster's virtual rows in this call (it grows when the cluster receives a virtual node between calls).
template <bool TRADE>
__global__ __launch_bounds__(kStreamThreads) void stream_retire_kernel(StreamArgsOf<TRADE> a) {
    __shared__ unsigned long long s_scan, s_ret, s_ab;
    __shared__ uint32_t s_first;
    const uint32_t c = blockIdx.x;
    const uint32_t tid = threadIdx.x;
    const uint32_t N = a.s.node_off[c + 1] - a.s.node_off[c];
    const uint64_t j0 = a.s.job_off[c];
    const uint64_t J = a.s.job_cnt[c];
    const uint64_t nb = (J + kSeriesBatch - 1) / kSeriesBatch;
    const uint64_t bi = j0 / kSeriesBatch + c;
    uint32_t* __restrict__ flags = a.flags + bi;
    const uint2* __restrict__ summ = a.summ + bi;
    const unsigned long long* __restrict__ bsum = a.bsum + bi;
    const bool wait = a.rec != nullptr;
    uint32_t TS;
    if constexpr (TRADE)
        TS = dt_series_tile(N + a.nv[c]);
    else
        TS = series_tile(N);
    const StreamCluster st = a.cl[c];
    if (tid == 0) {
        s_scan = s_ret = s_ab = 0ull;
        s_first = kNone;
    }
    __syncthreads();
    for (uint64_t b = (uint64_t)st.first_live + tid; b < nb; b += kStreamThreads) {
        uint32_t fl = flags[b];
        if ((fl & kStreamRetired) == 0u) {
            const uint2 sm = summ[b];
            const unsigned long long rows = J - b * kSeriesBatch < kSeriesBatch ? J - b * kSeriesBatch : kSeriesBatch;
            // loaded by stream_prep_kernel, by stream_accum_kernel (its records), or by a tile of series_kernel
            bool loaded = (fl & kStreamLoaded) != 0u || wait;
            for (uint32_t c0 = 0; !loaded && c0 < a.n_samples; c0 += a.chunk) {
                const uint32_t nk = a.n_samples - c0 < a.chunk ? a.n_samples - c0 : a.chunk;
                for (uint32_t k0 = 0; !loaded && k0 < nk; k0 += TS) {
                    const uint32_t tsa = nk - k0 < TS ? nk - k0 : TS;
                    const uint32_t t_first = a.t0 + (c0 + k0) * a.period, t_last = t_first + (tsa - 1u) * a.period;
                    loaded = sm.x <= t_last && sm.y > t_first;
                }
            }
            if (loaded) atomicAdd(&s_scan, rows);
            if ((fl & kStreamFinal) != 0u && sm.y < a.frontier) {
                fl |= kStreamRetired;
                atomicAdd(&s_ret, rows);
                atomicAdd(&s_ab, bsum[b]);
            }
            flags[b] = fl & ~kStreamLoaded;
        }
        if ((fl & kStreamRetired) == 0u) atomicMin(&s_first, (uint32_t)b);
    }
    __syncthreads();
    if (tid == 0) {
        a.cl[c].a_base = st.a_base + s_ab;
        a.cl[c].first_live = s_first < nb ? s_first : (uint32_t)nb;
        if (s_scan) atomicAdd(a.tot, s_scan);
        if (s_ret) atomicAdd(a.tot + 1, s_ret);
    }
}

__global__ __launch_bounds__(kStreamThreads) void stream_move_kernel(StreamMoveArgs a) {
    const uint32_t c = blockIdx.y;
    const uint64_t o0 = a.old_off[c], n0 = a.new_off[c];
    const uint64_t J = a.job_cnt[c];
    const uint64_t nb = (J + kSeriesBatch - 1) / kSeriesBatch;
    const uint64_t bo = o0 / kSeriesBatch + c, bn = n0 / kSeriesBatch + c;
    const uint64_t step = (uint64_t)gridDim.x * kStreamThreads;
    for (uint64_t b = (uint64_t)blockIdx.x * kStreamThreads + threadIdx.x; b < nb; b += step) {
        a.flags_n[bn + b] = a.flags_o[bo + b];
        a.summ_n[bn + b] = a.summ_o[bo + b];
        a.bsum_n[bn + b] = a.bsum_o[bo + b];
    }
    if (a.l1s_n)
        for (uint64_t b = (uint64_t)blockIdx.x * kStreamThreads + threadIdx.x; b < nb; b += step)
            a.l1s_n[bn + b] = a.l1s_o[bo + b];
    if (a.rec_n)
        for (uint64_t i = (uint64_t)blockIdx.x * kStreamThreads + threadIdx.x; i < J; i += step)
            a.rec_n[n0 + i] = a.rec_o[o0 + i];
}

// ---- Level1 samples on the cursor (mcs_stream_next_level1) --------------------------
//
// level1_summary_kernel's word for the batches stream_prep_kernel loaded in this call: one wave per
// batch, four rows per lane.  A batch that was final before the call is not loaded and keeps its word
// (its rows are decided: no s changes); one that became final in this call gets its last word here.
__global__ __launch_bounds__(kStreamThreads) void stream_level1_summ_kernel(StreamLevel1Args a) {
    const uint32_t c = blockIdx.x;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t j0 = a.job_off[c];
    const uint64_t J = a.job_cnt[c];
    const uint64_t nb = (J + kSeriesBatch - 1) / kSeriesBatch;
    const uint64_t bi = j0 / kSeriesBatch + c;
    const uint32_t* __restrict__ flags = a.flags + bi;
    const uint4* __restrict__ rec = a.rec + j0;
    uint32_t* __restrict__ l1s = a.l1s + bi;
    for (uint64_t b = (uint64_t)a.cl[c].first_live + wave; b < nb; b += kStreamThreads / kWave) {
        if ((flags[b] & kStreamLoaded) == 0u) continue;  // uniform over the wave
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
        if (lane == 0u) l1s[b] = v;
    }
}

// level1_series_kernel's samples with one wave per cluster, four clusters per workgroup: a call has
// few samples and many clusters, so the parallelism is over clusters, and a sample costs no barrier
// and no LDS.  The wave walks the chunk's samples in order from the carried pair {lo, hi} (both only
// move up, across calls as along a tile: DESIGN.md §14), scans the batches between them whose kept
// summary exceeds t, four rows per lane, and reduces with shuffles.  Batches below first_live are
// passed over unread: a retired batch has every start <= finish < F <= t, so it holds no member and
// its summary lies below every later sample.  Waves of a workgroup never wait for each other.
constexpr uint32_t kStreamL1Clusters = kStreamThreads / kWave;
__global__ __launch_bounds__(kStreamThreads) void stream_level1_kernel(StreamLevel1Args a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t c = blockIdx.x * kStreamL1Clusters + (threadIdx.x >> 6);
    if (c >= a.n_clusters) return;  // the whole wave
    const uint64_t j0 = a.job_off[c];
    const uint32_t J = a.job_cnt[c];
    const uint4* __restrict__ rec = a.rec + j0;
    const uint4* __restrict__ jobs = a.jobs + j0;
    const uint32_t* __restrict__ summ = a.l1s + (j0 / kSeriesBatch + c);
    const uint32_t first_live = a.cl[c].first_live;
    mcs_level1_sample* const row = a.out + (size_t)c * a.n_samples;
    const uint2 cr = a.carry[c];
    uint32_t lo = a.fresh ? 0u : cr.x, hi = a.fresh ? 0u : cr.y;
    unsigned long long rows = 0ull;  // uniform over the wave
    for (uint32_t k = 0; k < a.n_samples; ++k) {
        const uint32_t t = a.t0 + k * a.period;  // fits: the last sample is at most 0xFFFFFFFE
        hi = a.fresh && k == 0u ? level1_hi(rec, 0u, J, t) : level1_hi_next(rec, hi, J, t, lane);
        uint32_t len = 0u, sc = 0u, sm = 0u, dmax = 0u, first = kNone, last = 0u;
        if (lo < hi) {
            const uint32_t b1 = (hi - 1u) / kSeriesBatch;
            uint32_t b = lo / kSeriesBatch;
            if (b < first_live) b = first_live;
            for (; b <= b1; ++b) {
                if (summ[b] <= t) continue;  // the batch has wholly left Level1
                const uint64_t r0 = (uint64_t)b * kSeriesBatch;
                const uint64_t x0 = r0 > lo ? r0 : lo, x1 = r0 + kSeriesBatch < hi ? r0 + kSeriesBatch : hi;
                rows += x1 - x0;  // (x0 < x1: lo's batch at the least holds lo, every other starts below hi)
#pragma unroll
                for (uint32_t u = 0; u < kSeriesBatch / kWave; ++u) {
                    const uint64_t j = r0 + u * kWave + lane;
                    if (j >= x0 && j < x1 && is_member(rec[j], t)) {
                        const uint4 q = jobs[j];  // {arrival, dur, cores, mem}
                        ++len;
                        sc += q.z;
                        sm += q.w;
                        dmax = q.y > dmax ? q.y : dmax;
                        first = (uint32_t)j < first ? (uint32_t)j : first;
                        last = (uint32_t)j;  // rows rise along both loops
                    }
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
        uint32_t small = 0u;
        if (len != 0u && len % 20u == 0u) small = level1_small_time(rec, jobs, summ, first, last, t, lane);
        if (lane == 0u) {
            mcs_level1_sample s;
            s.len = len;
            s.cores = sc;
            s.mem = sm;
            s.fast_time_s = dmax;
            s.small_time_s = small;
            s.head = first;
            row[k] = s;
        }
        lo = len ? first : hi;  // no row below the head, and none below hi of an empty list, comes back
    }
    if (lane == 0u) {
        a.carry[c] = make_uint2(lo, hi);
        if (rows) atomicAdd(a.rows, rows);
    }
}

}  // namespace

hipError_t launch_stream_prep(const StreamArgs& a, hipStream_t s) {
    if (a.s.n_clusters == 0) return hipSuccess;
    if (!a.s.job_cnt) return hipErrorInvalidValue;  // a stream reads an online session's segments
    hipLaunchKernelGGL(stream_prep_kernel<false>, dim3(a.s.n_clusters), dim3(kStreamThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_trade_stream_prep(const StreamArgs& a, hipStream_t s) {
    if (a.s.n_clusters == 0) return hipSuccess;
    if (!a.s.job_cnt) return hipErrorInvalidValue;
    hipLaunchKernelGGL(stream_prep_kernel<true>, dim3(a.s.n_clusters), dim3(kStreamThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_stream_accum(const StreamArgs& a, hipStream_t s) {
    if (a.s.n_clusters == 0 || a.n_samples == 0) return hipSuccess;
    if (!a.s.job_cnt || !a.rec || !a.wout) return hipErrorInvalidValue;
    hipLaunchKernelGGL(stream_accum_kernel, dim3(a.s.n_clusters), dim3(kStreamThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_stream_retire(const StreamArgs& a, hipStream_t s) {
    if (a.s.n_clusters == 0) return hipSuccess;
    if (!a.s.job_cnt || a.chunk == 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(stream_retire_kernel<false>, dim3(a.s.n_clusters), dim3(kStreamThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_trade_stream_retire(const TradeStreamArgs& a, hipStream_t s) {
    if (a.s.n_clusters == 0) return hipSuccess;
    if (!a.s.job_cnt || a.chunk == 0 || !a.nv) return hipErrorInvalidValue;
    hipLaunchKernelGGL(stream_retire_kernel<true>, dim3(a.s.n_clusters), dim3(kStreamThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_stream_move(const StreamMoveArgs& a, hipStream_t s) {
    if (a.n_clusters == 0) return hipSuccess;
    hipLaunchKernelGGL(stream_move_kernel, dim3(8, a.n_clusters), dim3(kStreamThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_stream_level1_summ(const StreamLevel1Args& a, hipStream_t s) {
    if (a.n_clusters == 0) return hipSuccess;
    if (!a.job_cnt || !a.rec || !a.l1s || !a.flags || !a.cl) return hipErrorInvalidValue;
    hipLaunchKernelGGL(stream_level1_summ_kernel, dim3(a.n_clusters), dim3(kStreamThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_stream_level1(const StreamLevel1Args& a, hipStream_t s) {
    if (a.n_clusters == 0 || a.n_samples == 0) return hipSuccess;
    if (!a.job_cnt || !a.rec || !a.l1s || !a.cl || !a.carry || !a.out || !a.rows) return hipErrorInvalidValue;
    const uint32_t grid = (a.n_clusters + kStreamL1Clusters - 1u) / kStreamL1Clusters;
    hipLaunchKernelGGL(stream_level1_kernel, dim3(grid), dim3(kStreamThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace mcs
