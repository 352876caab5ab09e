// mcs_state.hip — the ClusterState telemetry record as a batched reduction.
//
// state_kernel rebuilds, for every cluster of the last FIFO/DELAY run and one simulated second t,
// the record the scheduler's Start stream sends (pkg/scheduler/trader_server.go:24-47):
//   cores/memory utilization = GetResourceUtilization (cluster.go:46-63) over the counters after
//   second t: sum_i (float32(Cores_i) - float32(CoresAvailable_i)) in node order, / float32(total);
//   totals = SetTotalResources (cluster.go:26-40), uint32 sums of the physical nodes.
// A job holds its node at t iff it was placed with start <= t < finish (releases precede decisions,
// D3; a zero-duration job never holds it).
//
// Layout: one 256-thread workgroup (4 waves) per cluster.  The results SoA (node, start, finish)
// is scanned with coalesced 4 B loads; only the jobs running at t load their record's cores and
// memory.  Per-node usage accumulates in LDS with u32 atomics; the float32 sum is serial in node
// order (lane 0), as Go's loop is.  HBM-bound: 12 B per job scanned plus 8 B per running job.
#include "mcs_internal.h"
#include "mcs_wave.h"

namespace mcs {

namespace {

constexpr int kStateThreads = 256;

__global__ __launch_bounds__(kStateThreads) void state_kernel(StateArgs a) {
    extern __shared__ uint32_t used[];  // [2 * max_n]: cores then memory per node
    const uint32_t c = blockIdx.x;
    const uint32_t tid = threadIdx.x;
    const uint32_t n0 = a.node_off[c], N = a.node_off[c + 1] - n0;
    for (uint32_t i = tid; i < 2u * N; i += kStateThreads) used[i] = 0u;
    __syncthreads();

    const uint64_t j0 = a.job_off[c];
    const uint32_t J = (uint32_t)(a.job_off[c + 1] - j0);
    const int32_t* __restrict__ node = a.out_node + j0;
    const uint32_t* __restrict__ start = a.out_start + j0;
    const uint32_t* __restrict__ finish = a.out_finish + j0;
    const uint4* __restrict__ jobs = a.jobs + j0;
    const uint32_t t = a.t;
    uint32_t nrun = 0;
#pragma unroll 4
    for (uint32_t i = tid; i < J; i += kStateThreads) {
        const int32_t k = __builtin_nontemporal_load(node + i);
        const uint32_t s = __builtin_nontemporal_load(start + i);
        const uint32_t f = __builtin_nontemporal_load(finish + i);
        if (k >= 0 && (uint32_t)k < N && s <= t && t < f) {
            const uint2 cm = *reinterpret_cast<const uint2*>(&jobs[i].z);
            atomicAdd(&used[k], cm.x);
            atomicAdd(&used[N + k], cm.y);
            ++nrun;
        }
    }
    // running-job count: wave sums, then one LDS add per wave
    for (int o = 32; o > 0; o >>= 1) nrun += (uint32_t)__shfl_xor((int)nrun, o);
    __shared__ uint32_t run_total;
    if (tid == 0) run_total = 0u;
    __syncthreads();
    if ((tid & 63u) == 0u) atomicAdd(&run_total, nrun);
    __syncthreads();

    if (tid == 0) {
        float cu = 0.0f, mu = 0.0f;
        uint32_t tc = 0, tm = 0;
        for (uint32_t i = 0; i < N; ++i) {
            const uint2 cap = a.cap[n0 + i];
            const uint2 fr0 = a.free0[n0 + i];
            // live counters (Go uint64; no trading here, so they never wrap)
            const uint32_t fc = fr0.x - used[i], fm = fr0.y - used[N + i];
            cu = __fadd_rn(cu, __fsub_rn((float)cap.x, (float)fc));
            mu = __fadd_rn(mu, __fsub_rn((float)cap.y, (float)fm));
            tc += cap.x;
            tm += cap.y;
        }
        mcs_cluster_state st;
        st.cores_utilization = __fdiv_rn(cu, (float)tc);
        st.memory_utilization = __fdiv_rn(mu, (float)tm);
        st.total_cpu = tc;
        st.total_memory = tm;
        st.running = run_total;
        st.t_s = t;
        a.out[c] = st;
    }
}

// ---- the time series: every sample t_k = t0 + k * period of every cluster in one launch --------
//
// One 256-thread workgroup per cluster walks the samples in tiles of TS = series_tile(N)
// consecutive samples.  LDS holds 2 N + 2 kSeriesRep + 2 rows of TS u32: per node the cores and the
// memory in use, kSeriesRep copies each of the running and the queued counters, and two result rows.
// Per tile:
//   1. the jobs that can touch the tile add their value at the first sample of their range and
//      subtract it behind the last (u32 atomics; wrap-around is exact, the true values fit);
//   2. one thread per row runs the prefix sum along the samples and, for a node row, leaves the
//      float32 term float(Cores) - float(CoresAvailable) of GetResourceUtilization in place;
//   3. one lane per (sample, resource) adds its column's terms serially in node order and divides
//      by the total — the one-lane loop of state_kernel, 2 TS lanes wide;
//   4. the samples leave with coalesced 16 B stores.
// A job is read only for the tiles its [arrival, finish) window meets: series_summary_kernel
// writes {arrival_min, end_max} per batch of kSeriesBatch jobs, and a tile tests the summaries
// (256 per round, one per thread) from a cursor that skips the leading batches that ended before
// the tile up to the first batch that arrives after it (arrivals are sorted).
constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint32_t kGroup = 8;  // hit batches whose records a thread loads before it uses the first

__global__ __launch_bounds__(kStateThreads) void series_summary_kernel(SeriesArgs a) {
    const uint32_t c = blockIdx.x;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t N = a.s.node_off[c + 1] - a.s.node_off[c];
    const uint64_t j0 = a.s.job_off[c];
    const uint64_t J = a.s.job_off[c + 1] - j0;
    const uint64_t nb = (J + kSeriesBatch - 1) / kSeriesBatch;
    const int32_t* __restrict__ node = a.s.out_node + j0;
    const uint32_t* __restrict__ finish = a.s.out_finish + j0;
    const uint4* __restrict__ jobs = a.s.jobs + j0;
    uint2* __restrict__ summ = a.summ + (j0 / kSeriesBatch + c);
    for (uint64_t b = wave; b < nb; b += kStateThreads / kWave) {
        uint32_t amin = kNone, emax = 0u;
#pragma unroll
        for (uint32_t u = 0; u < kSeriesBatch / kWave; ++u) {
            const uint64_t i = b * kSeriesBatch + u * kWave + lane;
            if (i < J) {
                const uint32_t arr = jobs[i].x;
                const int32_t k = node[i];
                const uint32_t end = (k >= 0 && (uint32_t)k < N) ? finish[i] : kNone;  // unplaced: queued for good
                amin = arr < amin ? arr : amin;
                emax = end > emax ? end : emax;
            }
        }
        for (int o = 32; o > 0; o >>= 1) {
            const uint32_t x = (uint32_t)__shfl_xor((int)amin, o), y = (uint32_t)__shfl_xor((int)emax, o);
            amin = x < amin ? x : amin;
            emax = y > emax ? y : emax;
        }
        if (lane == 0) summ[b] = make_uint2(amin, emax);
    }
}

// +v on the samples [lo, hi) of a tile's row of `tsa` samples, as a difference
__device__ __forceinline__ void range_add(uint32_t* row, uint32_t lo, uint32_t hi, uint32_t tsa, uint32_t v) {
    if (lo < hi) {
        atomicAdd(&row[lo], v);
        if (hi < tsa) atomicSub(&row[hi], v);
    }
}

__global__ __launch_bounds__(kStateThreads) void series_kernel(SeriesArgs a) {
    extern __shared__ uint32_t d[];   // [2 N + 2 kSeriesRep + 2][TS]
    __shared__ uint64_t masks[3][4];  // hit / dead / past ballots of a summary round, per wave
    __shared__ uint32_t hits[kStateThreads];  // the round's hit batches, in stream order
    __shared__ uint32_t tot[2];
    const uint32_t c = blockIdx.x;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t n0 = a.s.node_off[c], N = a.s.node_off[c + 1] - n0;
    const uint64_t j0 = a.s.job_off[c];
    const uint64_t J = a.s.job_off[c + 1] - j0;
    const uint64_t nb = (J + kSeriesBatch - 1) / kSeriesBatch;
    const int32_t* __restrict__ node = a.s.out_node + j0;
    const uint32_t* __restrict__ start = a.s.out_start + j0;
    const uint32_t* __restrict__ finish = a.s.out_finish + j0;
    const uint4* __restrict__ jobs = a.s.jobs + j0;
    const uint2* __restrict__ summ = a.summ + (j0 / kSeriesBatch + c);
    const uint32_t TS = series_tile(N);
    const uint32_t n = a.n_samples, period = a.period;
    // the two counters are kept in kSeriesRep copies, one per lane residue: the jobs of a wave are
    // neighbours in the stream, so their ranges begin and end on the same few samples
    uint32_t* const run_rows = d + 2u * N * TS;
    uint32_t* const que_rows = run_rows + kSeriesRep * TS;
    uint32_t* const res_row = que_rows + kSeriesRep * TS;  // two rows: cores, memory utilization
    uint32_t* const my_run = run_rows + (lane % kSeriesRep) * TS;
    uint32_t* const my_que = que_rows + (lane % kSeriesRep) * TS;
    const uint32_t n_rows = 2u * N + 2u * kSeriesRep;

    // SetTotalResources: u32 sums of the physical nodes
    if (tid < 2) tot[tid] = 0u;
    __syncthreads();
    uint32_t tc = 0, tm = 0;
    for (uint32_t i = tid; i < N; i += kStateThreads) {
        const uint2 cap = a.s.cap[n0 + i];
        tc += cap.x;
        tm += cap.y;
    }
    for (int o = 32; o > 0; o >>= 1) {
        tc += (uint32_t)__shfl_xor((int)tc, o);
        tm += (uint32_t)__shfl_xor((int)tm, o);
    }
    if (lane == 0) {
        atomicAdd(&tot[0], tc);
        atomicAdd(&tot[1], tm);
    }
    __syncthreads();
    const float ftc = (float)tot[0], ftm = (float)tot[1];

    uint64_t b_lo = 0;  // every batch below ended at or before the current tile's first sample
    for (uint32_t k0 = 0; k0 < n; k0 += TS) {
        const uint32_t tsa = n - k0 < TS ? n - k0 : TS;
        // both fit: the last sample of the series is at most 0xFFFFFFFE
        const uint32_t t_first = a.t0 + k0 * period, t_last = t_first + (tsa - 1u) * period;
        {  // zero the rows, 16 B per store (the dynamic LDS base is 16 B aligned)
            const uint32_t words = n_rows * TS;
            uint4* const d4 = reinterpret_cast<uint4*>(d);
            for (uint32_t i = tid; i < words / 4u; i += kStateThreads) d4[i] = make_uint4(0u, 0u, 0u, 0u);
            if (tid < (words & 3u)) d[(words & ~3u) + tid] = 0u;
        }
        __syncthreads();

        // tile-local index of the first sample at or after x, clipped to the tile; the quotient by
        // the period is the high word of x * ceil(2^64 / period), exact for every 32-bit x
        auto kt = [&](uint32_t x) -> uint32_t {
            if (x <= t_first) return 0u;
            const uint32_t y = x - t_first - 1u;
            const uint32_t q = period == 1u ? y : (uint32_t)__umul64hi(a.magic, (uint64_t)y);
            return q >= tsa ? tsa : q + 1u;
        };
        auto apply = [&](int32_t k, uint32_t s, uint32_t f, uint4 jr) {
            const bool placed = k >= 0 && (uint32_t)k < N;
            if (jr.x > t_last || (placed && f <= t_first)) return;
            const uint32_t ka = kt(jr.x), ks = placed ? kt(s) : tsa;
            range_add(my_que, ka, ks, tsa, 1u);
            if (placed) {
                const uint32_t kf = kt(f);
                range_add(my_run, ks, kf, tsa, 1u);
                if (jr.z) range_add(d + (uint32_t)k * TS, ks, kf, tsa, jr.z);
                if (jr.w) range_add(d + (N + (uint32_t)k) * TS, ks, kf, tsa, jr.w);
            }
        };

        bool leading = true;
        for (uint64_t base = b_lo; base < nb; base += kStateThreads) {
            const uint64_t b = base + tid;
            bool hit = false, dead = false, past = false;
            if (b < nb) {
                const uint2 s = summ[b];
                past = s.x > t_last;
                dead = s.y <= t_first;
                hit = !past && !dead;
            }
            const uint64_t hm = __ballot(hit), dm = __ballot(dead), pm = __ballot(past);
            if (lane == 0) {
                masks[0][wave] = hm;
                masks[1][wave] = dm;
                masks[2][wave] = pm;
            }
            __syncthreads();
            uint32_t lead = 0, n_hit = 0, before = 0;
            bool counting = leading, any_past = false;
            for (uint32_t w = 0; w < 4; ++w) {
                any_past |= masks[2][w] != 0;
                if (w == wave) before = n_hit;
                n_hit += (uint32_t)__popcll(masks[0][w]);
                if (counting) {
                    const uint64_t live = ~masks[1][w];
                    if (live == 0) {
                        lead += 64u;
                    } else {
                        lead += (uint32_t)__builtin_ctzll(live);
                        counting = false;
                    }
                }
            }
            if (hit) hits[before + (uint32_t)__popcll(hm & ((1ull << lane) - 1ull))] = tid;
            __syncthreads();
            // the hit batches eight at a time: every load of a group is issued before its first use
            n_hit = sgpr(n_hit);
            for (uint32_t h0 = 0; h0 < n_hit; h0 += kGroup) {
                int32_t k[kGroup];
                uint32_t s[kGroup], f[kGroup];
                uint4 jr[kGroup];
                bool ok[kGroup];
#pragma unroll
                for (uint32_t u = 0; u < kGroup; ++u) {
                    const uint64_t i = (base + hits[h0 + u < n_hit ? h0 + u : h0]) * kSeriesBatch + tid;
                    ok[u] = h0 + u < n_hit && i < J;
                    if (ok[u]) {
                        k[u] = node[i];
                        s[u] = start[i];
                        f[u] = finish[i];
                        jr[u] = jobs[i];
                    }
                }
#pragma unroll
                for (uint32_t u = 0; u < kGroup; ++u)
                    if (ok[u]) apply(k[u], s[u], f[u], jr[u]);
            }
            if (leading) {
                b_lo += lead;
                leading = lead == kStateThreads;
            }
            __syncthreads();  // masks and hits are rewritten by the next round
            if (any_past) break;
        }
        __syncthreads();

        // prefix sums along the samples, one thread per row; node rows leave their float32 term
        for (uint32_t r = tid; r < n_rows; r += kStateThreads) {
            uint32_t* row = d + r * TS;
            uint32_t acc = 0;
            if (r < 2u * N) {
                const bool mem = r >= N;
                const uint32_t i = mem ? r - N : r;
                const uint2 cap = a.s.cap[n0 + i], fr0 = a.s.free0[n0 + i];
                const float fcap = (float)(mem ? cap.y : cap.x);
                const uint32_t fr = mem ? fr0.y : fr0.x;
#pragma unroll 16
                for (uint32_t k = 0; k < tsa; ++k) {
                    acc += row[k];
                    row[k] = __float_as_uint(__fsub_rn(fcap, (float)(fr - acc)));
                }
            } else {
#pragma unroll 8
                for (uint32_t k = 0; k < tsa; ++k) {
                    acc += row[k];
                    row[k] = acc;
                }
            }
        }
        __syncthreads();

        // GetResourceUtilization: serial in node order, one lane per (sample, resource)
        for (uint32_t x = tid; x < 2u * tsa; x += kStateThreads) {
            const uint32_t mem = x >= tsa ? 1u : 0u, k = x - mem * tsa;
            const uint32_t* col = d + mem * N * TS + k;
            float f = 0.0f;
#pragma unroll 32
            for (uint32_t i = 0; i < N; ++i) f = __fadd_rn(f, __uint_as_float(col[i * TS]));
            res_row[mem * TS + k] = __float_as_uint(__fdiv_rn(f, mem ? ftm : ftc));
        }
        __syncthreads();

        if (tid < tsa) {
            uint32_t nrun = 0, nque = 0;
#pragma unroll
            for (uint32_t r = 0; r < kSeriesRep; ++r) {
                nrun += run_rows[r * TS + tid];
                nque += que_rows[r * TS + tid];
            }
            const uint4 v = make_uint4(res_row[tid], res_row[TS + tid], nrun, nque);
            reinterpret_cast<uint4*>(a.out)[(size_t)c * n + k0 + tid] = v;
        }
        __syncthreads();  // the rows are zeroed for the next tile
    }
}

}  // namespace

hipError_t launch_series_summary(const SeriesArgs& a, hipStream_t s) {
    if (a.s.n_clusters == 0) return hipSuccess;
    hipLaunchKernelGGL(series_summary_kernel, dim3(a.s.n_clusters), dim3(kStateThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_state_series(const SeriesArgs& a, uint32_t max_n, hipStream_t s) {
    if (a.s.n_clusters == 0) return hipSuccess;
    // series_tile(N) <= kSeriesMaxTile samples of series_rows(N) rows, N <= max_n, within kSeriesLds
    if (max_n > 1024u) return hipErrorInvalidValue;  // the ABI's node limit: a tile of at least 9 samples
    uint32_t lds = 4u * series_rows(max_n) * kSeriesMaxTile;
    if (lds > kSeriesLds) lds = kSeriesLds;
    hipError_t st = hipFuncSetAttribute(reinterpret_cast<const void*>(series_kernel),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)kSeriesLds);
    if (st != hipSuccess) return st;
    hipLaunchKernelGGL(series_kernel, dim3(a.s.n_clusters), dim3(kStateThreads), lds, s, a);
    return hipGetLastError();
}

hipError_t launch_state(const StateArgs& a, uint32_t max_n, hipStream_t s) {
    if (a.n_clusters == 0) return hipSuccess;
    hipLaunchKernelGGL(state_kernel, dim3(a.n_clusters), dim3(kStateThreads), 2 * max_n * sizeof(uint32_t), s, a);
    return hipGetLastError();
}

}  // namespace mcs
