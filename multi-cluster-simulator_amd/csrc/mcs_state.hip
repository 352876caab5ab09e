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
//
// After a FIFO trading run (policy FIFO with borrow and/or trader) the kernels are
// the TRADE instantiations and read a second stream, the lender's lent runs:
//   - a node is also held by every lent run of this lender with start <= t < finish, with the cores
//     and memory of the borrower's job (scheduler.go:277-290); the run counts in `running` and never
//     in `queued` (the LentQueue is the lender's foreign work);
//   - an own job moved to the BorrowedQueue (MCS_NODE_BORROWED, start = the borrow tick) is queued on
//     [arrival, start) and never running here; a job undecided at t_max_s stays queued;
//   - a node index at or above the physical node count is a zero-capacity virtual node
//     (AddVirtualNode, cluster.go:65-85), which only a 0-core 0-memory job takes: the record counts
//     as placed and running and touches no node row (every row index is guarded by k < N).  The
//     utilization sums run over the physical nodes only: a virtual node's term is
//     float32(0) - float32(0) = +0, and x + (+0) = x for every partial sum x these sums reach (they
//     start at +0 and never reach -0), and the totals are not recomputed (cluster.go:79), so the
//     virtual nodes change no bit.
// The plain instantiations read an index >= N as "unplaced", as they always did, and never touch the
// second stream.  lent_hist / lent_chunk_scan / lent_scan / lent_scatter / lent_summary_kernel build
// the per-lender lists from the engine's lent log (execution order, 32 B records) once per run.
//
// After a DELAY trading run (mcs_dtrade_state_series) dt_state_kernel and dt_series_kernel, further
// down, rebuild the record with virtual-node rows, Foreign jobs and 64-bit wrapping counters; in a
// trading session (mcs_trade_session_state_series) their SEG instantiations do, behind
// dt_foreign_live_kernel's per-call compaction of the Foreign log.  A trading session's cursor
// (mcs_trade_stream_next) keeps that list between calls: dt_stream_foreign_kernel.
//
// In an online session (mcs_online_state_series) the kernels are the SEG instantiations
// of the plain code: a cluster's rows are the first job_cnt[c] of the segment at job_off[c], and its
// batch summaries are indexed over segment capacity (series_summ_size).  Nothing else differs.
#include "mcs_internal.h"
#include "mcs_wave.h"

namespace mcs {

namespace {

constexpr int kStateThreads = 256;

// The rows of cluster c.  SEG: the first job_cnt[c] rows of the segment at job_off[c] (an online
// session: segments with slack after an append); else the dense CSR of a batch run.
// A job that no horizon has decided yet reads MCS_NODE_UNPLACED / MCS_TIME_NONE, which the plain
// code below already takes as "queued from its arrival on, never running".
template <bool SEG>
__device__ __forceinline__ uint64_t rows_of(const StateArgs& a, uint32_t c) {
    if constexpr (SEG)
        return a.job_cnt[c];
    else
        return a.job_off[c + 1] - a.job_off[c];
}

template <bool TRADE, bool SEG = false>
__global__ __launch_bounds__(kStateThreads) void state_kernel(StateArgs a) {
    static_assert(!(TRADE && SEG), "an online session has no trading");
    extern __shared__ uint32_t used[];  // [2 * max_n]: cores then memory per node
    const uint32_t c = blockIdx.x;
    const uint32_t tid = threadIdx.x;
    const uint32_t n0 = a.node_off[c], N = a.node_off[c + 1] - n0;
    for (uint32_t i = tid; i < 2u * N; i += kStateThreads) used[i] = 0u;
    __syncthreads();

    const uint64_t j0 = a.job_off[c];
    const uint32_t J = (uint32_t)rows_of<SEG>(a, c);
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
        if constexpr (TRADE) {
            if (k >= 0 && s <= t && t < f) {
                if ((uint32_t)k < N) {  // (a virtual node has no row)
                    const uint2 cm = *reinterpret_cast<const uint2*>(&jobs[i].z);
                    atomicAdd(&used[k], cm.x);
                    atomicAdd(&used[N + k], cm.y);
                }
                ++nrun;
            }
        } else if (k >= 0 && (uint32_t)k < N && s <= t && t < f) {
            const uint2 cm = *reinterpret_cast<const uint2*>(&jobs[i].z);
            atomicAdd(&used[k], cm.x);
            atomicAdd(&used[N + k], cm.y);
            ++nrun;
        }
    }
    if constexpr (TRADE) {  // the lender's lent runs, in any order
        const uint32_t l0 = a.lent_off[c], nl = a.lent_off[c + 1] - l0;
        const uint4* __restrict__ lr = reinterpret_cast<const uint4*>(a.lent + l0);
        for (uint32_t i = tid; i < nl; i += kStateThreads) {
            const uint4 r = lr[2u * i];  // {node, start, finish, cores}
            if (r.y <= t && t < r.z) {
                if (r.x < N) {
                    atomicAdd(&used[r.x], r.w);
                    atomicAdd(&used[N + r.x], lr[2u * i + 1u].x);
                }
                ++nrun;
            }
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

template <bool TRADE, bool SEG = false>
__global__ __launch_bounds__(kStateThreads) void series_summary_kernel(SeriesArgs a) {
    const uint32_t c = blockIdx.x;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t N = a.s.node_off[c + 1] - a.s.node_off[c];
    const uint64_t j0 = a.s.job_off[c];
    const uint64_t J = rows_of<SEG>(a.s, c);
    const uint64_t nb = (J + kSeriesBatch - 1) / kSeriesBatch;
    const int32_t* __restrict__ node = a.s.out_node + j0;
    const uint32_t* __restrict__ start = a.s.out_start + j0;
    const uint32_t* __restrict__ finish = a.s.out_finish + j0;
    const uint4* __restrict__ jobs = a.s.jobs + j0;
    uint2* __restrict__ summ = a.summ + (j0 / kSeriesBatch + c);
    (void)start;
    (void)N;
    for (uint64_t b = wave; b < nb; b += kStateThreads / kWave) {
        uint32_t amin = kNone, emax = 0u;
#pragma unroll
        for (uint32_t u = 0; u < kSeriesBatch / kWave; ++u) {
            const uint64_t i = b * kSeriesBatch + u * kWave + lane;
            if (i < J) {
                const uint32_t arr = jobs[i].x;
                const int32_t k = node[i];
                uint32_t end;
                if constexpr (TRADE)  // borrowed: out of the queue at its borrow tick; undecided: queued for good
                    end = k >= 0 ? finish[i] : (k == MCS_NODE_BORROWED ? start[i] : kNone);
                else
                    end = (k >= 0 && (uint32_t)k < N) ? finish[i] : kNone;  // unplaced: queued for good
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

template <bool TRADE, bool SEG = false>
__global__ __launch_bounds__(kStateThreads) void series_kernel(SeriesArgs a) {
    static_assert(!(TRADE && SEG), "an online session has no trading");
    extern __shared__ uint32_t d[];   // [2 N + 2 kSeriesRep + 2][TS]
    __shared__ uint64_t masks[3][4];  // hit / dead / past ballots of a summary round, per wave
    __shared__ uint32_t hits[kStateThreads];  // the round's hit batches, in stream order
    __shared__ uint32_t tot[2];
    const uint32_t c = blockIdx.x;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t n0 = a.s.node_off[c], N = a.s.node_off[c + 1] - n0;
    const uint64_t j0 = a.s.job_off[c];
    const uint64_t J = rows_of<SEG>(a.s, c);
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
    // (TRADE) the lender's lent runs and their summaries, with a cursor of their own
    uint32_t lb_lo = 0, lent_n = 0;
    const uint4* __restrict__ lr = nullptr;
    const uint2* __restrict__ lsumm = nullptr;
    if constexpr (TRADE) {
        const uint32_t l0 = a.s.lent_off[c];
        lent_n = a.s.lent_off[c + 1] - l0;
        lr = reinterpret_cast<const uint4*>(a.s.lent + l0);
        lsumm = a.s.lent_summ + (l0 / kSeriesBatch + c);
    }
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
            if constexpr (TRADE) {
                // placed on a physical or a virtual node; borrowed: queued up to the borrow tick s
                const bool placed = k >= 0, gone = placed || k == MCS_NODE_BORROWED;
                if (jr.x > t_last || (placed && f <= t_first) || (!placed && gone && s <= t_first)) return;
                const uint32_t ka = kt(jr.x), ks = gone ? kt(s) : tsa;
                range_add(my_que, ka, ks, tsa, 1u);
                if (placed) {
                    const uint32_t kf = kt(f);
                    range_add(my_run, ks, kf, tsa, 1u);
                    if ((uint32_t)k < N) {  // (a virtual node has no row)
                        if (jr.z) range_add(d + (uint32_t)k * TS, ks, kf, tsa, jr.z);
                        if (jr.w) range_add(d + (N + (uint32_t)k) * TS, ks, kf, tsa, jr.w);
                    }
                }
                return;
            }
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
        if constexpr (TRADE) {
            // the lender's lent runs, as the own jobs above: the summaries are tested from a cursor that
            // skips the leading batches that ended before the tile (they stay ended: tiles only move
            // on) up to the first batch whose x is past the tile.  x is the earliest start of the
            // batch AND of every batch behind it (lent_summary_kernel), so that break is right in
            // whatever order the lists are.  A hit batch is read by the whole workgroup; every run is
            // tested on its own.  A run feeds the running row and its node's two rows, never the queue.
            const uint32_t nl = lent_n;
            const uint32_t nlb = (nl + kSeriesBatch - 1u) / kSeriesBatch;
            bool lleading = true;
            for (uint32_t base = lb_lo; base < nlb; base += kStateThreads) {
                const uint32_t b = base + tid;
                bool hit = false, dead = false, past = false;
                if (b < nlb) {
                    const uint2 s = lsumm[b];
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
                bool counting = lleading, any_past = false;
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
                n_hit = sgpr(n_hit);
                for (uint32_t h = 0; h < n_hit; ++h) {
                    const uint32_t i = (base + hits[h]) * kSeriesBatch + tid;
                    if (i < nl) {
                        const uint4 r = lr[2u * i];  // {node, start, finish, cores}
                        if (r.y <= t_last && r.z > t_first) {
                            const uint32_t ks = kt(r.y), kf = kt(r.z);
                            range_add(my_run, ks, kf, tsa, 1u);
                            if (r.x < N) {  // (a virtual node has no row)
                                const uint32_t m = lr[2u * i + 1u].x;
                                if (r.w) range_add(d + r.x * TS, ks, kf, tsa, r.w);
                                if (m) range_add(d + (N + r.x) * TS, ks, kf, tsa, m);
                            }
                        }
                    }
                }
                if (lleading) {
                    lb_lo += lead;
                    lleading = lead == kStateThreads;
                }
                __syncthreads();  // masks and hits are rewritten by the next round
                if (any_past) break;
            }
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

// ---- the record after a DELAY trading run ----------------------------------------
//
// The third form of the three kernels, kernels of their own so that the plain and the TRADE
// instantiations above stay the code they are.  What differs:
//   - cluster c has NN = N + nv rows: its physical nodes, then the virtual nodes it received, whose
//     capacity and initial free counters are the contract's {cores, mem} (AddVirtualNode,
//     cluster.go:65-85).  A virtual row holds nothing before its trade, so its term is +0 until then.
//     An own job's node index runs over NN; every row index is guarded by k < NN.
//   - the counters are Go uint64: free = free0 - held (mod 2^64), the term is
//     float32(cap) - float32(uint64 free), round to nearest even.  The rows accumulate in 64-bit LDS
//     words with 64-bit atomics; differences and prefix sums wrap mod 2^64, which is exact.
//   - a Foreign job (mcs_foreign_rec with responder == c) holds {c, m} of its row on
//     start_s < t < finish_s: AllocateVirtualNodeResources runs in phase D of tick start_s, after that
//     tick's sample.  It counts in `running`, never in `queued`.  The log is scanned as it is by every
//     workgroup (C5-DELAY logs 232 records, 9 KB, §13); no order is assumed, the loop is bounded by
//     the record count passed at launch.
//   - the utilization sums run over the NN rows in order; the totals stay the physical sums.
// In a trading session (mcs_trade_session_state_series) both kernels are their SEG
// instantiations: the row count comes from job_cnt (rows_of) and the summaries are the TRADE summary
// kernel's SEG form, indexed over segment capacity.  Nothing else differs in dt_state_kernel.  The SEG
// series kernel scans, in place of the log, the list dt_foreign_live_kernel compacted from it for
// the call (a session's log grows with its age; the list holds what can hold at one of the call's
// samples).  The list's order is arbitrary: a Foreign hold is two integer adds modulo 2^64 into the
// row accumulators and an integer range count, all commutative and exact, so the order changes no bit.
__device__ __forceinline__ void range_add64(unsigned long long* row, uint32_t lo, uint32_t hi, uint32_t tsa,
                                            unsigned long long v) {
    if (lo < hi) {
        atomicAdd(&row[lo], v);
        if (hi < tsa) atomicAdd(&row[hi], 0ull - v);
    }
}

template <bool SEG = false>
__global__ __launch_bounds__(kStateThreads) void dt_state_kernel(DtStateArgs a) {
    extern __shared__ unsigned long long used64[];  // [2 * max_nn]: cores then memory per row
    const uint32_t c = blockIdx.x;
    const uint32_t tid = threadIdx.x;
    const uint32_t n0 = a.s.node_off[c], N = a.s.node_off[c + 1] - n0;
    const uint32_t nvc = a.nv[c] < a.V ? a.nv[c] : a.V, NN = N + nvc;
    for (uint32_t i = tid; i < 2u * NN; i += kStateThreads) used64[i] = 0ull;
    __syncthreads();

    const uint64_t j0 = a.s.job_off[c];
    const uint32_t J = (uint32_t)rows_of<SEG>(a.s, c);
    const int32_t* __restrict__ node = a.s.out_node + j0;
    const uint32_t* __restrict__ start = a.s.out_start + j0;
    const uint32_t* __restrict__ finish = a.s.out_finish + j0;
    const uint4* __restrict__ jobs = a.s.jobs + j0;
    const uint32_t t = a.s.t;
    uint32_t nrun = 0;
#pragma unroll 4
    for (uint32_t i = tid; i < J; i += kStateThreads) {
        const int32_t k = __builtin_nontemporal_load(node + i);
        const uint32_t s = __builtin_nontemporal_load(start + i);
        const uint32_t f = __builtin_nontemporal_load(finish + i);
        if (k >= 0 && s <= t && t < f) {
            if ((uint32_t)k < NN) {
                const uint2 cm = *reinterpret_cast<const uint2*>(&jobs[i].z);
                atomicAdd(&used64[k], (unsigned long long)cm.x);
                atomicAdd(&used64[NN + k], (unsigned long long)cm.y);
            }
            ++nrun;
        }
    }
    for (uint32_t i = tid; i < a.n_foreign; i += kStateThreads) {
        const mcs_foreign_rec r = a.flog[i];
        if (r.responder == c && r.start_s < t && t < r.finish_s) {
            if (r.node < NN) {
                atomicAdd(&used64[r.node], (unsigned long long)r.c);
                atomicAdd(&used64[NN + r.node], (unsigned long long)r.m);
            }
            ++nrun;
        }
    }
    for (int o = 32; o > 0; o >>= 1) nrun += (uint32_t)__shfl_xor((int)nrun, o);
    __shared__ uint32_t run_total;
    if (tid == 0) run_total = 0u;
    __syncthreads();
    if ((tid & 63u) == 0u) atomicAdd(&run_total, nrun);
    __syncthreads();

    if (tid == 0) {
        float cu = 0.0f, mu = 0.0f;
        uint32_t tc = 0, tm = 0;
        for (uint32_t i = 0; i < NN; ++i) {
            const uint2 cap = i < N ? a.s.cap[n0 + i] : a.vcap[(size_t)c * a.V + (i - N)];
            const uint2 fr0 = i < N ? a.s.free0[n0 + i] : cap;
            const unsigned long long fc = (unsigned long long)fr0.x - used64[i];
            const unsigned long long fm = (unsigned long long)fr0.y - used64[NN + i];
            cu = __fadd_rn(cu, __fsub_rn((float)cap.x, (float)fc));
            mu = __fadd_rn(mu, __fsub_rn((float)cap.y, (float)fm));
            if (i < N) {  // SetTotalResources ran before any trade (cluster.go:79)
                tc += cap.x;
                tm += cap.y;
            }
        }
        mcs_cluster_state st;
        st.cores_utilization = __fdiv_rn(cu, (float)tc);
        st.memory_utilization = __fdiv_rn(mu, (float)tm);
        st.total_cpu = tc;
        st.total_memory = tm;
        st.running = run_total;
        st.t_s = t;
        a.s.out[c] = st;
    }
}

// series_kernel's tile walk with 64-bit node rows: LDS holds 2 NN rows of TS u64 (cores, memory),
// then 2 kSeriesRep counter rows and two result rows of TS u32, TS = dt_series_tile(NN).
template <bool SEG = false>
__global__ __launch_bounds__(kStateThreads) void dt_series_kernel(DtSeriesArgs a) {
    extern __shared__ unsigned long long d64[];  // [2 NN][TS] u64, then [2 kSeriesRep + 2][TS] u32
    __shared__ uint64_t masks[3][4];
    __shared__ uint32_t hits[kStateThreads];
    __shared__ uint32_t tot[2];
    const StateArgs& s_ = a.d.s;
    const uint32_t c = blockIdx.x;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t n0 = s_.node_off[c], N = s_.node_off[c + 1] - n0;
    const uint32_t nvc = a.d.nv[c] < a.d.V ? a.d.nv[c] : a.d.V, NN = N + nvc;
    const uint64_t j0 = s_.job_off[c];
    const uint64_t J = rows_of<SEG>(s_, c);
    const uint64_t nb = (J + kSeriesBatch - 1) / kSeriesBatch;
    const int32_t* __restrict__ node = s_.out_node + j0;
    const uint32_t* __restrict__ start = s_.out_start + j0;
    const uint32_t* __restrict__ finish = s_.out_finish + j0;
    const uint4* __restrict__ jobs = s_.jobs + j0;
    const uint2* __restrict__ summ = a.summ + (j0 / kSeriesBatch + c);
    const uint2* __restrict__ vcap = a.d.vcap + (size_t)c * a.d.V;
    const uint32_t TS = dt_series_tile(NN);
    const uint32_t n = a.n_samples, period = a.period;
    uint32_t* const d32 = reinterpret_cast<uint32_t*>(d64 + (size_t)2u * NN * TS);
    uint32_t* const run_rows = d32;
    uint32_t* const que_rows = run_rows + kSeriesRep * TS;
    uint32_t* const res_row = que_rows + kSeriesRep * TS;
    uint32_t* const my_run = run_rows + (lane % kSeriesRep) * TS;
    uint32_t* const my_que = que_rows + (lane % kSeriesRep) * TS;

    if (tid < 2) tot[tid] = 0u;
    __syncthreads();
    uint32_t tc = 0, tm = 0;
    for (uint32_t i = tid; i < N; i += kStateThreads) {
        const uint2 cap = s_.cap[n0 + i];
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
    // the Foreign records a tile scans: the log as it is, or (SEG, a trading session's call with the
    // pre-pass) dt_foreign_live_kernel's list, whose length is read here: the pre-pass ran before
    // this launch on the same stream
    const mcs_foreign_rec* __restrict__ flog = a.d.flog;
    uint32_t n_foreign = a.d.n_foreign;
    if constexpr (SEG) {
        if (a.live_n) {
            const uint32_t nl = *a.live_n;
            flog = a.live;
            n_foreign = nl < n_foreign ? nl : n_foreign;  // (the list is sized to the log)
        }
    }

    uint64_t b_lo = 0;
    for (uint32_t k0 = 0; k0 < n; k0 += TS) {
        const uint32_t tsa = n - k0 < TS ? n - k0 : TS;
        const uint32_t t_first = a.t0 + k0 * period, t_last = t_first + (tsa - 1u) * period;
        {  // zero every row: 2 NN TS u64 words and (2 kSeriesRep + 2) TS u32 words
            const uint32_t w64 = 2u * NN * TS, w32 = (2u * kSeriesRep + 2u) * TS;
            for (uint32_t i = tid; i < w64; i += kStateThreads) d64[i] = 0ull;
            for (uint32_t i = tid; i < w32; i += kStateThreads) d32[i] = 0u;
        }
        __syncthreads();

        auto kt = [&](uint32_t x) -> uint32_t {
            if (x <= t_first) return 0u;
            const uint32_t y = x - t_first - 1u;
            const uint32_t q = period == 1u ? y : (uint32_t)__umul64hi(a.magic, (uint64_t)y);
            return q >= tsa ? tsa : q + 1u;
        };
        auto apply = [&](int32_t k, uint32_t s, uint32_t f, uint4 jr) {
            const bool placed = k >= 0;  // on a physical or a virtual node; -1: undecided, queued for good
            if (jr.x > t_last || (placed && f <= t_first)) return;
            const uint32_t ka = kt(jr.x), ks = placed ? kt(s) : tsa;
            range_add(my_que, ka, ks, tsa, 1u);
            if (placed) {
                const uint32_t kf = kt(f);
                range_add(my_run, ks, kf, tsa, 1u);
                if ((uint32_t)k < NN) {
                    if (jr.z) range_add64(d64 + (size_t)(uint32_t)k * TS, ks, kf, tsa, jr.z);
                    if (jr.w) range_add64(d64 + (size_t)(NN + (uint32_t)k) * TS, ks, kf, tsa, jr.w);
                }
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
            n_hit = sgpr(n_hit);
            for (uint32_t h = 0; h < n_hit; ++h) {
                const uint64_t i = (base + hits[h]) * kSeriesBatch + tid;
                if (i < J) apply(node[i], start[i], finish[i], jobs[i]);
            }
            if (leading) {
                b_lo += lead;
                leading = lead == kStateThreads;
            }
            __syncthreads();  // masks and hits are rewritten by the next round
            if (any_past) break;
        }
        // the Foreign jobs of this responder: they hold on start_s < t < finish_s
        for (uint32_t i = tid; i < n_foreign; i += kStateThreads) {
            const mcs_foreign_rec* __restrict__ r = flog + i;
            if (r->responder != c) continue;
            const uint32_t fs = r->start_s, ff = r->finish_s;
            if (fs >= t_last || ff <= t_first) continue;  // (fs < t_last <= 0xFFFFFFFE: fs + 1 fits)
            const uint32_t ks = kt(fs + 1u), kf = kt(ff);
            range_add(my_run, ks, kf, tsa, 1u);
            const uint32_t k = r->node;
            if (k < NN) {
                const unsigned long long fc = r->c, fm = r->m;
                if (fc) range_add64(d64 + (size_t)k * TS, ks, kf, tsa, fc);
                if (fm) range_add64(d64 + (size_t)(NN + k) * TS, ks, kf, tsa, fm);
            }
        }
        __syncthreads();

        // prefix sums along the samples, one thread per row; node rows leave their float32 term
        for (uint32_t r = tid; r < 2u * NN + 2u * kSeriesRep; r += kStateThreads) {
            if (r < 2u * NN) {
                unsigned long long* row = d64 + (size_t)r * TS;
                const bool mem = r >= NN;
                const uint32_t i = mem ? r - NN : r;
                const uint2 cap = i < N ? s_.cap[n0 + i] : vcap[i - N];
                const uint2 fr0 = i < N ? s_.free0[n0 + i] : cap;
                const float fcap = (float)(mem ? cap.y : cap.x);
                const unsigned long long fr = mem ? fr0.y : fr0.x;
                unsigned long long acc = 0ull;
#pragma unroll 8
                for (uint32_t k = 0; k < tsa; ++k) {
                    acc += row[k];
                    row[k] = (unsigned long long)__float_as_uint(__fsub_rn(fcap, (float)(fr - acc)));
                }
            } else {
                uint32_t* row = d32 + (r - 2u * NN) * TS;
                uint32_t acc = 0;
#pragma unroll 8
                for (uint32_t k = 0; k < tsa; ++k) {
                    acc += row[k];
                    row[k] = acc;
                }
            }
        }
        __syncthreads();

        // GetResourceUtilization: serial in row order, one lane per (sample, resource)
        for (uint32_t x = tid; x < 2u * tsa; x += kStateThreads) {
            const uint32_t mem = x >= tsa ? 1u : 0u, k = x - mem * tsa;
            const unsigned long long* col = d64 + (size_t)mem * NN * TS + k;
            float f = 0.0f;
#pragma unroll 16
            for (uint32_t i = 0; i < NN; ++i) f = __fadd_rn(f, __uint_as_float((uint32_t)col[(size_t)i * TS]));
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

// The pre-pass of a trading session's call: the Foreign records that can hold at one of the call's
// samples, which lie in [t_first, t_last]: start_s < t_last, finish_s > t_first and a window that is
// not empty.  One record per thread.  A wave counts its keepers with a ballot, lane 0 takes the wave's
// room in the list with one atomic, and every keeper stores its record behind the keepers of the
// lower lanes: the list's order is the order in which the waves arrive, which no reader depends on
// (see above).  The list has room for the whole log, so it cannot overflow; the store is guarded all
// the same.
__global__ __launch_bounds__(kStateThreads) void dt_foreign_live_kernel(const mcs_foreign_rec* __restrict__ flog,
                                                                        uint32_t n_foreign, uint32_t t_first,
                                                                        uint32_t t_last,
                                                                        mcs_foreign_rec* __restrict__ live,
                                                                        uint32_t* __restrict__ live_n) {
    const uint32_t i = blockIdx.x * kStateThreads + threadIdx.x;  // (n_foreign <= 2^32 - 2: no wrap below it)
    const uint32_t lane = threadIdx.x & 63u;
    mcs_foreign_rec r{};
    bool keep = false;
    if (i < n_foreign) {
        r = flog[i];
        keep = r.start_s < t_last && r.finish_s > t_first && r.start_s != r.finish_s;
    }
    const uint64_t km = __ballot(keep);
    if (km == 0ull) return;  // (uniform over the wave)
    uint32_t base = 0u;
    if (lane == 0u) base = atomicAdd(live_n, (uint32_t)__popcll(km));
    base = (uint32_t)__shfl((int)base, 0);
    if (keep) {
        const uint32_t at = base + (uint32_t)__popcll(km & ((1ull << lane) - 1ull));
        if (at < n_foreign) live[at] = r;
    }
}

// The Foreign take of a trading session's stream (mcs_trade_stream_next): the same
// compaction over two sources, one record per thread: thread i < old_n takes record i of the list the
// last call kept and keeps it while finish_s > t_first; the threads behind them take the log records
// appended since, [seen, n_log), and keep those with a window that is not empty and finish_s > t_first.
// Retiring is lazy: a record is dropped by the first call whose first sample it can no longer reach.
// Workgroup 0 also writes the call's virtual row counts from the session's cluster records.
__global__ __launch_bounds__(kStateThreads) void dt_stream_foreign_kernel(DtStreamForeignArgs a) {
    const uint32_t i = blockIdx.x * kStateThreads + threadIdx.x;  // (old_n + n_log - seen <= n_log <= 2^32 - 2)
    const uint32_t lane = threadIdx.x & 63u;
    if (blockIdx.x == 0u)
        for (uint32_t c = threadIdx.x; c < a.n_clusters; c += kStateThreads) {
            const uint32_t nv = a.nv_src[(size_t)c * a.nv_stride];
            a.nv_out[c] = nv < a.V ? nv : a.V;
        }
    const uint32_t n_new = a.n_log - a.seen;
    mcs_foreign_rec r{};
    bool keep = false;
    if (i < a.old_n) {
        r = a.old_list[i];
        keep = r.finish_s > a.t_first;
    } else if (i - a.old_n < n_new) {
        r = a.flog[a.seen + (i - a.old_n)];
        keep = r.start_s != r.finish_s && r.finish_s > a.t_first;
    }
    const uint64_t km = __ballot(keep);
    if (km == 0ull) return;  // (uniform over the wave)
    uint32_t base = 0u;
    if (lane == 0u) base = atomicAdd(a.new_n, (uint32_t)__popcll(km));
    base = (uint32_t)__shfl((int)base, 0);
    if (keep) {
        const uint32_t at = base + (uint32_t)__popcll(km & ((1ull << lane) - 1ull));
        if (at < a.cap) a.new_list[at] = r;
    }
}

// ---- the pre-pass over a FIFO trading run's lent log ---------------------------------------------
//
// The log is in execution order (starts ascend), every lender's records interleaved.  A counting
// sort by lender that keeps that order chunk by chunk: the log is cut in chunks of kLentChunk records;
// lent_hist_kernel counts each chunk's records per lender, lent_chunk_scan_kernel turns a lender's
// counts into the chunk's offset within the lender's list (and the list's length), lent_scan_kernel
// lays the lists out (exclusive scan over the lenders), lent_scatter_kernel moves the records, with
// the cores and memory of the borrower's job record.  Lender c's runs end up contiguous at
// [off[c], off[c + 1]), chunk after chunk, in no fixed order within a chunk: near enough to start
// order for the batch summaries to be narrow, and no reader assumes more.  A
// zero-duration run (finish == start) holds nothing; it is stored and joins no summary.
constexpr uint32_t kPrepThreads = 256;
constexpr uint32_t kLentChunk = 16u * kPrepThreads;
constexpr uint32_t kPrepMaxClusters = 1024;  // LDS counters per chunk (the trading path's cluster limit)

__global__ __launch_bounds__(kPrepThreads) void lent_hist_kernel(LentPrepArgs a) {
    __shared__ uint32_t hist[kPrepMaxClusters];
    const uint32_t tid = threadIdx.x, C = a.n_clusters;
    for (uint32_t l = tid; l < C; l += kPrepThreads) hist[l] = 0u;
    __syncthreads();
    const uint64_t i0 = (uint64_t)blockIdx.x * kLentChunk;
#pragma unroll 4
    for (uint32_t u = 0; u < kLentChunk / kPrepThreads; ++u) {
        const uint64_t i = i0 + u * kPrepThreads + tid;
        if (i < a.n) {
            const uint32_t l = a.log[i].lender;
            if (l < C) atomicAdd(&hist[l], 1u);
        }
    }
    __syncthreads();
    for (uint32_t l = tid; l < C; l += kPrepThreads) a.cnt[(size_t)blockIdx.x * C + l] = hist[l];
}

// one workgroup per lender: cnt[chunk][lender] becomes the records of the lender in the chunks
// before (exclusive scan along the chunks), cursor[lender] their total
__global__ __launch_bounds__(kPrepThreads) void lent_chunk_scan_kernel(LentPrepArgs a) {
    __shared__ uint32_t part[kPrepThreads];
    const uint32_t tid = threadIdx.x, l = blockIdx.x, C = a.n_clusters, nc = a.n_chunks;
    const uint32_t per = (nc + kPrepThreads - 1u) / kPrepThreads;
    const uint32_t lo = tid * per < nc ? tid * per : nc, hi = lo + per < nc ? lo + per : nc;
    uint32_t sum = 0;
    for (uint32_t ch = lo; ch < hi; ++ch) sum += a.cnt[(size_t)ch * C + l];
    part[tid] = sum;
    __syncthreads();
    uint32_t acc = 0;
    for (uint32_t w = 0; w < tid; ++w) acc += part[w];
    for (uint32_t ch = lo; ch < hi; ++ch) {
        const uint32_t n = a.cnt[(size_t)ch * C + l];
        a.cnt[(size_t)ch * C + l] = acc;
        acc += n;
    }
    if (tid == kPrepThreads - 1u) a.cursor[l] = acc;  // (the spans behind the last chunk are empty)
}

// one workgroup: off = exclusive scan of the list lengths (at most 1024 clusters, 4 per thread)
__global__ __launch_bounds__(kPrepThreads) void lent_scan_kernel(LentPrepArgs a) {
    __shared__ uint32_t part[kPrepThreads];
    const uint32_t tid = threadIdx.x, C = a.n_clusters;
    const uint32_t per = (C + kPrepThreads - 1u) / kPrepThreads;
    const uint32_t lo = tid * per < C ? tid * per : C, hi = lo + per < C ? lo + per : C;
    uint32_t sum = 0;
    for (uint32_t i = lo; i < hi; ++i) sum += a.cursor[i];
    part[tid] = sum;
    __syncthreads();
    uint32_t acc = 0;
    for (uint32_t w = 0; w < tid; ++w) acc += part[w];
    for (uint32_t i = lo; i < hi; ++i) {
        a.off[i] = acc;
        acc += a.cursor[i];
    }
    if (tid == kPrepThreads - 1u) a.off[C] = acc;
}

__global__ __launch_bounds__(kPrepThreads) void lent_scatter_kernel(LentPrepArgs a) {
    __shared__ uint32_t cur[kPrepMaxClusters];
    const uint32_t tid = threadIdx.x, C = a.n_clusters;
    for (uint32_t l = tid; l < C; l += kPrepThreads) cur[l] = a.off[l] + a.cnt[(size_t)blockIdx.x * C + l];
    __syncthreads();
    const uint64_t i0 = (uint64_t)blockIdx.x * kLentChunk;
#pragma unroll 4
    for (uint32_t u = 0; u < kLentChunk / kPrepThreads; ++u) {
        const uint64_t i = i0 + u * kPrepThreads + tid;
        if (i >= a.n) continue;
        const mcs_lent_rec r = a.log[i];
        if (r.lender >= C) continue;  // (not counted either)
        const uint32_t at = atomicAdd(&cur[r.lender], 1u);
        if (at >= a.n) continue;
        uint4 jr = make_uint4(0u, 0u, 0u, 0u);
        bool ok = r.borrower < C;
        if (ok) {
            const uint64_t j0 = a.job_off[r.borrower];
            ok = r.job < a.job_off[r.borrower + 1] - j0;
            if (ok) jr = a.jobs[j0 + r.job];
        }
        // (a record that names no job of this engine holds nothing: an empty range)
        uint4* out = reinterpret_cast<uint4*>(a.runs + at);
        out[0] = make_uint4(r.node, r.start_s, ok ? r.finish_s : r.start_s, jr.z);
        out[1] = make_uint4(jr.w, 0u, 0u, 0u);
    }
}

// Per kSeriesBatch runs of a lender's list {x, finish_max}; an empty run joins neither.  x starts as
// the batch's earliest start and becomes, in the second pass, the earliest start of the batch and of
// every batch behind it (a suffix minimum): "x is past the tile" then holds for all later batches
// too, in whatever order the list is.
__global__ __launch_bounds__(kStateThreads) void lent_summary_kernel(LentPrepArgs a) {
    __shared__ uint32_t part[kStateThreads];
    const uint32_t c = blockIdx.x, tid = threadIdx.x;
    const uint32_t lane = tid & 63u, wave = tid >> 6;
    const uint32_t l0 = a.off[c], nl = a.off[c + 1] - l0;
    const uint32_t nb = (nl + kSeriesBatch - 1u) / kSeriesBatch;
    const uint4* __restrict__ lr = reinterpret_cast<const uint4*>(a.runs + l0);
    uint2* summ = a.summ + (l0 / kSeriesBatch + c);
    for (uint32_t b = wave; b < nb; b += kStateThreads / kWave) {
        uint32_t smin = kNone, fmax = 0u;
#pragma unroll
        for (uint32_t u = 0; u < kSeriesBatch / kWave; ++u) {
            const uint32_t i = b * kSeriesBatch + u * kWave + lane;
            if (i < nl) {
                const uint4 r = lr[2u * i];
                if (r.y < r.z) {
                    smin = r.y < smin ? r.y : smin;
                    fmax = r.z > fmax ? r.z : fmax;
                }
            }
        }
        for (int o = 32; o > 0; o >>= 1) {
            const uint32_t x = (uint32_t)__shfl_xor((int)smin, o), y = (uint32_t)__shfl_xor((int)fmax, o);
            smin = x < smin ? x : smin;
            fmax = y > fmax ? y : fmax;
        }
        if (lane == 0) summ[b] = make_uint2(smin, fmax);
    }
    __syncthreads();  // (the summaries above are this workgroup's own writes)
    const uint32_t per = (nb + kStateThreads - 1u) / kStateThreads;
    const uint32_t lo = tid * per < nb ? tid * per : nb, hi = lo + per < nb ? lo + per : nb;
    uint32_t m = kNone;
    for (uint32_t b = lo; b < hi; ++b) {
        const uint32_t x = summ[b].x;
        m = x < m ? x : m;
    }
    part[tid] = m;
    __syncthreads();
    uint32_t acc = kNone;
    for (uint32_t w = tid + 1u; w < kStateThreads; ++w) acc = part[w] < acc ? part[w] : acc;
    for (uint32_t b = hi; b-- > lo;) {
        const uint32_t x = summ[b].x;
        acc = x < acc ? x : acc;
        summ[b].x = acc;
    }
}

}  // namespace

uint32_t lent_chunks(uint64_t n) { return (uint32_t)((n + kLentChunk - 1u) / kLentChunk); }

hipError_t launch_lent_prep(const LentPrepArgs& a, hipStream_t s) {
    if (a.n_clusters == 0) return hipSuccess;
    if (a.n_clusters > kPrepMaxClusters || a.n_chunks != lent_chunks(a.n)) return hipErrorInvalidValue;
    if (a.n_chunks) hipLaunchKernelGGL(lent_hist_kernel, dim3(a.n_chunks), dim3(kPrepThreads), 0, s, a);
    hipLaunchKernelGGL(lent_chunk_scan_kernel, dim3(a.n_clusters), dim3(kPrepThreads), 0, s, a);
    hipLaunchKernelGGL(lent_scan_kernel, dim3(1), dim3(kPrepThreads), 0, s, a);
    if (a.n_chunks) hipLaunchKernelGGL(lent_scatter_kernel, dim3(a.n_chunks), dim3(kPrepThreads), 0, s, a);
    hipLaunchKernelGGL(lent_summary_kernel, dim3(a.n_clusters), dim3(kStateThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_series_summary(const SeriesArgs& a, hipStream_t s) {
    if (a.s.n_clusters == 0) return hipSuccess;
    if (a.s.job_cnt)
        hipLaunchKernelGGL((series_summary_kernel<false, true>), dim3(a.s.n_clusters), dim3(kStateThreads), 0, s, a);
    else if (a.s.lent_off)
        hipLaunchKernelGGL(series_summary_kernel<true>, dim3(a.s.n_clusters), dim3(kStateThreads), 0, s, a);
    else
        hipLaunchKernelGGL(series_summary_kernel<false>, dim3(a.s.n_clusters), dim3(kStateThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_state_series(const SeriesArgs& a, uint32_t max_n, hipStream_t s) {
    if (a.s.n_clusters == 0) return hipSuccess;
    // series_tile(N) <= kSeriesMaxTile samples of series_rows(N) rows, N <= max_n, within kSeriesLds
    if (max_n > 1024u) return hipErrorInvalidValue;  // the ABI's node limit: a tile of at least 9 samples
    uint32_t lds = 4u * series_rows(max_n) * kSeriesMaxTile;
    if (lds > kSeriesLds) lds = kSeriesLds;
    if (a.s.job_cnt && a.s.lent_off) return hipErrorInvalidValue;  // no trading in an online session
    const void* fn = a.s.job_cnt    ? reinterpret_cast<const void*>(series_kernel<false, true>)
                     : a.s.lent_off ? reinterpret_cast<const void*>(series_kernel<true>)
                                    : reinterpret_cast<const void*>(series_kernel<false>);
    hipError_t st = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kSeriesLds);
    if (st != hipSuccess) return st;
    if (a.s.job_cnt)
        hipLaunchKernelGGL((series_kernel<false, true>), dim3(a.s.n_clusters), dim3(kStateThreads), lds, s, a);
    else if (a.s.lent_off)
        hipLaunchKernelGGL(series_kernel<true>, dim3(a.s.n_clusters), dim3(kStateThreads), lds, s, a);
    else
        hipLaunchKernelGGL(series_kernel<false>, dim3(a.s.n_clusters), dim3(kStateThreads), lds, s, a);
    return hipGetLastError();
}

hipError_t launch_dt_state(const DtStateArgs& a, uint32_t max_nn, hipStream_t s) {
    if (a.s.n_clusters == 0) return hipSuccess;
    if (max_nn == 0 || max_nn > 1280u) return hipErrorInvalidValue;  // 1024 physical + 256 virtual rows: 20 KB
    if (a.s.job_cnt)  // a trading session's segments
        hipLaunchKernelGGL(dt_state_kernel<true>, dim3(a.s.n_clusters), dim3(kStateThreads),
                           2 * max_nn * sizeof(unsigned long long), s, a);
    else
        hipLaunchKernelGGL(dt_state_kernel<false>, dim3(a.s.n_clusters), dim3(kStateThreads),
                           2 * max_nn * sizeof(unsigned long long), s, a);
    return hipGetLastError();
}

// the list of the Foreign records that can hold at a sample in [t_first, t_last]; live has room for
// n_foreign records, *live_n is their count afterwards
hipError_t launch_dt_foreign_live(const mcs_foreign_rec* flog, uint32_t n_foreign, uint32_t t_first, uint32_t t_last,
                                  mcs_foreign_rec* live, uint32_t* live_n, hipStream_t s) {
    hipError_t st = hipMemsetAsync(live_n, 0, sizeof(uint32_t), s);
    if (st != hipSuccess || n_foreign == 0) return st;
    const uint32_t blocks = (uint32_t)(((uint64_t)n_foreign + kStateThreads - 1u) / kStateThreads);
    hipLaunchKernelGGL(dt_foreign_live_kernel, dim3(blocks), dim3(kStateThreads), 0, s, flog, n_foreign, t_first,
                       t_last, live, live_n);
    return hipGetLastError();
}

hipError_t launch_dt_stream_foreign(const DtStreamForeignArgs& a, hipStream_t s) {
    // every index the kernel forms stays inside its array: the old list and the log within their lengths,
    // the new list within cap
    if (a.seen > a.n_log || a.old_n > a.seen || a.n_log > a.cap || !a.new_n || !a.nv_out || !a.nv_src)
        return hipErrorInvalidValue;
    if ((a.old_n && !a.old_list) || (a.n_log && (!a.flog || !a.new_list))) return hipErrorInvalidValue;
    hipError_t st = hipMemsetAsync(a.new_n, 0, sizeof(uint32_t), s);
    if (st != hipSuccess) return st;
    const uint64_t n = (uint64_t)a.old_n + (a.n_log - a.seen);
    const uint32_t blocks = n ? (uint32_t)((n + kStateThreads - 1u) / kStateThreads) : 1u;  // (workgroup 0 writes nv_out)
    hipLaunchKernelGGL(dt_stream_foreign_kernel, dim3(blocks), dim3(kStateThreads), 0, s, a);
    return hipGetLastError();
}

// the TRADE summaries: end = finish of every placed job, physical or virtual node (a DELAY run has no
// borrowed job); an undecided job keeps its batch alive for good
hipError_t launch_dt_series_summary(const DtSeriesArgs& a, hipStream_t s) {
    if (a.d.s.n_clusters == 0) return hipSuccess;
    SeriesArgs p{};
    p.s = a.d.s;
    p.summ = a.summ;
    if (p.s.job_cnt)
        hipLaunchKernelGGL((series_summary_kernel<true, true>), dim3(a.d.s.n_clusters), dim3(kStateThreads), 0, s, p);
    else
        hipLaunchKernelGGL(series_summary_kernel<true>, dim3(a.d.s.n_clusters), dim3(kStateThreads), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_dt_state_series(const DtSeriesArgs& a, uint32_t max_nn, hipStream_t s) {
    if (a.d.s.n_clusters == 0) return hipSuccess;
    // dt_series_tile(NN) samples of dt_series_bytes(NN) bytes, NN <= max_nn, within kSeriesLds
    if (max_nn == 0 || max_nn > 1280u) return hipErrorInvalidValue;  // a tile of at least 3 samples
    uint32_t lds = dt_series_bytes(max_nn) * kSeriesMaxTile;
    if (lds > kSeriesLds) lds = kSeriesLds;
    if (!a.d.s.job_cnt && (a.live || a.live_n)) return hipErrorInvalidValue;  // the list is a session's
    const void* fn = a.d.s.job_cnt ? reinterpret_cast<const void*>(dt_series_kernel<true>)
                                   : reinterpret_cast<const void*>(dt_series_kernel<false>);
    hipError_t st = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kSeriesLds);
    if (st != hipSuccess) return st;
    if (a.d.s.job_cnt)
        hipLaunchKernelGGL(dt_series_kernel<true>, dim3(a.d.s.n_clusters), dim3(kStateThreads), lds, s, a);
    else
        hipLaunchKernelGGL(dt_series_kernel<false>, dim3(a.d.s.n_clusters), dim3(kStateThreads), lds, s, a);
    return hipGetLastError();
}

hipError_t launch_state(const StateArgs& a, uint32_t max_n, hipStream_t s) {
    if (a.n_clusters == 0) return hipSuccess;
    if (a.job_cnt && a.lent_off) return hipErrorInvalidValue;  // no trading in an online session
    if (a.job_cnt)
        hipLaunchKernelGGL((state_kernel<false, true>), dim3(a.n_clusters), dim3(kStateThreads), 2 * max_n * sizeof(uint32_t), s, a);
    else if (a.lent_off)
        hipLaunchKernelGGL(state_kernel<true>, dim3(a.n_clusters), dim3(kStateThreads), 2 * max_n * sizeof(uint32_t), s, a);
    else
        hipLaunchKernelGGL(state_kernel<false>, dim3(a.n_clusters), dim3(kStateThreads), 2 * max_n * sizeof(uint32_t), s, a);
    return hipGetLastError();
}

}  // namespace mcs
