// mcs_stream.cpp — host side of the start-stream cursor (mcs_stream_open / next / close; kernels in
// mcs_stream.hip).  Host code; compiled by hipcc.
//
// The engine owns the kept arrays: per batch of kSeriesBatch rows a flag word, the summary pair and the
// sum of s - a (indexed as the series summaries are: by segment start, over segment capacity), per row
// the wait record (a stream with wait statistics or with Level1), per cluster a StreamCluster; a stream
// opened with Level1 (mcs_stream_open_level1) adds per batch the Level1 summary and per cluster the
// carried scan bounds.  They are freed when the stream closes and at destroy, and follow the segments
// through a relayout (stream_relayout).
// A trading session's cursor (mcs_trade_stream_open / next / close, mcs_trade.h) shares all of it, since
// plain and trading sessions exclude each other, and adds the two Foreign lists, the log position and
// the row counts of the current call; its frontier F* and its hooks in dtrade_session_run are below.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "mcs_engine_impl.h"
#include "mcs_internal.h"

namespace mcs {

void stream_free(mcs_engine* e) {
    dfree(e->d_st_cl);
    dfree(e->d_st_flags);
    dfree(e->d_st_summ);
    dfree(e->d_st_bsum);
    dfree(e->d_st_rec);
    dfree(e->d_st_tot);
    dfree(e->d_st_out);
    dfree(e->d_st_wout);
    dfree(e->d_st_fl[0]);
    dfree(e->d_st_fl[1]);
    dfree(e->d_st_fl_n);
    dfree(e->d_st_nv);
    dfree(e->d_st_l1s);
    dfree(e->d_st_l1c);
    dfree(e->d_st_l1out);
    dfree(e->d_st_l1rows);
    for (hipEvent_t& ev : e->st_l1ev) {
        if (ev) (void)hipEventDestroy(ev);
        ev = nullptr;
    }
    e->st_l1 = e->st_l1_fresh = false;
    e->st_fl_cap = e->st_fl_n = e->st_seen = 0;
    e->st_out_cap = 0;
    e->st_open = false;
}

namespace {

// the kept arrays for the segment layout `off` (capacity off[C]); the flags start at 0: nothing known
int stream_alloc(mcs_engine* e, const std::vector<uint64_t>& off, uint32_t** flags, uint2** summ,
                 unsigned long long** bsum, uint4** rec, uint32_t** l1s) {
    const size_t nbat = series_summ_size(off[e->C], e->C);
    HIPCHK(e, hipMalloc(flags, nbat * sizeof(uint32_t)));
    HIPCHK(e, hipMemsetAsync(*flags, 0, nbat * sizeof(uint32_t), e->stream));
    HIPCHK(e, hipMalloc(summ, nbat * sizeof(uint2)));
    HIPCHK(e, hipMalloc(bsum, nbat * sizeof(unsigned long long)));
    // the records serve the wait statistics and Level1 alike
    if (e->st_wait || e->st_l1) HIPCHK(e, hipMalloc(rec, (size_t)(off[e->C] ? off[e->C] : 1) * sizeof(uint4)));
    if (e->st_l1) HIPCHK(e, hipMalloc(l1s, nbat * sizeof(uint32_t)));
    return MCS_OK;
}

}  // namespace

int stream_reset_kept(mcs_engine* e) {
    const size_t C = e->C ? e->C : 1;
    const size_t nbat = series_summ_size(e->job_off[e->C], e->C);
    HIPCHK(e, hipStreamSynchronize(e->stream));
    HIPCHK(e, hipMemset(e->d_st_flags, 0, nbat * sizeof(uint32_t)));
    HIPCHK(e, hipMemset(e->d_st_tot, 0, 2 * sizeof(unsigned long long)));
    std::vector<StreamCluster> cl(C, StreamCluster{-1, 0ull, 0u, 0u});
    HIPCHK(e, hipMemcpy(e->d_st_cl, cl.data(), C * sizeof(StreamCluster), hipMemcpyHostToDevice));
    e->st_retired = 0;
    if (e->st_l1) {  // the carried bounds are dropped with the rest
        HIPCHK(e, hipMemset(e->d_st_l1c, 0, C * sizeof(uint2)));
        e->st_l1_fresh = true;
    }
    return MCS_OK;
}

int stream_alloc_kept(mcs_engine* e, const char* call) {
    int rc = stream_alloc(e, e->job_off, &e->d_st_flags, &e->d_st_summ, &e->d_st_bsum, &e->d_st_rec, &e->d_st_l1s);
    const size_t C = e->C ? e->C : 1;
    hipError_t st = hipSuccess;
    if (rc == MCS_OK) st = hipMalloc(&e->d_st_cl, C * sizeof(StreamCluster));
    if (rc == MCS_OK && st == hipSuccess) st = hipMalloc(&e->d_st_tot, 2 * sizeof(unsigned long long));
    if (rc == MCS_OK && st == hipSuccess && e->st_l1) {
        st = hipMalloc(&e->d_st_l1c, C * sizeof(uint2));
        if (st == hipSuccess) st = hipMalloc(&e->d_st_l1rows, sizeof(unsigned long long));
        for (hipEvent_t& ev : e->st_l1ev)
            if (st == hipSuccess) st = hipEventCreate(&ev);
    }
    if (rc == MCS_OK && st != hipSuccess) rc = fail(e, MCS_E_HIP, std::string(call) + ": " + hipGetErrorString(st));
    if (rc == MCS_OK) rc = stream_reset_kept(e);
    if (rc != MCS_OK) stream_free(e);
    return rc;
}

void stream_shut(mcs_engine* e, const char* cause) {
    if (!e->st_open) return;
    (void)hipStreamSynchronize(e->stream);
    stream_free(e);
    e->st_cause = cause;
}

void stream_run_begin(mcs_engine* e, uint32_t t_hor) {
    if (t_hor != MCS_TIME_NONE && t_hor < e->on_t_done) return;  // online_run refuses it: nothing runs
    if (e->st_open && e->st_drained)
        stream_shut(e, "an mcs_run after a drain (samples at or past the last finite horizon were not final)");
}

void stream_run_end(mcs_engine* e, uint32_t t_hor, int status) {
    if (status == MCS_E_INVALID) return;  // a refused argument (a decreasing horizon): nothing ran
    e->on_run_failed = status != MCS_OK;
    if (!e->st_open) return;
    if (status != MCS_OK)
        stream_shut(e, "an mcs_run that failed");
    else if (t_hor == MCS_TIME_NONE)
        e->st_drained = true;  // the frontier stays at the last finite horizon
    else
        e->st_h = t_hor;
}

// ---- a trading session's stream: the frontier F* and the replay --------------------
//
// The lock-step clock is common to all clusters and appended arrivals lie above the last executed tick,
// so a drain that ends at tick T_d decides exactly as mcs_run(T_d + 1) would: F* is the largest of the
// session's finite horizons and, where a tick has been executed, t_last + 1.  It never decreases.
static uint32_t trade_frontier(const mcs_engine* e) {
    if (!e->has_run) return 0u;
    return std::max(e->on_t_hor, e->ts_ticks_total ? e->ts_t_last + 1u : 0u);
}

void trade_stream_restart(mcs_engine* e) {
    if (!e->st_open || !e->st_trade) return;
    // nothing is proved about the kept state across a replay: it is dropped and rebuilt once
    if (stream_reset_kept(e) != MCS_OK) {
        const std::string msg = e->err;
        stream_shut(e, "a replay of the session whose reset of the kept state failed");
        e->err = msg;
        return;
    }
    e->st_seen = 0;
    e->st_fl_n = 0;
    e->st_rebuild = true;
}

void trade_stream_run_end(mcs_engine* e, uint32_t t_hor, int status) {
    (void)t_hor;
    e->on_run_failed = status != MCS_OK;
    if (!e->st_open || !e->st_trade) return;
    if (status != MCS_OK) {
        stream_shut(e, "an mcs_run that failed");
        return;
    }
    DtStreamView v{};
    if (!dtrade_stream_view(e, &v)) return;
    // (a slot-pool or virtual-node overflow never ends a run well: dtrade_session_run escalates and replays,
    // or fails with MCS_E_CAPACITY, which the branch above closes on)
    if ((v.flags & MCS_FLAG_LOG_OVERFLOW) || v.n_foreign > v.foreign_cap || v.n_trades > v.trade_cap) {
        stream_shut(e, "an mcs_run whose Foreign or contract log overflowed (MCS_FLAG_LOG_OVERFLOW): records "
                       "were dropped");
        return;
    }
    e->st_h = std::max(e->st_h, trade_frontier(e));
}

int stream_relayout(mcs_engine* e, const uint64_t* d_old_off, const uint64_t* d_new_off,
                    const std::vector<uint64_t>& new_off) {
    if (!e->st_open) return MCS_OK;
    uint32_t* flags = nullptr;
    uint2* summ = nullptr;
    unsigned long long* bsum = nullptr;
    uint4* rec = nullptr;
    uint32_t* l1s = nullptr;
    int rc = stream_alloc(e, new_off, &flags, &summ, &bsum, &rec, &l1s);
    if (rc == MCS_OK) {
        StreamMoveArgs m{};
        m.old_off = d_old_off;
        m.new_off = d_new_off;
        m.job_cnt = e->d_job_cnt;
        m.flags_o = e->d_st_flags;
        m.flags_n = flags;
        m.summ_o = e->d_st_summ;
        m.summ_n = summ;
        m.bsum_o = e->d_st_bsum;
        m.bsum_n = bsum;
        m.rec_o = e->d_st_rec;
        m.rec_n = rec;
        m.l1s_o = e->d_st_l1s;
        m.l1s_n = l1s;
        m.n_clusters = e->C;
        hipError_t st = launch_stream_move(m, e->stream);
        if (st == hipSuccess) st = hipStreamSynchronize(e->stream);
        if (st != hipSuccess) rc = fail(e, MCS_E_HIP, std::string("stream relayout: ") + hipGetErrorString(st));
    }
    if (rc != MCS_OK) {
        dfree(flags);
        dfree(summ);
        dfree(bsum);
        dfree(rec);
        dfree(l1s);
        const std::string msg = e->err;
        stream_shut(e, "a segment relayout that failed");
        e->err = msg;
        return rc;
    }
    dfree(e->d_st_flags);
    dfree(e->d_st_summ);
    dfree(e->d_st_bsum);
    dfree(e->d_st_rec);
    dfree(e->d_st_l1s);
    e->d_st_l1s = l1s;
    e->d_st_flags = flags;
    e->d_st_summ = summ;
    e->d_st_bsum = bsum;
    e->d_st_rec = rec;
    return MCS_OK;
}

}  // namespace mcs

// mcs_stream_open and mcs_stream_open_level1 behind check_engine
static int stream_open_impl(mcs_engine* e, uint32_t t0_s, uint32_t period_s, uint32_t with_wait, bool level1) {
    if (int st = mcs::refuse_trade_session(e, "mcs_stream_open")) return st;
    if (!e->online)
        return fail(e, MCS_E_STATE, "mcs_stream_open subscribes to an online session (mcs_run with a horizon, "
                                    "mcs_append_jobs; FIFO or DELAY without trading)");
    if (e->st_open) return fail(e, MCS_E_STATE, "a stream is open already: one stream per engine (mcs_stream_close)");
    if (e->on_run_failed)
        return fail(e, MCS_E_STATE, "the session's last mcs_run failed: its rows are not a decided prefix (mcs_rewind)");
    if (period_s == 0) return fail(e, MCS_E_INVALID, "period_s must be positive");
    if (with_wait && e->cfg.policy != MCS_POLICY_DELAY)
        return fail(e, MCS_E_INVALID, "the wait statistics need a DELAY session: only \"/delay\" feeds WaitTime");
    if (level1 && e->cfg.policy != MCS_POLICY_DELAY)
        return fail(e, MCS_E_INVALID, "Level1 samples need a DELAY session: Scheduler.Fifo has no Level1");
    HIPCHK(e, hipStreamSynchronize(e->stream));
    e->st_wait = with_wait != 0;
    e->st_l1 = level1;
    e->st_cause.clear();
    e->st_trade = false;
    if (int rc = mcs::stream_alloc_kept(e, "mcs_stream_open")) return rc;
    e->st_open = true;
    e->st_period = period_s;
    e->st_next = t0_s;
    e->st_h = e->has_run ? e->on_t_hor : 0u;  // the last finite horizon of the session (0: none yet)
    e->st_drained = e->has_run && e->on_series_hor == MCS_TIME_NONE;  // the last run was a drain
    e->st_retired = 0;
    return MCS_OK;
}

extern "C" {

int mcs_stream_open(mcs_engine* e, uint32_t t0_s, uint32_t period_s, uint32_t with_wait) {
    if (int st = check_engine(e)) return st;
    return stream_open_impl(e, t0_s, period_s, with_wait, false);
}

int mcs_stream_open_level1(mcs_engine* e, uint32_t t0_s, uint32_t period_s, uint32_t with_wait) {
    if (int st = check_engine(e)) return st;
    return stream_open_impl(e, t0_s, period_s, with_wait, true);
}

}  // extern "C"

// The body of mcs_stream_next and mcs_trade_stream_next behind their state checks.  A trading session's
// call differs in three places: the Foreign take before the prep kernel, dt_series_kernel over the kept
// summaries and the kept Foreign list in place of series_kernel, and the TRADE instantiations of the prep
// and the retire kernel (StreamArgs::nv).
static int stream_next_impl(mcs_engine* e, bool trade, uint32_t max_samples, mcs_cluster_sample* out,
                            mcs_wait_sample* wait, mcs_level1_sample* level1, uint32_t n_clusters,
                            mcs_trade_stream_stats* stats, mcs_level1_stream_stats* l1stats) {
    const std::string call = trade ? "mcs_trade_stream_next" : "mcs_stream_next";
    if (n_clusters != e->C)
        return fail(e, MCS_E_INVALID, "n_clusters must equal mcs_num_clusters: the frontier is common to all clusters");
    if (!out || max_samples == 0) return fail(e, MCS_E_INVALID, "bad output");
    if ((wait != nullptr) != e->st_wait)
        return fail(e, MCS_E_INVALID, "wait must be given exactly when the stream was opened with_wait");
    if ((level1 != nullptr) != e->st_l1)
        return fail(e, MCS_E_INVALID, "level1 must be given exactly when the stream was opened with Level1 "
                                      "(mcs_stream_open_level1, mcs_trade_stream_open_level1; their next calls)");
    const uint32_t period = e->st_period, t0 = e->st_next, h = e->st_h;
    const uint64_t decided = t0 < h ? ((uint64_t)(h - t0) + period - 1) / period : 0ull;  // samples below h
    const uint32_t n = (uint32_t)std::min<uint64_t>(decided, max_samples);
    // the next sample second; past the uint32 range no second is ever decided: the stream rests there
    const uint32_t t_after = (uint32_t)std::min<uint64_t>(t0 + (uint64_t)n * period, 0xFFFFFFFFull);
    if (stats) {
        stats->n_written = n;
        stats->t_first = t0;
        stats->t_next = t_after;
        stats->pending = (uint32_t)std::min<uint64_t>(decided - n, 0xFFFFFFFFull);
        stats->rows_retired = e->st_retired;
    }
    if (n == 0 || n_clusters == 0) {
        e->st_next = t_after;
        return MCS_OK;
    }
    if (e->st_wait || e->st_l1)
        for (uint32_t c = 0; c < e->C; ++c)  // job indices within a cluster are 32-bit on the device
            if (e->job_cnt[c] > 0xFFFFFFFEull) return fail(e, MCS_E_INVALID, "a cluster holds more than 2^32 - 2 jobs");
    if (int st = mcs::ensure_job_records(e)) return st;
    // samples per launch: the device buffers stay within 256 MiB (MCS_SERIES_CHUNK overrides the count)
    uint64_t chunk = (256ull << 20) / ((sizeof(mcs_cluster_sample) + sizeof(mcs_wait_sample) +
                                        (e->st_l1 ? sizeof(mcs_level1_sample) : 0)) * (uint64_t)n_clusters);
    if (const char* env = getenv("MCS_SERIES_CHUNK"))
        if (atoll(env) > 0) chunk = (uint64_t)atoll(env);
    if (chunk < 1) chunk = 1;
    if (chunk > n) chunk = n;
    if (e->st_out_cap < chunk) {
        dfree(e->d_st_out);
        dfree(e->d_st_wout);
        dfree(e->d_st_l1out);
        e->st_out_cap = 0;
        const uint64_t cap = std::max<uint64_t>(chunk, 16);
        HIPCHK(e, hipMalloc(&e->d_st_out, (size_t)n_clusters * cap * sizeof(mcs_cluster_sample)));
        if (e->st_wait) HIPCHK(e, hipMalloc(&e->d_st_wout, (size_t)n_clusters * cap * sizeof(mcs_wait_sample)));
        if (e->st_l1) HIPCHK(e, hipMalloc(&e->d_st_l1out, (size_t)n_clusters * cap * sizeof(mcs_level1_sample)));
        e->st_out_cap = cap;
    }
    mcs::DtStreamView v{};
    mcs::DtStreamForeignArgs fa{};
    uint32_t n_log = 0;
    const bool rebuilt = trade && e->st_rebuild;
    if (trade) {
        if (!mcs::dtrade_stream_view(e, &v))
            return fail(e, MCS_E_STATE, call + ": the trading session holds no lock-step state (mcs_run first)");
        if (v.n_foreign > 0xFFFFFFFEull) return fail(e, MCS_E_INVALID, "more than 2^32 - 2 Foreign jobs");
        n_log = (uint32_t)std::min<uint64_t>(v.n_foreign, v.foreign_cap);
        if (!e->d_st_nv) HIPCHK(e, hipMalloc(&e->d_st_nv, (size_t)n_clusters * sizeof(uint32_t)));
        if (!e->d_st_fl_n) HIPCHK(e, hipMalloc(&e->d_st_fl_n, sizeof(uint32_t)));
        if (e->st_fl_cap < n_log || !e->d_st_fl[0]) {  // both lists hold the log as it stands: no overflow
            const uint64_t cap = std::min<uint64_t>(std::max<uint64_t>(2ull * n_log, 1024), std::max<uint64_t>(v.foreign_cap, 1));
            mcs_foreign_rec* nl[2] = {nullptr, nullptr};
            hipError_t gs = hipMalloc(&nl[0], (size_t)cap * sizeof(mcs_foreign_rec));
            if (gs == hipSuccess) gs = hipMalloc(&nl[1], (size_t)cap * sizeof(mcs_foreign_rec));
            if (gs == hipSuccess && e->st_fl_n)  // the kept list moves to the larger buffer
                gs = hipMemcpy(nl[0], e->d_st_fl[e->st_fl_cur], (size_t)e->st_fl_n * sizeof(mcs_foreign_rec),
                               hipMemcpyDeviceToDevice);
            if (gs != hipSuccess) {  // (the stream stays as it was: the kept list is untouched)
                dfree(nl[0]);
                dfree(nl[1]);
                return fail(e, MCS_E_HIP, call + ": growing the Foreign lists: " + hipGetErrorString(gs));
            }
            dfree(e->d_st_fl[0]);
            dfree(e->d_st_fl[1]);
            e->d_st_fl[0] = nl[0];
            e->d_st_fl[1] = nl[1];
            e->st_fl_cur = 0;
            e->st_fl_cap = (uint32_t)cap;
        }
        fa.flog = v.flog;
        fa.old_list = e->d_st_fl[e->st_fl_cur];
        fa.new_list = e->d_st_fl[e->st_fl_cur ^ 1];
        fa.new_n = e->d_st_fl_n;
        fa.old_n = e->st_fl_n;
        fa.seen = e->st_seen;
        fa.n_log = n_log;
        fa.t_first = t0;
        fa.cap = e->st_fl_cap;
        fa.nv_src = v.nv_src;
        fa.nv_stride = v.nv_stride;
        fa.V = v.V;
        fa.n_clusters = n_clusters;
        fa.nv_out = e->d_st_nv;
    }
    mcs::TradeStreamArgs a{};  // (a plain session's launches take its StreamArgs part)
    a.nv = trade ? e->d_st_nv : nullptr;
    a.s.node_off = e->d_node_off;
    a.s.cap = e->d_cap;
    a.s.free0 = e->d_free0;
    a.s.jobs = e->d_jobs;
    a.s.job_off = e->d_job_off;
    a.s.out_node = e->d_out_node;
    a.s.out_start = e->d_out_start;
    a.s.out_finish = e->d_out_finish;
    a.s.n_clusters = n_clusters;
    a.s.job_cnt = e->d_job_cnt;
    a.cl = e->d_st_cl;
    a.flags = e->d_st_flags;
    a.summ = e->d_st_summ;
    a.bsum = e->d_st_bsum;
    a.rec = e->d_st_rec;
    a.wout = e->d_st_wout;
    a.tot = e->d_st_tot;
    a.hor = h;
    a.max_wait = e->cfg.max_wait_s;
    a.period = period;
    a.chunk = (uint32_t)chunk;
    a.frontier = t_after;
    mcs::SeriesArgs sa{};
    sa.s = a.s;
    sa.summ = e->d_st_summ;
    sa.out = e->d_st_out;
    sa.period = period;
    sa.magic = period > 1 ? ~0ull / period + 1ull : 0ull;
    mcs::DtSeriesArgs da{};
    uint32_t max_nn = 1;
    if (trade) {
        da.d.s = a.s;
        da.d.vcap = v.vcap;
        da.d.nv = e->d_st_nv;
        da.d.flog = v.flog;
        da.d.n_foreign = n_log;  // bounds the list's length as the kernel reads it
        da.d.V = v.V;
        da.summ = e->d_st_summ;
        da.out = e->d_st_out;
        da.period = period;
        da.magic = sa.magic;
        da.live = fa.new_list;
        da.live_n = e->d_st_fl_n;
        // the LDS a launch asks for: the widest cluster the session can hold (the kernel cuts its tiles
        // by the rows the device's nv gives, which need no more)
        max_nn = std::min<uint32_t>(std::max<uint32_t>(e->max_n, 1u) + v.V, 1280u);
    }
    mcs::WaitArgs wa{};
    wa.jobs = e->d_jobs;
    wa.job_off = e->d_job_off;
    wa.job_cnt = e->d_job_cnt;
    wa.out_node = e->d_out_node;
    wa.out_start = e->d_out_start;
    wa.rec = e->d_st_rec;
    wa.out = e->d_st_wout;
    wa.max_wait = e->cfg.max_wait_s;
    wa.period = period;
    wa.n_clusters = n_clusters;
    mcs::StreamLevel1Args la{};
    la.jobs = e->d_jobs;
    la.job_off = e->d_job_off;
    la.job_cnt = e->d_job_cnt;
    la.cl = e->d_st_cl;
    la.flags = e->d_st_flags;
    la.rec = e->d_st_rec;
    la.l1s = e->d_st_l1s;
    la.carry = e->d_st_l1c;
    la.out = e->d_st_l1out;
    la.rows = e->d_st_l1rows;
    la.period = period;
    la.n_clusters = n_clusters;
    double total_ms = 0.0, l1_ms = 0.0;
    unsigned long long tot[2] = {0ull, 0ull}, l1_rows = 0ull;
    hipError_t st = hipMemsetAsync(e->d_st_tot, 0, sizeof(unsigned long long), e->stream);  // [0]: this call's rows
    if (st == hipSuccess && e->st_l1) st = hipMemsetAsync(e->d_st_l1rows, 0, sizeof(unsigned long long), e->stream);
    for (uint64_t k0 = 0; st == hipSuccess && k0 < n; k0 += chunk) {
        const uint32_t nk = (uint32_t)(n - k0 < chunk ? n - k0 : chunk);
        const bool last = k0 + nk == n;
        a.t0 = sa.t0 = wa.t0 = da.t0 = (uint32_t)(t0 + k0 * period);
        a.n_samples = sa.n_samples = wa.n_samples = da.n_samples = nk;
        st = hipEventRecord(e->ev0, e->stream);
        if (st == hipSuccess && k0 == 0 && trade) st = mcs::launch_dt_stream_foreign(fa, e->stream);
        if (st == hipSuccess && k0 == 0)
            st = trade ? mcs::launch_trade_stream_prep(a, e->stream) : mcs::launch_stream_prep(a, e->stream);
        if (st == hipSuccess && trade) st = mcs::launch_dt_state_series(da, max_nn, e->stream);
        if (st == hipSuccess && !trade) st = mcs::launch_state_series(sa, e->max_n ? e->max_n : 1, e->stream);
        if (st == hipSuccess && e->st_wait) {
            st = hipMemsetAsync(e->d_st_wout, 0, (size_t)n_clusters * nk * sizeof(mcs_wait_sample), e->stream);
            if (st == hipSuccess) st = mcs::launch_stream_accum(a, e->stream);
            if (st == hipSuccess) st = mcs::launch_wait_finish(wa, e->stream);
        }
        if (st == hipSuccess && e->st_l1) {  // before the retire kernel: first_live is the last call's
            la.t0 = a.t0;
            la.n_samples = nk;
            la.fresh = e->st_l1_fresh && k0 == 0 ? 1u : 0u;
            st = hipEventRecord(e->st_l1ev[0], e->stream);
            if (st == hipSuccess && k0 == 0) st = mcs::launch_stream_level1_summ(la, e->stream);
            if (st == hipSuccess) st = mcs::launch_stream_level1(la, e->stream);
            if (st == hipSuccess) st = hipEventRecord(e->st_l1ev[1], e->stream);
        }
        if (st == hipSuccess && last) {  // the whole call's samples against the new frontier
            mcs::TradeStreamArgs ra = a;
            ra.t0 = t0;
            ra.n_samples = n;
            if (!e->st_wait) ra.rec = nullptr;  // records kept for Level1 alone: no accum kernel loaded them
            st = trade ? mcs::launch_trade_stream_retire(ra, e->stream) : mcs::launch_stream_retire(ra, e->stream);
        }
        if (st == hipSuccess) st = hipEventRecord(e->ev1, e->stream);
        if (st == hipSuccess) st = hipStreamSynchronize(e->stream);
        float ms = 0.0f;
        if (st == hipSuccess) st = hipEventElapsedTime(&ms, e->ev0, e->ev1);
        total_ms += ms;
        if (st == hipSuccess && e->st_l1) {
            st = hipEventElapsedTime(&ms, e->st_l1ev[0], e->st_l1ev[1]);
            l1_ms += ms;
            if (st == hipSuccess)
                st = hipMemcpy2D(level1 + k0, (size_t)max_samples * sizeof(mcs_level1_sample), e->d_st_l1out,
                                 (size_t)nk * sizeof(mcs_level1_sample), (size_t)nk * sizeof(mcs_level1_sample),
                                 n_clusters, hipMemcpyDeviceToHost);
        }
        if (st == hipSuccess)  // the chunk's columns of every cluster's row
            st = hipMemcpy2D(out + k0, (size_t)max_samples * sizeof(mcs_cluster_sample), e->d_st_out,
                             (size_t)nk * sizeof(mcs_cluster_sample), (size_t)nk * sizeof(mcs_cluster_sample),
                             n_clusters, hipMemcpyDeviceToHost);
        if (st == hipSuccess && e->st_wait)
            st = hipMemcpy2D(wait + k0, (size_t)max_samples * sizeof(mcs_wait_sample), e->d_st_wout,
                             (size_t)nk * sizeof(mcs_wait_sample), (size_t)nk * sizeof(mcs_wait_sample), n_clusters,
                             hipMemcpyDeviceToHost);
    }
    if (st == hipSuccess) st = hipMemcpy(tot, e->d_st_tot, sizeof(tot), hipMemcpyDeviceToHost);
    if (st == hipSuccess && e->st_l1) st = hipMemcpy(&l1_rows, e->d_st_l1rows, sizeof(l1_rows), hipMemcpyDeviceToHost);
    uint32_t fl_n = 0;
    if (st == hipSuccess && trade) st = hipMemcpy(&fl_n, e->d_st_fl_n, sizeof(fl_n), hipMemcpyDeviceToHost);
    if (st != hipSuccess) {
        const int rc = fail(e, MCS_E_HIP, call + ": " + hipGetErrorString(st));
        const std::string msg = e->err;
        mcs::stream_shut(e, trade ? "a device error in mcs_trade_stream_next" : "a device error in mcs_stream_next");
        e->err = msg;
        return rc;
    }
    e->st_next = a.frontier;
    e->st_retired = tot[1];
    e->st_l1_fresh = false;  // the carried bounds are those of this call's last sample
    if (l1stats) {
        l1stats->rows_scanned = l1_rows;
        l1stats->kernel_ms = l1_ms;
    }
    if (trade) {  // the new list is the kept one; the log is taken up to n_log
        e->st_fl_cur ^= 1;
        e->st_fl_n = std::min(fl_n, e->st_fl_cap);
        e->st_rebuild = false;
        if (stats) {
            stats->foreign_scanned = n_log - e->st_seen;
            stats->foreign_live = e->st_fl_n;
            stats->rebuilt = rebuilt ? 1u : 0u;
        }
        e->st_seen = n_log;
    }
    if (stats) {
        stats->rows_scanned = tot[0];
        stats->rows_retired = tot[1];
        stats->kernel_ms = total_ms;
    }
    return MCS_OK;
}

extern "C" {

int mcs_stream_next(mcs_engine* e, uint32_t max_samples, mcs_cluster_sample* out, mcs_wait_sample* wait,
                    uint32_t n_clusters, mcs_stream_stats* stats) {
    return mcs_stream_next_level1(e, max_samples, out, wait, nullptr, n_clusters, stats, nullptr);
}

int mcs_stream_next_level1(mcs_engine* e, uint32_t max_samples, mcs_cluster_sample* out, mcs_wait_sample* wait,
                           mcs_level1_sample* level1, uint32_t n_clusters, mcs_stream_stats* stats,
                           mcs_level1_stream_stats* l1stats) {
    if (int st = check_engine(e)) return st;
    if (stats) *stats = mcs_stream_stats{};
    if (l1stats) *l1stats = mcs_level1_stream_stats{};
    if (e->st_trade && (e->st_open || !e->st_cause.empty()))
        return fail(e, MCS_E_STATE, "the engine's stream is a trading session's (mcs_trade_stream_next, "
                                    "mcs_trade_stream_close)");
    if (!e->st_open) {
        if (e->st_cause.empty()) return fail(e, MCS_E_STATE, "no stream is open (mcs_stream_open)");
        return fail(e, MCS_E_STATE, "the stream was closed by " + e->st_cause + ": reopen it (mcs_stream_open)");
    }
    mcs_trade_stream_stats ts{};
    const int rc = stream_next_impl(e, false, max_samples, out, wait, level1, n_clusters, &ts, l1stats);
    if (stats) {
        stats->n_written = ts.n_written;
        stats->t_first = ts.t_first;
        stats->t_next = ts.t_next;
        stats->pending = ts.pending;
        stats->rows_scanned = ts.rows_scanned;
        stats->rows_retired = ts.rows_retired;
        stats->kernel_ms = ts.kernel_ms;
    }
    return rc;
}

int mcs_stream_close(mcs_engine* e) {
    if (int st = check_engine(e)) return st;
    if (e->st_trade && (e->st_open || !e->st_cause.empty()))
        return fail(e, MCS_E_STATE, "the engine's stream is a trading session's (mcs_trade_stream_close)");
    if (!e->st_open) {
        if (e->st_cause.empty()) return fail(e, MCS_E_STATE, "no stream is open");
        e->st_cause.clear();  // closed by the engine already: acknowledged
        return MCS_OK;
    }
    mcs::stream_shut(e, "mcs_stream_close");
    e->st_cause.clear();
    return MCS_OK;
}

// ---- the cursor of a trading session (mcs_trade.h) ----------------------------------

static int no_trade_session(mcs_engine* e, const char* call) {
    return fail(e, MCS_E_STATE, std::string(call) + " subscribes to a trading session (online mode with "
                                    "MCS_POLICY_DELAY and cfg.trader: mcs_run with a horizon, mcs_append_jobs); "
                                    "there is no trading session (in a session without trading: mcs_stream_open)");
}

static int trade_stream_open_impl(mcs_engine* e, uint32_t t0_s, uint32_t period_s, uint32_t with_wait, bool level1) {
    if (!mcs::is_trade_session(e)) return no_trade_session(e, "mcs_trade_stream_open");
    if (e->st_open)
        return fail(e, MCS_E_STATE, "a stream is open already: one stream per engine (mcs_trade_stream_close)");
    if (e->ts_failed)
        return fail(e, MCS_E_STATE, "mcs_trade_stream_open: the trading session failed (capacity exhausted, "
                                    "MCS_E_CAPACITY): mcs_rewind or submit again, then run");
    if (e->on_run_failed)
        return fail(e, MCS_E_STATE, "the session's last mcs_run failed: its rows are not a decided prefix (mcs_rewind)");
    mcs::DtStreamView v{};
    if (e->has_run && mcs::dtrade_stream_view(e, &v)) {  // the cases in which the series call refuses
        if (v.flags & (MCS_FLAG_OVERFLOW | MCS_FLAG_VNODE_OVERFLOW))
            return fail(e, MCS_E_STATE, "mcs_trade_stream_open: the session's last run was cut short by a slot-pool "
                                        "or virtual-node overflow (MCS_FLAG_VNODE_OVERFLOW)");
        if ((v.flags & MCS_FLAG_LOG_OVERFLOW) || v.n_foreign > v.foreign_cap || v.n_trades > v.trade_cap)
            return fail(e, MCS_E_STATE, "mcs_trade_stream_open: the session's Foreign or contract log overflowed "
                                        "(MCS_FLAG_LOG_OVERFLOW): records were dropped");
    }
    if (period_s == 0) return fail(e, MCS_E_INVALID, "period_s must be positive");
    HIPCHK(e, hipStreamSynchronize(e->stream));
    e->st_wait = with_wait != 0;
    e->st_l1 = level1;  // (a trading session is a DELAY session: it has Level1)
    e->st_cause.clear();
    e->st_trade = true;
    if (int rc = mcs::stream_alloc_kept(e, "mcs_trade_stream_open")) return rc;
    e->st_open = true;
    e->st_period = period_s;
    e->st_next = t0_s;
    e->st_h = mcs::trade_frontier(e);
    e->st_drained = false;
    e->st_retired = 0;
    e->st_seen = e->st_fl_n = 0;
    e->st_fl_cur = 0;
    e->st_rebuild = true;  // the first call that writes samples builds the kept state
    return MCS_OK;
}

int mcs_trade_stream_open(mcs_engine* e, uint32_t t0_s, uint32_t period_s, uint32_t with_wait) {
    if (int st = check_engine(e)) return st;
    return trade_stream_open_impl(e, t0_s, period_s, with_wait, false);
}

int mcs_trade_stream_open_level1(mcs_engine* e, uint32_t t0_s, uint32_t period_s, uint32_t with_wait) {
    if (int st = check_engine(e)) return st;
    return trade_stream_open_impl(e, t0_s, period_s, with_wait, true);
}

int mcs_trade_stream_next(mcs_engine* e, uint32_t max_samples, mcs_cluster_sample* out, mcs_wait_sample* wait,
                          uint32_t n_clusters, mcs_trade_stream_stats* stats) {
    return mcs_trade_stream_next_level1(e, max_samples, out, wait, nullptr, n_clusters, stats, nullptr);
}

int mcs_trade_stream_next_level1(mcs_engine* e, uint32_t max_samples, mcs_cluster_sample* out, mcs_wait_sample* wait,
                                 mcs_level1_sample* level1, uint32_t n_clusters, mcs_trade_stream_stats* stats,
                                 mcs_level1_stream_stats* l1stats) {
    if (int st = check_engine(e)) return st;
    if (stats) *stats = mcs_trade_stream_stats{};
    if (l1stats) *l1stats = mcs_level1_stream_stats{};
    if (!mcs::is_trade_session(e) && !(e->st_trade && !e->st_cause.empty()))
        return no_trade_session(e, "mcs_trade_stream_next");
    if (!e->st_open || !e->st_trade) {
        if (e->st_cause.empty() || !e->st_trade)
            return fail(e, MCS_E_STATE, "no stream is open (mcs_trade_stream_open)");
        return fail(e, MCS_E_STATE, "the stream was closed by " + e->st_cause + ": reopen it (mcs_trade_stream_open)");
    }
    const int rc = stream_next_impl(e, true, max_samples, out, wait, level1, n_clusters, stats, l1stats);
    if (stats) stats->frontier = e->st_h;
    return rc;
}

int mcs_trade_stream_close(mcs_engine* e) {
    if (int st = check_engine(e)) return st;
    if (!e->st_trade && e->st_open)
        return fail(e, MCS_E_STATE, "the engine's stream is a plain session's (mcs_stream_close)");
    if (!e->st_open) {
        if (e->st_cause.empty() || !e->st_trade) return fail(e, MCS_E_STATE, "no stream is open");
        e->st_cause.clear();  // closed by the engine already: acknowledged
        return MCS_OK;
    }
    mcs::stream_shut(e, "mcs_trade_stream_close");
    e->st_cause.clear();
    return MCS_OK;
}

}  // extern "C"
