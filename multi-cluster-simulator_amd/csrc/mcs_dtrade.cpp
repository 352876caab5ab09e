// mcs_dtrade.cpp — host side of the lock-step trading system with DELAY schedulers (DESIGN.md
// §11): device state, the tick loop (two kernels per tick; world 1: 256 ticks per captured
// hipGraph, one host poll per replay; world > 1: an ncclAllGather of the exchange blocks between
// the kernels, or the caller-driven phases), capacity escalation and the result readers of
// mcs_trade.h; and trading sessions: the same system in online mode, resumed from
// its control block slice by slice on the replayed kernels (dts_slice, dtrade_session_run), and the
// session's Start stream (mcs_trade_session_state_series, mcs_trade_session_level1_series).
// Every decision is made by the gfx950 kernels of mcs_dtrade.hip; there is no CPU path.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "mcs_dtrade_grant.h"
#include "mcs_dtrade_internal.h"
#include "mcs_engine_impl.h"

namespace mcs {

struct DtradeDev {
    DtArgs a{};
    unsigned long long* tn = nullptr;
    unsigned long long* vn = nullptr;
    uint2* vcap = nullptr;
    uint32_t* sfin = nullptr;
    uint32_t* snode = nullptr;
    unsigned long long* scm = nullptr;
    unsigned long long* l1cm = nullptr;
    unsigned long long* l1jd = nullptr;
    unsigned long long* l1al = nullptr;
    DtCluster* cl = nullptr;
    DtTrader* tr = nullptr;
    DtCtl* ctl = nullptr;
    unsigned long long* l1snap = nullptr;
    mcs_contract_rec* trades = nullptr;
    mcs_foreign_rec* foreign = nullptr;
    unsigned char* xb = nullptr;  // world exchange blocks
    uint32_t* nv_all = nullptr;
    DtCtl* h_ctl = nullptr;  // 4 entries: [0] the control block as last read; [1], [2] the graph loop's polls;
                             // [3] a trading session's patch of the block (dts_slice)
    hipEvent_t pev[2] = {nullptr, nullptr};
    hipEvent_t tev[2] = {nullptr, nullptr};  // timing: the end of each pipelined replay
    double kernel_ms = 0.0;                  // device time of the last run (mcs_read_trade_stats)
    uint32_t tag[4] = {0, 0, 0, 0};          // caller-driven blocks: the layout tag (kDtTagBytes at the end)
    hipGraphExec_t graph = nullptr;
    hipGraphExec_t rgraph = nullptr;  // RCCL loop: kernels + all-gathers of kDtGraphTicks ticks
    // the resident tick (mcs_dtrade_mw.hip): exchange granules, placement granules + failure word
    // (uncached), the queued side effects of phase D
    unsigned long long* gx = nullptr;
    unsigned long long* gu = nullptr;
    void* ops = nullptr;
    uint32_t ops_cap = 0;
    bool rgraph_tried = false;
    uint32_t loop_form = kLoopGraph;
    bool begun = false;  // caller-driven lock-step in progress
    // external traders' calls (mcs_dtrade_grant.hip): the call's arguments and results, the walk's stash
    unsigned char* gbuf = nullptr;
    size_t gbuf_bytes = 0;
    unsigned long long* gstash = nullptr;
    size_t gstash_rows = 0;
    std::chrono::steady_clock::time_point w0{};
};

namespace {

constexpr uint64_t kDtTagBytes = 16;  // caller-driven exchange blocks end in the layout tag
constexpr uint32_t kDtGraphTicks = 256;  // (r05: 64 -> 256, A/B 14.57 -> 14.44 us per C5-DELAY tick)
constexpr uint32_t kDtResTicks = 1u << 16;  // ticks per launch of the resident tick
constexpr int kDtResFallback = -100;       // dt_run_res: the launch failed over (dtrade_run re-runs)

int dt_hip_fail(mcs_engine* e, const char* what, hipError_t st) {
    return fail(e, MCS_E_HIP, std::string(what) + ": " + hipGetErrorString(st));
}

uint32_t dt_auto_slots(uint32_t max_n) {
    uint32_t s = 256;
    while (s < 4u * max_n && s < kDtMaxSlots) s *= 2;
    return s;
}

int dtrade_alloc(mcs_engine* e) {
    if (e->dtd) return MCS_OK;
    const uint32_t C = e->C, Ct = e->C * e->world;
    if (Ct > kDtMaxClusters) return fail(e, MCS_E_INVALID, "more than 1024 clusters in a trading system");
    if (e->max_n > kDtMaxNodes) return fail(e, MCS_E_INVALID, "more than 1024 nodes in a cluster");
    const uint32_t S = e->cfg.slot_pool ? 64u * e->cfg.slot_pool : (e->tr_slots ? e->tr_slots : dt_auto_slots(e->max_n));
    if (S > kDtMaxSlots) return fail(e, MCS_E_INVALID, "slot pool above 4096");
    const uint32_t V = e->dt_vnodes ? e->dt_vnodes : 64u;
    const uint32_t NS = std::max<uint32_t>(e->dt_ns ? e->dt_ns : e->max_n, 1u), W = NS + V;
    // (a caller-driven block ends in a 16-byte layout tag that phase 1 checks on every gathered block)
    const unsigned long long blk = (unsigned long long)C * sizeof(DtRec) + (unsigned long long)C * W * 8ull +
                                   (e->comm ? 0ull : kDtTagBytes);
    DtradeDev* d = new (std::nothrow) DtradeDev();
    if (!d) return fail(e, MCS_E_NOMEM, "DELAY trading state");
    e->dtd = d;
    d->tag[0] = 0x5853434Du;  // "MCSX"
    d->tag[1] = 8u | (e->tr_agreed ? 4u : 0u);  // (8: the DELAY trading block)
    d->tag[2] = W;
    d->tag[3] = C;
    // (a trading session: the segments' capacity, job_off holding the segment starts)
    const size_t nj = std::max<uint64_t>(std::max<uint64_t>(e->total_jobs, e->job_off.empty() ? 0 : e->job_off[C]), 1);
    const uint64_t trade_cap = 1ull << 20;
    uint64_t foreign_cap = 1ull << 22;
    if (const char* env = getenv("MCS_DTRADE_FOREIGN_LOG_CAP"))  // tests: a Foreign log that overflows
        if (atoll(env) > 0 && (uint64_t)atoll(env) < foreign_cap) foreign_cap = (uint64_t)atoll(env);
    HIPCHK(e, hipMalloc(&d->tn, std::max<uint64_t>(e->total_nodes, 1) * 8));
    HIPCHK(e, hipMalloc(&d->vn, (size_t)C * V * 8));
    HIPCHK(e, hipMalloc(&d->vcap, (size_t)C * V * sizeof(uint2)));
    HIPCHK(e, hipMalloc(&d->sfin, (size_t)C * S * 4));
    HIPCHK(e, hipMalloc(&d->snode, (size_t)C * S * 4));
    HIPCHK(e, hipMalloc(&d->scm, (size_t)C * S * 8));
    HIPCHK(e, hipMalloc(&d->l1cm, nj * 8));
    HIPCHK(e, hipMalloc(&d->l1jd, nj * 8));
    HIPCHK(e, hipMalloc(&d->l1al, nj * 8));
    HIPCHK(e, hipMalloc(&d->cl, C * sizeof(DtCluster)));
    HIPCHK(e, hipMalloc(&d->tr, Ct * sizeof(DtTrader)));
    HIPCHK(e, hipMalloc(&d->xb, std::max<unsigned long long>(blk * e->world, 8ull)));
    HIPCHK(e, hipMemset(d->xb, 0, blk * e->world));
    HIPCHK(e, hipMalloc(&d->nv_all, Ct * 4));
    HIPCHK(e, hipMalloc(&d->ctl, sizeof(DtCtl)));
    HIPCHK(e, hipMalloc(&d->l1snap, (size_t)C * W * 8));
    HIPCHK(e, hipMalloc(&d->trades, trade_cap * sizeof(mcs_contract_rec)));
    HIPCHK(e, hipMalloc(&d->foreign, foreign_cap * sizeof(mcs_foreign_rec)));
    HIPCHK(e, hipHostMalloc(&d->h_ctl, 4 * sizeof(DtCtl), hipHostMallocDefault));
    DtArgs& a = d->a;
    a.C = C;
    a.V = V;
    a.S = S;
    a.base = e->rank * C;
    a.Ct = Ct;
    a.NS = NS;
    a.W = W;
    a.rank = e->rank;
    a.blk = blk;
    a.xb = d->xb;
    a.nv_all = d->nv_all;
    a.period = e->dt_external ? 0u : e->cfg.trader_period_s;  // (external traders: a system without rounds)
    a.ok_sleep = e->cfg.trade_ok_sleep_s;
    a.fail_sleep = e->cfg.trade_fail_sleep_s;
    a.lock_s = e->cfg.lock_s;
    a.sample_period = e->cfg.sample_period_s ? e->cfg.sample_period_s : 5u;
    a.max_wait = e->cfg.max_wait_s;
    a.t_max = e->cfg.t_max_s ? e->cfg.t_max_s : 0xFFFFFFFEu;
    a.trade_cap = trade_cap;
    a.foreign_cap = foreign_cap;
    a.node_off = e->d_node_off;
    a.cap = e->d_cap;
    a.free0 = e->d_free0;
    a.tn = d->tn;
    a.vn = d->vn;
    a.vcap = d->vcap;
    a.jobs = e->d_jobs;
    a.job_off = e->d_job_off;
    a.out_node = e->d_out_node;
    a.out_start = e->d_out_start;
    a.out_finish = e->d_out_finish;
    a.sfin = d->sfin;
    a.snode = d->snode;
    a.scm = d->scm;
    a.l1cm = d->l1cm;
    a.l1jd = d->l1jd;
    a.l1al = d->l1al;
    a.cl = d->cl;
    a.tr = d->tr;
    a.ctl = d->ctl;
    a.l1snap = d->l1snap;
    a.trade_log = d->trades;
    a.foreign_log = d->foreign;
    a.job_cnt = e->online ? e->d_job_cnt : nullptr;
    return MCS_OK;
}

int dt_poll(mcs_engine* e) {
    HIPCHK(e, hipMemcpyAsync(e->dtd->h_ctl, e->dtd->ctl, sizeof(DtCtl), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return MCS_OK;
}

// kDtGraphTicks ticks of the two kernels, captured once (released whenever a captured pointer changes)
int dt_ensure_graph(mcs_engine* e) {
    DtradeDev* d = e->dtd;
    hipError_t st = hipSuccess;
    if (!d->graph) {
        hipGraph_t g = nullptr;
        HIPCHK(e, hipStreamBeginCapture(e->stream, hipStreamCaptureModeThreadLocal));
        for (uint32_t t = 0; t < kDtGraphTicks; ++t) {
            st = launch_dtrade_tick(d->a, e->stream);
            if (st != hipSuccess) {
                (void)hipStreamEndCapture(e->stream, &g);
                if (g) (void)hipGraphDestroy(g);
                return dt_hip_fail(e, "DELAY trading capture", st);
            }
        }
        HIPCHK(e, hipStreamEndCapture(e->stream, &g));
        st = hipGraphInstantiate(&d->graph, g, nullptr, nullptr, 0);
        (void)hipGraphDestroy(g);
        if (st != hipSuccess) return dt_hip_fail(e, "hipGraphInstantiate", st);
    }
    for (hipEvent_t& ev : d->pev)
        if (!ev) HIPCHK(e, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    for (hipEvent_t& ev : d->tev)
        if (!ev) HIPCHK(e, hipEventCreate(&ev));
    return MCS_OK;
}

// the replayed loop from the control block as it stands until it reports done (after dt_ensure_graph);
// *end_ev_out: the end of the replay that finished the run
int dt_graph_loop(mcs_engine* e, hipEvent_t* end_ev_out) {
    DtradeDev* d = e->dtd;
    d->loop_form = kLoopGraph;
    // the polls are pipelined: replay k + 1 is queued before replay k's control block is read, so
    // the GPU never idles through a host round trip (a run that ended in replay k runs one more
    // replay of finished ticks, whose kernels return at once and write nothing)
    DtCtl* const hp = d->h_ctl + 1;
    hipEvent_t end_ev = nullptr;
    for (uint32_t k = 0;; ++k) {
        HIPCHK(e, hipGraphLaunch(d->graph, e->stream));
        HIPCHK(e, hipEventRecord(d->tev[k & 1u], e->stream));
        HIPCHK(e, hipMemcpyAsync(hp + (k & 1u), d->ctl, sizeof(DtCtl), hipMemcpyDeviceToHost, e->stream));
        HIPCHK(e, hipEventRecord(d->pev[k & 1u], e->stream));
        if (k == 0u) continue;
        HIPCHK(e, hipEventSynchronize(d->pev[(k - 1u) & 1u]));
        if (hp[(k - 1u) & 1u].done) {
            end_ev = d->tev[(k - 1u) & 1u];  // (kernel_ms ends with the replay that finished the run)
            break;
        }
    }
    HIPCHK(e, hipStreamSynchronize(e->stream));
    if (int s = dt_poll(e)) return s;  // (the final control block into h_ctl[0])
    *end_ev_out = end_ev;
    return MCS_OK;
}

int dt_run_once(mcs_engine* e, double* kernel_ms) {
    const hipError_t st = launch_dtrade_init(e->dtd->a, e->stream);
    if (st != hipSuccess) return dt_hip_fail(e, "DELAY trading init", st);
    if (int s = dt_ensure_graph(e)) return s;
    HIPCHK(e, hipEventRecord(e->ev0, e->stream));
    hipEvent_t end_ev = nullptr;
    if (int s = dt_graph_loop(e, &end_ev)) return s;
    float ms = 0.0f;
    HIPCHK(e, hipEventElapsedTime(&ms, e->ev0, end_ev));
    *kernel_ms = ms;
    return MCS_OK;
}

// MCS_DT_RESIDENT=0 forces the replayed kernels; the resident tick needs the whole system on this
// engine (no communicator, world 1), at most 64 clusters of at most 320 nodes (physical + virtual)
// and 1024 slots each.
bool dt_res_ok(mcs_engine* e) {
    const char* env = getenv("MCS_DT_RESIDENT");
    if ((env && atoi(env) == 0) || e->tr_no_resident || e->comm || e->world != 1) return false;
    if (e->dt_external) return false;  // (the system without rounds runs on the replayed kernels)
    const DtArgs& a = e->dtd->a;
    return a.Ct == a.C && a.C <= kDtResMaxClusters && e->max_n + a.V <= kDtResMaxNN && a.S <= kDtResMaxSlots &&
           a.S % 64u == 0u;
}

// the resident tick: one launch per kDtResTicks ticks (MCS_DT_RES_TICKS: fewer, so tests cross
// launch boundaries); kDtResFallback when a launch's workers were not all on one XCD or an
// exchange timed out, with nothing of the run kept
int dt_run_res(mcs_engine* e, double* kernel_ms) {
    DtradeDev* d = e->dtd;
    hipError_t st = launch_dtrade_init(d->a, e->stream);
    if (st != hipSuccess) return dt_hip_fail(e, "DELAY trading init", st);
    DtResArgs m{};
    m.ops_cap = d->a.S + d->a.V + 8u;  // a tick's side effects on a cluster: one per slot it takes, per virtual node
    if (!d->gx) {
        HIPCHK(e, hipMalloc(&d->gx, dtrade_mw_gx_bytes()));
        HIPCHK(e, hipExtMallocWithFlags((void**)&d->gu, dtrade_mw_gu_bytes(), hipDeviceMallocUncached));
        HIPCHK(e, hipMalloc(&d->ops, (size_t)d->a.C * m.ops_cap * dtrade_mw_op_bytes()));
        d->ops_cap = m.ops_cap;
    }
    m.gx = d->gx;
    m.gu = d->gu;
    m.ops = d->ops;
    m.ops_cap = d->ops_cap;
    const char* tenv = getenv("MCS_DT_RES_TICKS");
    const long tv = tenv ? atol(tenv) : 0;
    m.budget = tv > 0 && tv < (long)kDtResTicks ? (uint32_t)tv : kDtResTicks;
    m.nwg = (d->a.C + 3u) / 4u;
    d->loop_form = kLoopResidentMwXcd;
    HIPCHK(e, hipEventRecord(e->ev0, e->stream));
    for (;;) {
        st = launch_dtrade_mw(d->a, m, e->stream);
        if (st != hipSuccess) return dt_hip_fail(e, "resident DELAY trading tick", st);
        unsigned long long fw = 0;
        HIPCHK(e, hipMemcpyAsync(&fw, d->gu + dtrade_mw_fail_word(), sizeof(fw), hipMemcpyDeviceToHost, e->stream));
        if (int s = dt_poll(e)) return s;
        if (fw != 0ull) return kDtResFallback;
        // (MCS_DT_RES_FORCE_FAIL=1: tests take the fail-over path after the first launch)
        if (const char* ff = getenv("MCS_DT_RES_FORCE_FAIL"); ff && atoi(ff) != 0) return kDtResFallback;
        if (d->h_ctl->done) break;
    }
    HIPCHK(e, hipEventRecord(e->ev1, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    float ms = 0.0f;
    HIPCHK(e, hipEventElapsedTime(&ms, e->ev0, e->ev1));
    *kernel_ms = ms;
    return MCS_OK;
}

// N engines (one per GPU): the exchange blocks are all-gathered in place over xGMI between the two
// kernels of every tick; one host poll per kDtGraphTicks ticks (the kernels of finished ticks
// return at once on ctl->done, identically on every rank)
int dt_run_rccl(mcs_engine* e, double* kernel_ms) {
    DtradeDev* d = e->dtd;
    ncclComm_t comm = (ncclComm_t)e->comm;
    hipError_t st = launch_dtrade_init(d->a, e->stream);
    if (st != hipSuccess) return dt_hip_fail(e, "DELAY trading init", st);
    auto tick = [&](hipStream_t s) -> bool {
        if (launch_dtrade_step(d->a, s) != hipSuccess) return false;
        if (ncclAllGather(d->xb + (size_t)e->rank * d->a.blk, d->xb, d->a.blk, ncclUint8, comm, s) != ncclSuccess)
            return false;
        return launch_dtrade_trader(d->a, s) == hipSuccess;
    };
    if (!d->rgraph_tried) {  // (no host enqueue per tick when RCCL can be captured)
        d->rgraph_tried = true;
        d->rgraph = capture_tick_graph(e->stream, kDtGraphTicks, tick);
    }
    d->loop_form = d->rgraph ? kLoopRcclGraph : kLoopRcclEager;
    HIPCHK(e, hipEventRecord(e->ev0, e->stream));
    for (;;) {
        if (d->rgraph) {
            HIPCHK(e, hipGraphLaunch(d->rgraph, e->stream));
            if (int s = dt_poll(e)) return s;
            if (d->h_ctl->done) break;
            continue;
        }
        for (uint32_t t = 0; t < kDtGraphTicks; ++t) {
            st = launch_dtrade_step(d->a, e->stream);
            if (st != hipSuccess) return dt_hip_fail(e, "dt_step_kernel", st);
            const ncclResult_t r = ncclAllGather(d->xb + (size_t)e->rank * d->a.blk, d->xb, d->a.blk, ncclUint8,
                                                 comm, e->stream);
            if (r != ncclSuccess)
                return fail(e, MCS_E_RCCL, std::string("ncclAllGather(exchange blocks): ") + ncclGetErrorString(r));
            st = launch_dtrade_trader(d->a, e->stream);
            if (st != hipSuccess) return dt_hip_fail(e, "dt_trader_kernel", st);
        }
        if (int s = dt_poll(e)) return s;
        if (d->h_ctl->done) break;
    }
    HIPCHK(e, hipEventRecord(e->ev1, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    float ms = 0.0f;
    HIPCHK(e, hipEventElapsedTime(&ms, e->ev0, e->ev1));
    *kernel_ms = ms;
    return MCS_OK;
}

// every rank must lay its exchange block out alike: the snapshot stride is the largest cluster of
// the whole system, and the cluster count per rank must match
int dt_agree_shape(mcs_engine* e) {
    uint32_t* buf = nullptr;
    HIPCHK(e, hipMalloc(&buf, 5 * sizeof(uint32_t)));
    /* max of C and of ~C (= ~min C): every rank sees the same verdict, so a mismatch fails on
     * every rank instead of leaving the ranks with the largest C in the tick loop */
    // (and the largest learned capacities, so every rank allocates the same slot and vnode pools)
    const uint32_t h[5] = {e->max_n, e->C, ~e->C, e->tr_slots, e->dt_vnodes};
    uint32_t mx[5] = {0, 0, 0, 0, 0};
    HIPCHK(e, hipMemcpy(buf, h, sizeof(h), hipMemcpyHostToDevice));
    ncclResult_t r = ncclAllReduce(buf, buf, 5, ncclUint32, ncclMax, (ncclComm_t)e->comm, e->stream);
    hipError_t st = hipStreamSynchronize(e->stream);
    if (r == ncclSuccess && st == hipSuccess) st = hipMemcpy(mx, buf, sizeof(mx), hipMemcpyDeviceToHost);
    (void)hipFree(buf);
    if (r != ncclSuccess) return fail(e, MCS_E_RCCL, std::string("ncclAllReduce(shape): ") + ncclGetErrorString(r));
    if (st != hipSuccess) return dt_hip_fail(e, "shape exchange", st);
    if (mx[1] != ~mx[2]) return fail(e, MCS_E_INVALID, "sharded DELAY trading needs the same cluster count on every rank");
    e->dt_ns = mx[0];
    e->tr_slots = mx[3];
    e->dt_vnodes = mx[4];
    return MCS_OK;
}

int dt_clusters(mcs_engine* e, std::vector<DtCluster>& cl) {
    cl.resize(e->C);
    HIPCHK(e, hipStreamSynchronize(e->stream));
    HIPCHK(e, hipMemcpy(cl.data(), e->dtd->cl, e->C * sizeof(DtCluster), hipMemcpyDeviceToHost));
    HIPCHK(e, hipMemcpy(e->dtd->h_ctl, e->dtd->ctl, sizeof(DtCtl), hipMemcpyDeviceToHost));
    return MCS_OK;
}

// One slice of a trading session (DESIGN.md §14 "Trading sessions"): every tick T < t_hor from where
// the session stands, or with t_hor = MCS_TIME_NONE every tick until each job held is decided.  The
// lock-step state is in HBM as the last tick left it; the host only re-plans the control block: the
// resume tick min(parked tick, earliest arrival appended since), the rounds due at it, the horizon.
// Short slices run eagerly (8 ticks, then 32, each with one poll); longer ones through the graph.
int dts_resume(mcs_engine* e, uint32_t t_res, uint32_t any_due, uint32_t t_hor, double* kernel_ms);

int dts_slice(mcs_engine* e, uint32_t t_hor, double* kernel_ms) {
    DtradeDev* d = e->dtd;
    *kernel_ms = 0.0;
    e->ts_ticks_last = 0;
    DtCtl& c = d->h_ctl[0];  // (the control block as the last slice, or the init kernel, left it)
    const bool fresh = c.ticks == 0u && c.done == 0u;
    if (!fresh && (c.flags & (MCS_FLAG_T_MAX | MCS_FLAG_OVERFLOW))) return MCS_OK;  // the clock stays at t_max_s
    uint32_t t_res = 0u, any_due = 1u;
    if (!fresh) {
        t_res = std::min(e->ts_t_next, e->ts_pend_min);
        any_due = t_res == e->ts_t_next ? e->ts_any_due : 0u;  // (below the parked tick no round is due)
    }
    if (t_hor != MCS_TIME_NONE) {
        if (t_res < t_hor)
            if (int s = dts_resume(e, t_res, any_due, t_hor, kernel_ms)) return s;
        // External traders (DESIGN.md §14 "External traders"): a grant acts on the node state the last
        // executed tick left, so a finite horizon always ends with a tick at h - 1.  Where the next-tick
        // rule parked below it, the run is resumed once at T = h - 1 and parks again: that tick does the
        // releases due and, on a multiple of the sample period, the sample; it decides nothing (ticks are
        // consecutive while any job is queued), and no arrival lies below h (the rule would have chosen it).
        if (e->dt_external && t_hor != 0u && c.ticks != 0u && !(c.flags & (MCS_FLAG_T_MAX | MCS_FLAG_OVERFLOW)) &&
            c.T < t_hor - 1u)
            if (int s = dts_resume(e, t_hor - 1u, 0u, t_hor, kernel_ms)) return s;
        return MCS_OK;
    }
    std::vector<DtCluster> cl;
    if (int s = dt_clusters(e, cl)) return s;
    uint64_t decided = 0;
    for (uint32_t k = 0; k < e->C; ++k) decided += cl[k].decided;
    if (decided == e->total_jobs) return MCS_OK;  // a drain with nothing undecided executes no tick
    return dts_resume(e, t_res, any_due, t_hor, kernel_ms);
}

// the session from tick t_res until it parks or ends under the horizon t_hor; adds to *kernel_ms and to
// the ticks of the run
int dts_resume(mcs_engine* e, uint32_t t_res, uint32_t any_due, uint32_t t_hor, double* kernel_ms) {
    DtradeDev* d = e->dtd;
    DtCtl& c = d->h_ctl[0];
    const uint32_t ticks0 = c.ticks;
    DtCtl& p = d->h_ctl[3];
    p = c;
    p.T = t_res;
    p.done = 0u;
    p.any_due = any_due;
    p.pad0 = t_hor;
    if (int s = dt_ensure_graph(e)) return s;  // (before the timed section: the capture is host work)
    HIPCHK(e, hipEventRecord(e->ev0, e->stream));
    HIPCHK(e, hipMemcpyAsync(d->ctl, &p, sizeof(DtCtl), hipMemcpyHostToDevice, e->stream));
    d->loop_form = kLoopGraph;
    hipEvent_t end_ev = nullptr;
    for (const uint32_t n : {8u, 32u}) {
        for (uint32_t t = 0; t < n; ++t) {
            const hipError_t st = launch_dtrade_tick(d->a, e->stream);
            if (st != hipSuccess) return dt_hip_fail(e, "DELAY trading tick", st);
        }
        HIPCHK(e, hipEventRecord(e->ev1, e->stream));
        if (int s = dt_poll(e)) return s;
        if (c.done) {
            end_ev = e->ev1;
            break;
        }
    }
    if (!end_ev)
        if (int s = dt_graph_loop(e, &end_ev)) return s;
    float ms = 0.0f;
    HIPCHK(e, hipEventElapsedTime(&ms, e->ev0, end_ev));
    *kernel_ms += ms;
    e->ts_ticks_last += c.ticks - ticks0;
    e->ts_ticks_total = c.ticks;
    e->ts_t_last = c.T;
    e->ts_pend_min = MCS_TIME_NONE;  // every arrival held was known to the last tick's next-tick rule
    if (!(c.flags & (MCS_FLAG_T_MAX | MCS_FLAG_OVERFLOW))) {
        e->ts_t_next = c.pad0;
        e->ts_any_due = c.any_due;
    }
    return MCS_OK;
}

}  // namespace

void dtrade_session_reset(mcs_engine* e) {
    dtrade_free(e);  // (its arrays follow the segments: allocated again by the first run)
    e->ts_begun = e->ts_failed = e->ts_drained = false;
    e->ts_t_last = e->ts_t_next = 0u;
    e->ts_any_due = 1u;
    e->ts_pend_min = MCS_TIME_NONE;
    e->ts_ticks_last = e->ts_ticks_total = e->ts_restarts = 0u;
    e->ts_grants.clear();  // (the external traders' timeline starts over)
}

bool dtrade_stream_view(mcs_engine* e, DtStreamView* v) {
    const DtradeDev* d = e->dtd;
    if (!d) return false;
    static_assert(sizeof(DtCluster) % sizeof(uint32_t) == 0, "nv is read with a word stride");
    v->vcap = d->vcap;
    v->flog = d->foreign;
    v->nv_src = &d->cl->nv;
    v->nv_stride = (uint32_t)(sizeof(DtCluster) / sizeof(uint32_t));
    v->V = d->a.V;
    v->flags = d->h_ctl->flags;
    v->n_foreign = d->h_ctl->n_foreign;
    v->foreign_cap = d->a.foreign_cap;
    v->n_trades = d->h_ctl->n_trades;
    v->trade_cap = d->a.trade_cap;
    return true;
}

static int dtrade_session_run_body(mcs_engine* e, uint32_t t_hor, mcs_stats* stats);

int dtrade_session_run(mcs_engine* e, uint32_t t_hor, mcs_stats* stats) {
    if (e->world != 1 || e->comm)
        return fail(e, MCS_E_STATE, "a trading session runs on one engine that holds the whole system (rank 0 of "
                                    "world 1, no communicator): sharded DELAY trading runs as a batch");
    if (e->dtd && e->dtd->begun)
        return fail(e, MCS_E_STATE, "a caller-driven lock-step run is in progress (mcs_trade_end first)");
    if (!e->online)
        if (int s = online_begin(e)) return s;
    if (e->ts_failed)
        return fail(e, MCS_E_STATE, "the trading session failed (capacity exhausted): mcs_rewind or submit again");
    const uint32_t t_max = e->cfg.t_max_s ? e->cfg.t_max_s : 0xFFFFFFFEu;
    if (t_hor != MCS_TIME_NONE && t_hor < e->on_t_hor)
        return fail(e, MCS_E_INVALID, "horizons must be non-decreasing (last: " + std::to_string(e->on_t_hor) + ")");
    if (t_hor != MCS_TIME_NONE && (uint64_t)t_hor > (uint64_t)t_max + 1u)
        return fail(e, MCS_E_INVALID, "the horizon lies above t_max_s + 1 = " + std::to_string((uint64_t)t_max + 1u) +
                                          ": cfg.t_max_s bounds the lock-step clock");
    // (a call refused above executed nothing: an open stream stays as it is)
    const int st = dtrade_session_run_body(e, t_hor, stats);
    trade_stream_run_end(e, t_hor, st);
    return st;
}

// ---- external traders: one grant call on the device (mcs_dtrade_grant.hip) -------------------------
// The call's entries, stably grouped by the cluster they act on, go up in one copy with the zeroed
// status; the results and the status come back in one copy behind one synchronisation: the launches and
// synchronisations of a call do not depend on n.  *flags: MCS_FLAG_OVERFLOW / MCS_FLAG_VNODE_OVERFLOW
// when a pool overflowed (the device state is then partly written: the caller escalates and replays).
static int dt_grant_apply(mcs_engine* e, const DtGrantCall& call, mcs_vnode_result* res, uint32_t* flags,
                          uint32_t* added, double* kernel_ms) {
    DtradeDev* d = e->dtd;
    const bool provide = !call.req.empty();
    const uint32_t n = (uint32_t)(provide ? call.req.size() : call.node.size());
    *flags = 0u;
    *added = 0u;
    *kernel_ms = 0.0;
    if (n == 0) return MCS_OK;
    std::vector<uint32_t> order(n), inv(n), soff(n);
    for (uint32_t i = 0; i < n; ++i) order[i] = i;
    auto key = [&](uint32_t i) { return provide ? call.req[i].responder : call.node[i].cluster; };
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return key(x) < key(y); });
    std::vector<DtGrantGroup> groups;
    uint64_t rows = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t c = key(order[i]);
        inv[order[i]] = i;
        if (groups.empty() || groups.back().cluster != c) groups.push_back(DtGrantGroup{c, i, i, 0u});
        groups.back().end = i + 1u;
        soff[i] = (uint32_t)rows;  // (at most 4096 * (1024 + 256) rows)
        if (provide) rows += (e->node_off[c + 1] - e->node_off[c]) + d->a.V;
    }
    const uint32_t ng = (uint32_t)groups.size();
    // [results | status | entries | order | inv | soff | groups | counts]: the upload is [status, counts),
    // the download [results, entries)
    const size_t esz = provide ? sizeof(mcs_vnode_request) : sizeof(mcs_vnode_grant);
    const size_t o_res = 0, o_status = o_res + (size_t)n * sizeof(mcs_vnode_result);
    const size_t o_ent = o_status + sizeof(DtGrantStatus), o_order = o_ent + (size_t)n * esz;
    const size_t o_inv = o_order + (size_t)n * 4, o_soff = o_inv + (size_t)n * 4, o_groups = o_soff + (size_t)n * 4;
    const size_t o_cnt = o_groups + (size_t)ng * sizeof(DtGrantGroup), total = o_cnt + (size_t)n * 4;
    static_assert(sizeof(mcs_vnode_result) == 16 && sizeof(DtGrantStatus) == 16 && sizeof(DtGrantGroup) == 16 &&
                      sizeof(mcs_vnode_request) % 8 == 0 && sizeof(mcs_vnode_grant) == 16,
                  "grant buffer layout");
    if (d->gbuf_bytes < total) {
        dfree(d->gbuf);
        d->gbuf_bytes = 0;
        HIPCHK(e, hipMalloc(&d->gbuf, total * 2));
        d->gbuf_bytes = total * 2;
    }
    if (provide && d->gstash_rows < rows) {
        dfree(d->gstash);
        d->gstash_rows = 0;
        HIPCHK(e, hipMalloc(&d->gstash, rows * 2 * 16));
        d->gstash_rows = rows * 2;
    }
    std::vector<unsigned char> up(o_cnt - o_status, 0), down(o_ent - o_res);
    unsigned char* u = up.data() - o_status;  // (indexed by the buffer's offsets)
    for (uint32_t i = 0; i < n; ++i) {
        if (provide) std::memcpy(u + o_ent + (size_t)i * esz, &call.req[order[i]], esz);
        else std::memcpy(u + o_ent + (size_t)i * esz, &call.node[order[i]], esz);
    }
    std::memcpy(u + o_order, order.data(), (size_t)n * 4);
    std::memcpy(u + o_inv, inv.data(), (size_t)n * 4);
    std::memcpy(u + o_soff, soff.data(), (size_t)n * 4);
    std::memcpy(u + o_groups, groups.data(), (size_t)ng * sizeof(DtGrantGroup));
    DtGrantArgs g{};
    g.req = provide ? reinterpret_cast<const mcs_vnode_request*>(d->gbuf + o_ent) : nullptr;
    g.node = provide ? nullptr : reinterpret_cast<const mcs_vnode_grant*>(d->gbuf + o_ent);
    g.order = reinterpret_cast<const uint32_t*>(d->gbuf + o_order);
    g.inv = reinterpret_cast<const uint32_t*>(d->gbuf + o_inv);
    g.soff = reinterpret_cast<const uint32_t*>(d->gbuf + o_soff);
    g.groups = reinterpret_cast<const DtGrantGroup*>(d->gbuf + o_groups);
    g.res = reinterpret_cast<mcs_vnode_result*>(d->gbuf + o_res);
    g.cnt = reinterpret_cast<uint32_t*>(d->gbuf + o_cnt);
    g.stash = d->gstash;
    g.status = reinterpret_cast<DtGrantStatus*>(d->gbuf + o_status);
    g.n_foreign = d->h_ctl->n_foreign;
    g.n = n;
    g.n_groups = ng;
    g.T = e->ts_t_last;
    HIPCHK(e, hipMemcpyAsync(d->gbuf + o_status, up.data(), up.size(), hipMemcpyHostToDevice, e->stream));
    HIPCHK(e, hipEventRecord(e->ev0, e->stream));
    const hipError_t st = provide ? launch_dtrade_grant_provide(d->a, g, e->stream)
                                  : launch_dtrade_grant_receive(d->a, g, e->stream);
    if (st != hipSuccess) return dt_hip_fail(e, "external traders' grant", st);
    HIPCHK(e, hipEventRecord(e->ev1, e->stream));
    HIPCHK(e, hipMemcpyAsync(down.data(), d->gbuf + o_res, down.size(), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));  // (the call's one synchronisation)
    float ms = 0.0f;
    HIPCHK(e, hipEventElapsedTime(&ms, e->ev0, e->ev1));
    *kernel_ms = ms;
    DtGrantStatus status;
    std::memcpy(&status, down.data() + o_status, sizeof(status));
    *flags = status.flags;
    if (status.flags & (MCS_FLAG_OVERFLOW | MCS_FLAG_VNODE_OVERFLOW)) return MCS_OK;
    if (provide) {
        if (res) std::memcpy(res, down.data() + o_res, (size_t)n * sizeof(mcs_vnode_result));
        *added = status.added;
        d->h_ctl->n_foreign = status.n_foreign;  // (the host's copy of the control block follows the device's)
        if (status.flags & MCS_FLAG_LOG_OVERFLOW) d->h_ctl->flags |= MCS_FLAG_LOG_OVERFLOW;
    }
    return MCS_OK;
}

// A replay of a session that holds grants (after a capacity escalation): slice by slice, up to t + 1 with
// its forced tick, then the calls kept for tick t in order, and so on; then the slice to the horizon.
// *gflags: a pool overflow of a re-applied call (the caller escalates again).
static int dts_replay(mcs_engine* e, uint32_t t_hor, double* kernel_ms, uint32_t* gflags) {
    uint32_t ticks = 0;
    for (size_t i = 0; i < e->ts_grants.size();) {
        const uint32_t t = e->ts_grants[i].t;
        double ms = 0.0;
        if (int s = dts_slice(e, t + 1u, &ms)) return s;
        *kernel_ms += ms;
        ticks += e->ts_ticks_last;
        if (e->dtd->h_ctl->flags & (MCS_FLAG_OVERFLOW | MCS_FLAG_VNODE_OVERFLOW)) return MCS_OK;
        if (e->ts_t_last != t)
            return fail(e, MCS_E_STATE, "the replay of a trading session did not reach a kept grant's tick");
        for (; i < e->ts_grants.size() && e->ts_grants[i].t == t; ++i) {
            uint32_t fl = 0, added = 0;
            if (int s = dt_grant_apply(e, e->ts_grants[i], nullptr, &fl, &added, &ms)) return s;
            *kernel_ms += ms;
            if (fl & (MCS_FLAG_OVERFLOW | MCS_FLAG_VNODE_OVERFLOW)) {
                *gflags |= fl;
                return MCS_OK;
            }
        }
    }
    double ms = 0.0;
    if (int s = dts_slice(e, t_hor, &ms)) return s;
    *kernel_ms += ms;
    e->ts_ticks_last += ticks;
    return MCS_OK;
}

static int dts_run_loop(mcs_engine* e, uint32_t t_hor, double* kms_out, uint32_t* escalations_out);

static int dtrade_session_run_body(mcs_engine* e, uint32_t t_hor, mcs_stats* stats) {
    const auto w0 = std::chrono::steady_clock::now();
    e->on_series_ok = false;  // until this run has ended well (mcs_trade_session_state_series)
    uint32_t escalations = 0;
    double kms = 0.0;
    if (int s = dts_run_loop(e, t_hor, &kms, &escalations)) return s;
    e->dt_learn_s = e->cfg.slot_pool ? 0u : e->dtd->a.S;
    e->dt_learn_v = e->dtd->a.V;
    e->dtd->kernel_ms = kms;
    e->has_run = true;
    e->dtrade_run = true;
    e->trade_run = false;
    e->delay_run = true;
    e->ts_drained = t_hor == MCS_TIME_NONE;
    e->on_series_ok = true;
    e->on_series_hor = t_hor;
    if (t_hor != MCS_TIME_NONE) e->on_t_hor = e->on_t_done = t_hor;
    // the lock-step clock is common to all clusters: later arrivals lie above the last executed tick
    if (e->ts_ticks_total) e->on_floor.assign(e->C, e->ts_t_last + 1u);
    if (stats) {
        std::vector<DtCluster> cl;
        if (int s = dt_clusters(e, cl)) return s;
        mcs_stats st{};
        st.jobs = e->total_jobs;
        for (uint32_t k = 0; k < e->C; ++k) {
            st.placed += cl[k].decided;
            st.waited += cl[k].moved;
        }
        st.pending = e->total_jobs - st.placed;
        st.clusters = e->C;
        st.escalations = escalations;
        st.slot_pool = e->dtd->a.S / 64u;
        st.kernel_ms = kms;
        st.wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - w0).count();
        st.t_horizon = t_hor;
        st.online = 1u;
        *stats = st;
    }
    return MCS_OK;
}

// a slot-pool or virtual-node overflow (flags) in a slice or a grant: the pools grow as dtrade_run's do and
// the lock-step state is dropped, so that the next slice replays the session from t = 0 over every job held
// (which the slicing guarantee makes the state a session with these capacities would hold); or, with the
// capacity exhausted, the session fails
static int dts_escalate(mcs_engine* e, uint32_t flags) {
    const uint32_t S = e->dtd->a.S, V = e->dtd->a.V;
    const bool grow_s = (flags & MCS_FLAG_OVERFLOW) != 0, grow_v = (flags & MCS_FLAG_VNODE_OVERFLOW) != 0;
    if ((grow_s && (e->cfg.slot_pool || S >= kDtMaxSlots)) || (grow_v && V >= kDtMaxVnodes)) {
        e->ts_failed = true;
        return fail(e, MCS_E_CAPACITY, "DELAY trading capacity exhausted (slots or virtual nodes): the session "
                                       "is failed until mcs_rewind or a new submit");
    }
    const uint32_t ns = grow_s ? std::min<uint32_t>((S + S / 2u + 63u) / 64u * 64u, kDtMaxSlots) : S,
                   nv = grow_v ? std::min<uint32_t>(V * 4u, kDtMaxVnodes) : V;
    dtrade_free(e);
    e->tr_slots = ns;
    e->dt_vnodes = nv;
    ++e->ts_restarts;
    trade_stream_restart(e);  // (an open stream keeps t_next and rebuilds once)
    return MCS_OK;
}

// the slices of one run (or of a grant's replay) with the capacity escalation around them: on a slot-pool
// or virtual-node overflow the pools grow and the session is replayed from t = 0, its grants included
static int dts_run_loop(mcs_engine* e, uint32_t t_hor, double* kms_out, uint32_t* escalations_out) {
    uint32_t escalations = 0;
    double kms = 0.0;
    for (;;) {
        bool from0 = false;
        if (!e->ts_begun || !e->dtd) {  // from t = 0: the session's first run, or a replay after an escalation
            from0 = true;
            if (!e->ts_begun) {  // (the capacities the last run of these inputs escalated to)
                e->tr_slots = e->dt_learn_s;
                e->dt_vnodes = e->dt_learn_v;
            }
            e->dt_ns = 0;
            if (e->dtd) dtrade_free(e);
            if (int s = dtrade_alloc(e)) return s;
            const hipError_t st = launch_dtrade_init(e->dtd->a, e->stream);
            if (st != hipSuccess) return dt_hip_fail(e, "DELAY trading init", st);
            if (int s = dt_poll(e)) return s;
            e->ts_begun = true;
            e->ts_t_last = e->ts_t_next = 0u;
            e->ts_any_due = 1u;
            e->ts_ticks_total = 0u;
        }
        double ms = 0.0;
        uint32_t gflags = 0u;
        if (from0 && !e->ts_grants.empty()) {  // (external traders: a replay re-applies the grants)
            if (int s = dts_replay(e, t_hor, &ms, &gflags)) return s;
        } else {
            if (int s = dts_slice(e, t_hor, &ms)) return s;
        }
        kms += ms;
        const uint32_t flags = e->dtd->h_ctl->flags | gflags;
        if (!(flags & (MCS_FLAG_OVERFLOW | MCS_FLAG_VNODE_OVERFLOW))) break;
        if (int s = dts_escalate(e, flags)) return s;
        ++escalations;
    }
    *kms_out += kms;
    *escalations_out += escalations;
    return MCS_OK;
}

// what both grant calls check before their arguments
static int dt_grant_check(mcs_engine* e, const char* call) {
    const std::string c(call);
    if (!is_trade_session(e))
        return fail(e, MCS_E_STATE, c + " acts on a trading session (online mode with MCS_POLICY_DELAY and "
                                        "cfg.trader): there is no trading session");
    if (!e->dt_external)
        return fail(e, MCS_E_STATE, c + " needs external mode (mcs_trade_external): the built-in trader rounds are "
                                        "on, and they share no locks with a trader outside the engine");
    if (e->ts_failed)
        return fail(e, MCS_E_STATE, c + ": the trading session failed (capacity exhausted, MCS_E_CAPACITY): "
                                        "mcs_rewind or submit again, then run");
    if (!e->ts_begun || !e->dtd || e->ts_ticks_total == 0u)
        return fail(e, MCS_E_STATE, c + " acts on the state the last executed tick left: no tick has been executed "
                                        "yet (mcs_run first)");
    const DtCtl& ctl = *e->dtd->h_ctl;
    // (MCS_FLAG_T_MAX does not refuse: the tick at t_max_s raises it, and the reference's traders run their
    // rounds at that tick too (DT-KAT1 and DT-KAT6b end with one); the clock then stays there, so such a
    // grant reaches the logs and the counters and no later decision)
    if (ctl.flags & (MCS_FLAG_OVERFLOW | MCS_FLAG_VNODE_OVERFLOW))
        return fail(e, MCS_E_STATE, c + ": a slot-pool or virtual-node overflow (MCS_FLAG_VNODE_OVERFLOW) cut the "
                                        "run short");
    if ((ctl.flags & MCS_FLAG_LOG_OVERFLOW) || ctl.n_foreign > e->dtd->a.foreign_cap ||
        ctl.n_trades > e->dtd->a.trade_cap)
        return fail(e, MCS_E_STATE, c + ": the Foreign or contract log overflowed (MCS_FLAG_LOG_OVERFLOW): records "
                                        "were dropped");
    return MCS_OK;
}

// an accepted grant call: applied to the device state; on a pool overflow the session escalates, is
// replayed from t = 0 up to the tick the call acts at (its earlier grants re-applied) and the call is
// applied again; then it joins the kept calls
static int dt_grant_call(mcs_engine* e, DtGrantCall&& call, mcs_vnode_result* res, mcs_vnode_stats* stats) {
    mcs_vnode_stats st{};
    const uint32_t t = e->ts_t_last;
    call.t = t;
    st.n = (uint32_t)(call.req.size() + call.node.size());
    for (;;) {
        uint32_t fl = 0, added = 0;
        double ms = 0.0;
        if (int s = dt_grant_apply(e, call, res, &fl, &added, &ms)) return s;
        st.kernel_ms += ms;
        st.foreign_added = added;
        if (!(fl & (MCS_FLAG_OVERFLOW | MCS_FLAG_VNODE_OVERFLOW))) break;
        int s = dts_escalate(e, fl);
        uint32_t esc = 0;
        double kms = 0.0;
        if (s == MCS_OK) s = dts_run_loop(e, t + 1u, &kms, &esc);
        if (s != MCS_OK) {  // (as a run that failed: an open stream closes)
            trade_stream_run_end(e, t + 1u, s);
            return s;
        }
        st.kernel_ms += kms;
        st.replayed = 1u;
        e->dt_learn_s = e->cfg.slot_pool ? 0u : e->dtd->a.S;
        e->dt_learn_v = e->dtd->a.V;
        e->dtrade_run = true;  // (dtrade_free dropped it with the state)
        if (e->ts_t_last != t)
            return fail(e, MCS_E_STATE, "the replay of a trading session did not reach the grant's tick");
    }
    if (res)
        for (uint32_t i = 0; i < st.n; ++i) st.n_ok += res[i].ok ? 1u : 0u;
    else
        st.n_ok = st.n;
    e->ts_grants.push_back(std::move(call));
    if (stats) *stats = st;
    return MCS_OK;
}

int dtrade_session_relayout(mcs_engine* e, const uint64_t* d_old_off, const uint64_t* d_new_off, size_t rows) {
    DtradeDev* d = e->dtd;
    if (!d) return MCS_OK;  // (no run yet: the first one allocates for the new segments)
    unsigned long long* nw[3] = {nullptr, nullptr, nullptr};
    for (auto& p : nw) HIPCHK(e, hipMalloc(&p, (rows ? rows : 1) * 8));
    const unsigned long long* src[3] = {d->l1cm, d->l1jd, d->l1al};
    const hipError_t st = launch_dtrade_relayout(d->cl, e->C, d_old_off, d_new_off, src, nw, e->stream);
    if (st != hipSuccess) return dt_hip_fail(e, "Level1 relayout", st);
    HIPCHK(e, hipStreamSynchronize(e->stream));
    dfree(d->l1cm);
    dfree(d->l1jd);
    dfree(d->l1al);
    d->a.l1cm = d->l1cm = nw[0];
    d->a.l1jd = d->l1jd = nw[1];
    d->a.l1al = d->l1al = nw[2];
    return MCS_OK;
}

void dtrade_session_rebind(mcs_engine* e) {
    DtradeDev* d = e->dtd;
    if (!d) return;
    dtrade_release_graphs(e);  // (a captured graph holds the kernels' arguments by value)
    d->a.jobs = e->d_jobs;
    d->a.job_off = e->d_job_off;
    d->a.out_node = e->d_out_node;
    d->a.out_start = e->d_out_start;
    d->a.out_finish = e->d_out_finish;
    d->a.job_cnt = e->d_job_cnt;
}

int refuse_trade_session(mcs_engine* e, const char* call) {
    if (!is_trade_session(e)) return MCS_OK;
    return fail(e, MCS_E_STATE, std::string(call) + " is not available in a trading session (online mode with "
                                    "MCS_POLICY_DELAY and cfg.trader): it reads batch runs and sessions without "
                                    "trading (in a trading session: mcs_trade_session_state_series, "
                                    "mcs_trade_session_level1_series, mcs_trade_stream_open)");
}

void dtrade_release_graphs(mcs_engine* e) {
    if (DtradeDev* d = e->dtd) {
        if (d->graph) (void)hipGraphExecDestroy(d->graph);
        if (d->rgraph) (void)hipGraphExecDestroy(d->rgraph);
        d->graph = d->rgraph = nullptr;
    }
}

void dtrade_free(mcs_engine* e) {
    DtradeDev* d = e->dtd;
    if (!d) return;
    if (e->stream) (void)hipStreamSynchronize(e->stream);
    if (d->graph) (void)hipGraphExecDestroy(d->graph);
    if (d->rgraph) (void)hipGraphExecDestroy(d->rgraph);
    dfree(d->tn);
    dfree(d->vn);
    dfree(d->vcap);
    dfree(d->sfin);
    dfree(d->snode);
    dfree(d->scm);
    dfree(d->l1cm);
    dfree(d->l1jd);
    dfree(d->l1al);
    dfree(d->cl);
    dfree(d->tr);
    dfree(d->ctl);
    dfree(d->l1snap);
    dfree(d->trades);
    dfree(d->foreign);
    dfree(d->xb);
    dfree(d->nv_all);
    dfree(d->gx);
    dfree(d->gu);
    dfree(d->ops);
    dfree(d->gbuf);
    dfree(d->gstash);
    if (d->h_ctl) (void)hipHostFree(d->h_ctl);
    for (hipEvent_t& ev : d->pev)
        if (ev) (void)hipEventDestroy(ev);
    for (hipEvent_t& ev : d->tev)
        if (ev) (void)hipEventDestroy(ev);
    delete d;
    e->dtd = nullptr;
    e->dtrade_run = false;
}

int dtrade_run(mcs_engine* e, mcs_stats* stats) {
    if (e->world > 1 && !e->comm)
        return fail(e, MCS_E_STATE, "sharded DELAY trading run needs mcs_comm_init (or mcs_trade_phase)");
    const auto w0 = std::chrono::steady_clock::now();
    if (e->dtd && e->dtd->a.job_cnt) dtrade_free(e);  // (a trading session's state: segments, not dense rows)
    // the capacities the last run of these inputs escalated to (reset when clusters, jobs or the
    // shard change): a re-run of the same system starts there instead of repeating the overflowed run
    e->tr_slots = e->dt_learn_s;
    e->dt_vnodes = e->dt_learn_v;
    // a communicator selects the RCCL loop (world 1 included: one rank's all-gather is a copy)
    const bool rccl = e->comm != nullptr;
    e->tr_no_resident = false;  // (set when the resident tick fails over, for the rest of this run)
    struct Reset {
        mcs_engine* e;
        ~Reset() { e->tr_no_resident = false; }
    } reset{e};
    if (rccl) {
        dtrade_free(e);
        if (int s = dt_agree_shape(e)) return s;
    } else {
        e->dt_ns = 0;
    }
    uint32_t escalations = 0;
    double kms = 0.0;
    for (;;) {
        if (int s = dtrade_alloc(e)) return s;
        double ms = 0.0;
        int s = MCS_OK;
        if (rccl) {
            s = dt_run_rccl(e, &ms);
        } else if (dt_res_ok(e)) {
            s = dt_run_res(e, &ms);
            if (s == kDtResFallback) {  // (the run is redone from its start on the replayed kernels)
                e->tr_no_resident = true;
                s = dt_run_once(e, &ms);
                e->dtd->loop_form = kLoopGraphAfterTimeout;
            }
        } else {
            s = dt_run_once(e, &ms);
            if (e->tr_no_resident) e->dtd->loop_form = kLoopGraphAfterTimeout;
        }
        if (s) return s;
        kms += ms;
        if (int s = dt_poll(e)) return s;
        // ctl->flags is replicated (it ORs every cluster's record), so every rank escalates alike
        const uint32_t flags = e->dtd->h_ctl->flags;
        const uint32_t S = e->dtd->a.S, V = e->dtd->a.V;
        bool grow_s = (flags & MCS_FLAG_OVERFLOW) != 0, grow_v = (flags & MCS_FLAG_VNODE_OVERFLOW) != 0;
        if (!grow_s && !grow_v) break;
        if ((grow_s && (e->cfg.slot_pool || S >= kDtMaxSlots)) || (grow_v && V >= kDtMaxVnodes))
            return fail(e, MCS_E_CAPACITY, "DELAY trading capacity exhausted (slots or virtual nodes)");
        // slots grow by half (a multiple of 64): C5-DELAY peaks just above 256 (384, not 512, slots
        // for dt_step to stage through LDS every tick)
        const uint32_t ns = grow_s ? std::min<uint32_t>((S + S / 2u + 63u) / 64u * 64u, kDtMaxSlots) : S, nv = grow_v ? std::min<uint32_t>(V * 4u, kDtMaxVnodes) : V;
        dtrade_free(e);
        e->tr_slots = ns;
        e->dt_vnodes = nv;
        ++escalations;
    }
    e->dt_learn_s = e->cfg.slot_pool ? 0u : e->dtd->a.S;
    e->dt_learn_v = e->dtd->a.V;
    e->dtd->kernel_ms = kms;
    e->has_run = true;
    e->dtrade_run = true;
    e->trade_run = false;
    e->delay_run = true;
    if (stats) {
        std::vector<DtCluster> cl;
        if (int s = dt_clusters(e, cl)) return s;
        mcs_stats st{};
        st.jobs = e->total_jobs;
        for (uint32_t k = 0; k < e->C; ++k) {
            st.placed += cl[k].decided;
            st.waited += cl[k].moved;
        }
        st.unplaced = e->total_jobs - st.placed;
        st.clusters = e->C;
        st.escalations = escalations;
        st.slot_pool = e->dtd->a.S / 64u;
        st.kernel_ms = kms;
        st.wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - w0).count();
        *stats = st;
    }
    return MCS_OK;
}

// ---- caller-driven lock-step (mcs_trade_begin/xfer_bytes/phase/end with MCS_POLICY_DELAY) ----
// A tick is phase 0 (dt_step_kernel; out = this rank's exchange block) and phase 1 (in = every
// rank's block in rank order; dt_trader_kernel).  Phases 2 and 3 move no bytes; phase 3 reports
// done.  Every rank must hold the same cluster count and the same largest cluster (block layout).
int dtrade_begin(mcs_engine* e) {
    if (int s = dtrade_alloc(e)) return s;
    DtradeDev* d = e->dtd;
    d->w0 = std::chrono::steady_clock::now();
    const hipError_t st = launch_dtrade_init(d->a, e->stream);
    if (st != hipSuccess) return dt_hip_fail(e, "DELAY trading init", st);
    HIPCHK(e, hipStreamSynchronize(e->stream));
    HIPCHK(e, hipEventRecord(e->ev0, e->stream));
    d->begun = true;
    e->has_run = false;
    e->dtrade_run = false;
    return MCS_OK;
}

int dtrade_xfer_bytes(mcs_engine* e, uint32_t phase, uint64_t* in_bytes, uint64_t* out_bytes) {
    if (int s = dtrade_alloc(e)) return s;
    const uint64_t blk = e->dtd->a.blk;
    switch (phase) {
        case 0: *in_bytes = 0; *out_bytes = blk; break;
        case 1: *in_bytes = blk * e->world; *out_bytes = 0; break;
        default: *in_bytes = 0; *out_bytes = 0; break;
    }
    return MCS_OK;
}

int dtrade_phase(mcs_engine* e, uint32_t phase, const void* in, uint64_t in_bytes, void* out,
                 uint64_t out_bytes, uint32_t* done) {
    DtradeDev* d = e->dtd;
    if (!d || !d->begun) return fail(e, MCS_E_STATE, "mcs_trade_begin first");
    uint64_t ib = 0, ob = 0;
    if (int s = dtrade_xfer_bytes(e, phase, &ib, &ob)) return s;
    if (in_bytes != ib || out_bytes != ob || (ib && !in) || (ob && !out))
        return fail(e, MCS_E_INVALID, "exchange buffer sizes do not match mcs_trade_xfer_bytes");
    if (phase == 1) {  // every gathered block must carry this rank's layout tag
        const unsigned char* p = static_cast<const unsigned char*>(in);
        for (uint32_t r = 0; r < e->world; ++r)
            if (std::memcmp(p + (size_t)(r + 1u) * d->a.blk - kDtTagBytes, d->tag, kDtTagBytes) != 0)
                return fail(e, MCS_E_INVALID, "exchange block of rank " + std::to_string(r) +
                                                  " has another layout (stride or clusters): agree on the shape"
                                                  " with mcs_trade_set_shape");
    }
    hipError_t st = hipSuccess;
    switch (phase) {
        case 0:
            st = launch_dtrade_step(d->a, e->stream);
            if (st != hipSuccess) return dt_hip_fail(e, "dt_step_kernel", st);
            HIPCHK(e, hipMemcpyAsync(out, d->xb + (size_t)e->rank * d->a.blk, ob, hipMemcpyDeviceToHost, e->stream));
            break;
        case 1:
            HIPCHK(e, hipMemcpyAsync(d->xb, in, ib, hipMemcpyHostToDevice, e->stream));
            st = launch_dtrade_trader(d->a, e->stream);
            if (st != hipSuccess) return dt_hip_fail(e, "dt_trader_kernel", st);
            HIPCHK(e, hipMemcpyAsync(d->h_ctl, d->ctl, sizeof(DtCtl), hipMemcpyDeviceToHost, e->stream));
            break;
        default:
            break;
    }
    HIPCHK(e, hipStreamSynchronize(e->stream));
    if (phase == 0) std::memcpy(static_cast<unsigned char*>(out) + ob - kDtTagBytes, d->tag, kDtTagBytes);
    if (done) *done = phase == 3 ? d->h_ctl->done : 0u;
    return MCS_OK;
}

int dtrade_end(mcs_engine* e, mcs_stats* stats) {
    DtradeDev* d = e->dtd;
    if (!d || !d->begun) return fail(e, MCS_E_STATE, "mcs_trade_begin first");
    HIPCHK(e, hipEventRecord(e->ev1, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    d->begun = false;
    e->has_run = true;
    e->dtrade_run = true;
    e->trade_run = false;
    e->delay_run = true;
    if (int s = dt_poll(e)) return s;
    const uint32_t flags = d->h_ctl->flags;
    {
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, e->ev0, e->ev1) != hipSuccess) ms = 0.0f;
        d->kernel_ms = ms;
    }
    if (stats) {
        std::vector<DtCluster> cl;
        if (int s = dt_clusters(e, cl)) return s;
        mcs_stats st{};
        st.jobs = e->total_jobs;
        for (uint32_t k = 0; k < e->C; ++k) {
            st.placed += cl[k].decided;
            st.waited += cl[k].moved;
        }
        st.unplaced = e->total_jobs - st.placed;
        st.clusters = e->C;
        st.slot_pool = d->a.S / 64u;
        st.kernel_ms = d->kernel_ms;
        st.wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - d->w0).count();
        *stats = st;
    }
    if (flags & MCS_FLAG_OVERFLOW)
        return fail(e, MCS_E_CAPACITY, "running-slot pool overflow (raise mcs_config.slot_pool)");
    if (flags & MCS_FLAG_VNODE_OVERFLOW)
        return fail(e, MCS_E_CAPACITY, "virtual-node capacity overflow");
    return MCS_OK;
}

int dtrade_cluster_stats(mcs_engine* e, mcs_cluster_stats* out, uint32_t n) {
    std::vector<DtCluster> cl;
    if (int s = dt_clusters(e, cl)) return s;
    for (uint32_t k = 0; k < n; ++k) {
        mcs_cluster_stats s{};
        s.t_end = e->dtd->h_ctl->T;
        s.placed = cl[k].decided;
        s.waited = cl[k].moved;
        s.peak_running = cl[k].peak;
        s.flags = cl[k].flags;
        s.pool = e->dtd->a.S / 64u;
        s.iterations = e->dtd->h_ctl->ticks;
        s.release_scans = 0;
        out[k] = s;
    }
    return MCS_OK;
}

int dtrade_delay_stats(mcs_engine* e, mcs_delay_cluster_stats* out, uint32_t n) {
    std::vector<DtCluster> cl;
    if (int s = dt_clusters(e, cl)) return s;
    for (uint32_t k = 0; k < n; ++k) {
        mcs_delay_cluster_stats d{};
        d.total_wait_ms = cl[k].total;
        d.jobs_count = cl[k].count;
        d.moved_l1 = cl[k].moved;
        d.placed_l1 = cl[k].placed_l1;
        d.peak_l1 = 0;
        d.l1_left = cl[k].l1n;
        out[k] = d;
    }
    return MCS_OK;
}

int dtrade_trade_stats(mcs_engine* e, mcs_trade_stats* out) {
    std::vector<DtCluster> cl;
    if (int s = dt_clusters(e, cl)) return s;
    const DtCtl& c = *e->dtd->h_ctl;
    mcs_trade_stats s{};
    uint32_t flags = c.flags;
    for (uint32_t k = 0; k < e->C; ++k) {
        const uint64_t J = e->online ? e->job_cnt[k] : e->job_off[k + 1] - e->job_off[k];
        s.placed += cl[k].decided;
        s.waited += cl[k].moved;
        s.undecided += J - cl[k].decided;
        flags |= cl[k].flags;
    }
    if (c.n_trades > e->dtd->a.trade_cap || c.n_foreign > e->dtd->a.foreign_cap) flags |= MCS_FLAG_LOG_OVERFLOW;
    s.trades = c.n_trades;
    s.trades_won = c.n_won;
    s.ticks = c.ticks;
    s.t_final = c.T;
    s.flags = flags;
    s.loop_form = e->dtd->loop_form;
    s.kernel_ms = e->dtd->kernel_ms;
    s.block_bytes = e->dtd->a.blk;
    s.snaps = 1u;
    s.agreed = (e->comm || e->tr_agreed) ? 1u : 0u;
    *out = s;
    return MCS_OK;
}

int dtrade_read_trades(mcs_engine* e, mcs_trade_rec* out, uint64_t cap, uint64_t* n) {
    HIPCHK(e, hipStreamSynchronize(e->stream));
    HIPCHK(e, hipMemcpy(e->dtd->h_ctl, e->dtd->ctl, sizeof(DtCtl), hipMemcpyDeviceToHost));
    const uint64_t total = e->dtd->h_ctl->n_trades;
    const uint64_t k = std::min<uint64_t>(std::min<uint64_t>(total, e->dtd->a.trade_cap), cap);
    if (k) {
        std::vector<mcs_contract_rec> v(k);
        HIPCHK(e, hipMemcpy(v.data(), e->dtd->trades, k * sizeof(mcs_contract_rec), hipMemcpyDeviceToHost));
        for (uint64_t i = 0; i < k; ++i) out[i] = mcs_trade_rec{v[i].t_s, v[i].requester, v[i].winner, v[i].approvals};
    }
    *n = total;
    return MCS_OK;
}

int dtrade_read_vnode_counts(mcs_engine* e, uint32_t* out, uint32_t n) {
    HIPCHK(e, hipStreamSynchronize(e->stream));
    if (n) HIPCHK(e, hipMemcpy(out, e->dtd->nv_all, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return MCS_OK;
}

}  // namespace mcs

extern "C" {

int mcs_trade_session_info(mcs_engine* e, mcs_trade_session* out) {
    if (int st = check_engine(e)) return st;
    if (!out) return fail(e, MCS_E_INVALID, "null output");
    if (!mcs::is_trade_session(e))
        return fail(e, MCS_E_STATE, "no trading session (online mode with MCS_POLICY_DELAY and cfg.trader: mcs_run "
                                    "with a horizon, mcs_append_jobs, mcs_rewind)");
    mcs_trade_session s{};
    s.t_horizon = e->on_t_hor;
    s.t_last = e->ts_t_last;
    s.t_next = e->ts_ticks_total ? std::min(e->ts_t_next, e->ts_pend_min) : 0u;
    s.ticks_last_run = e->ts_ticks_last;
    s.ticks_total = e->ts_ticks_total;
    s.restarts = e->ts_restarts;
    s.drained = e->ts_drained ? 1u : 0u;
    s.failed = e->ts_failed ? 1u : 0u;
    *out = s;
    return MCS_OK;
}

// ---- external traders (DESIGN.md §14 "External traders") ------------------------------------------
int mcs_trade_external(mcs_engine* e, uint32_t on) {
    if (int st = check_engine(e)) return st;
    if (!e->has_clusters) return fail(e, MCS_E_STATE, "mcs_trade_external: mcs_load_clusters first");
    if (!mcs::is_dtrade(e) || e->cfg.borrow)
        return fail(e, MCS_E_STATE, "mcs_trade_external needs a DELAY trading system (MCS_POLICY_DELAY with "
                                    "cfg.trader = 1 and cfg.borrow = 0): FIFO trading and systems without "
                                    "traders have no virtual nodes to grant");
    if (e->world != 1 || e->rank != 0 || e->comm)
        return fail(e, MCS_E_STATE, "mcs_trade_external needs one engine that holds the whole system (rank 0 of "
                                    "world 1, no communicator): a sharded engine runs the built-in traders");
    if (e->dtd && e->dtd->begun)
        return fail(e, MCS_E_STATE, "mcs_trade_external: a caller-driven lock-step run is in progress "
                                    "(mcs_trade_end first)");
    if (e->online && e->ts_begun && e->ts_ticks_total != 0u)
        return fail(e, MCS_E_STATE, "mcs_trade_external: a lock-step tick of the current session has run (switch "
                                    "before the first mcs_run, right after mcs_rewind or after a new submit)");
    e->dt_external = on != 0u;
    if (e->dtd) {  // (a captured graph holds the kernels' arguments by value)
        mcs::dtrade_release_graphs(e);
        e->dtd->a.period = e->dt_external ? 0u : e->cfg.trader_period_s;
    }
    return MCS_OK;
}

int mcs_trade_session_provide_vnodes(mcs_engine* e, const mcs_vnode_request* req, uint32_t n,
                                     mcs_vnode_result* res, mcs_vnode_stats* stats) {
    if (int st = check_engine(e)) return st;
    if (stats) *stats = mcs_vnode_stats{};
    if (int st = mcs::dt_grant_check(e, "mcs_trade_session_provide_vnodes")) return st;
    if (n == 0) return MCS_OK;
    if (!req || !res) return fail(e, MCS_E_INVALID, "null requests or results");
    if (n > 4096u) return fail(e, MCS_E_INVALID, "more than 4096 requests in one call");
    for (uint32_t i = 0; i < n; ++i) {
        if (req[i].responder >= e->C || req[i].requester >= e->C)
            return fail(e, MCS_E_INVALID, "request " + std::to_string(i) + ": responder or requester out of range");
        if ((uint64_t)e->ts_t_last + req[i].time_s > 0xFFFFFFFEull)
            return fail(e, MCS_E_INVALID, "request " + std::to_string(i) + ": t_last + time_s lies past second "
                                              "0xFFFFFFFE");
    }
    mcs::DtGrantCall call;
    call.req.assign(req, req + n);
    return mcs::dt_grant_call(e, std::move(call), res, stats);
}

int mcs_trade_session_receive_vnodes(mcs_engine* e, const mcs_vnode_grant* node, uint32_t n, mcs_vnode_stats* stats) {
    if (int st = check_engine(e)) return st;
    if (stats) *stats = mcs_vnode_stats{};
    if (int st = mcs::dt_grant_check(e, "mcs_trade_session_receive_vnodes")) return st;
    if (n == 0) return MCS_OK;
    if (!node) return fail(e, MCS_E_INVALID, "null nodes");
    if (n > 4096u) return fail(e, MCS_E_INVALID, "more than 4096 nodes in one call");
    for (uint32_t i = 0; i < n; ++i)
        if (node[i].cluster >= e->C)
            return fail(e, MCS_E_INVALID, "node " + std::to_string(i) + ": cluster index out of range");
    mcs::DtGrantCall call;
    call.node.assign(node, node + n);
    return mcs::dt_grant_call(e, std::move(call), nullptr, stats);
}

int mcs_trade_session_read_nodes(mcs_engine* e, uint32_t cluster, uint64_t* free_cores, uint64_t* free_memory,
                                 uint32_t cap, uint32_t* n) {
    if (int st = check_engine(e)) return st;
    if (!n || (cap && (!free_cores || !free_memory))) return fail(e, MCS_E_INVALID, "bad output");
    if (!mcs::is_trade_session(e))
        return fail(e, MCS_E_STATE, "mcs_trade_session_read_nodes reads a trading session (online mode with "
                                    "MCS_POLICY_DELAY and cfg.trader): there is no trading session");
    if (e->ts_failed)
        return fail(e, MCS_E_STATE, "mcs_trade_session_read_nodes: the trading session failed (capacity exhausted)");
    if (!e->ts_begun || !e->dtd || e->ts_ticks_total == 0u)
        return fail(e, MCS_E_STATE, "mcs_trade_session_read_nodes reads the state the last executed tick left: no "
                                    "tick has been executed yet (mcs_run first)");
    if (cluster >= e->C) return fail(e, MCS_E_INVALID, "cluster index out of range");
    mcs::DtradeDev* d = e->dtd;
    mcs::DtCluster k{};
    HIPCHK(e, hipStreamSynchronize(e->stream));
    HIPCHK(e, hipMemcpy(&k, d->cl + cluster, sizeof(k), hipMemcpyDeviceToHost));
    const uint32_t N = e->node_off[cluster + 1] - e->node_off[cluster], nv = std::min(k.nv, d->a.V);
    std::vector<unsigned long long> v((size_t)N + nv + 1u);
    if (N) HIPCHK(e, hipMemcpy(v.data(), d->tn + e->node_off[cluster], (size_t)N * 8, hipMemcpyDeviceToHost));
    if (nv) HIPCHK(e, hipMemcpy(v.data() + N, d->vn + (size_t)cluster * d->a.V, (size_t)nv * 8, hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < N + nv && i < cap; ++i) {  // Go uint64: the sign-extended u32 halves
        free_cores[i] = (uint64_t)(int64_t)(int32_t)(uint32_t)v[i];
        free_memory[i] = (uint64_t)(int64_t)(int32_t)(uint32_t)(v[i] >> 32);
    }
    *n = N + nv;
    return MCS_OK;
}

int mcs_read_contracts(mcs_engine* e, mcs_contract_rec* out, uint64_t cap, uint64_t* n) {
    if (int st = check_engine(e)) return st;
    if (!n || (cap && !out)) return fail(e, MCS_E_INVALID, "bad output");
    if (!e->dtrade_run || !e->dtd) return fail(e, MCS_E_STATE, "no DELAY trading run");
    mcs::DtradeDev* d = e->dtd;
    HIPCHK(e, hipStreamSynchronize(e->stream));
    HIPCHK(e, hipMemcpy(d->h_ctl, d->ctl, sizeof(mcs::DtCtl), hipMemcpyDeviceToHost));
    const uint64_t total = d->h_ctl->n_trades;
    const uint64_t k = std::min<uint64_t>(std::min<uint64_t>(total, d->a.trade_cap), cap);
    if (k) HIPCHK(e, hipMemcpy(out, d->trades, k * sizeof(mcs_contract_rec), hipMemcpyDeviceToHost));
    *n = total;
    return MCS_OK;
}

int mcs_read_foreign(mcs_engine* e, mcs_foreign_rec* out, uint64_t cap, uint64_t* n) {
    if (int st = check_engine(e)) return st;
    if (!n || (cap && !out)) return fail(e, MCS_E_INVALID, "bad output");
    if (!e->dtrade_run || !e->dtd) return fail(e, MCS_E_STATE, "no DELAY trading run");
    mcs::DtradeDev* d = e->dtd;
    HIPCHK(e, hipStreamSynchronize(e->stream));
    HIPCHK(e, hipMemcpy(d->h_ctl, d->ctl, sizeof(mcs::DtCtl), hipMemcpyDeviceToHost));
    const uint64_t total = d->h_ctl->n_foreign;
    const uint64_t k = std::min<uint64_t>(std::min<uint64_t>(total, d->a.foreign_cap), cap);
    if (k) HIPCHK(e, hipMemcpy(out, d->foreign, k * sizeof(mcs_foreign_rec), hipMemcpyDeviceToHost));
    *n = total;
    return MCS_OK;
}

int mcs_read_virtual_node_caps(mcs_engine* e, uint32_t cluster, uint32_t* cores, uint32_t* mem,
                               uint32_t cap, uint32_t* n) {
    if (int st = check_engine(e)) return st;
    if (!n || (cap && (!cores || !mem))) return fail(e, MCS_E_INVALID, "bad output");
    if (!e->dtrade_run || !e->dtd) return fail(e, MCS_E_STATE, "no DELAY trading run");
    if (cluster >= e->C) return fail(e, MCS_E_INVALID, "cluster index out of range");
    mcs::DtradeDev* d = e->dtd;
    mcs::DtCluster k{};
    HIPCHK(e, hipStreamSynchronize(e->stream));
    HIPCHK(e, hipMemcpy(&k, d->cl + cluster, sizeof(k), hipMemcpyDeviceToHost));
    const uint32_t m = std::min<uint32_t>(std::min<uint32_t>(k.nv, d->a.V), cap);
    if (m) {
        std::vector<uint2> v(m);
        HIPCHK(e, hipMemcpy(v.data(), d->vcap + (size_t)cluster * d->a.V, m * sizeof(uint2), hipMemcpyDeviceToHost));
        for (uint32_t i = 0; i < m; ++i) {
            cores[i] = v[i].x;
            mem[i] = v[i].y;
        }
    }
    *n = k.nv;
    return MCS_OK;
}

}  // extern "C"

static int dt_state_series(mcs_engine* e, uint32_t t0_s, uint32_t period_s, uint32_t n_samples,
                           mcs_cluster_sample* out, mcs_wait_sample* wait, mcs_cluster_state* first,
                           uint32_t n_clusters, double* kernel_ms, bool seg, uint32_t hor);

// the run's flags (dt_clusters has just read the control block): the telemetry refuses a run that an
// overflow cut short or whose logs dropped records
static int dt_flags_check(mcs_engine* e, const std::vector<mcs::DtCluster>& cl) {
    const mcs::DtradeDev* d = e->dtd;
    const mcs::DtCtl ctl = *d->h_ctl;
    uint32_t flags = ctl.flags;
    for (uint32_t k = 0; k < e->C; ++k) flags |= cl[k].flags;
    if (flags & (MCS_FLAG_OVERFLOW | MCS_FLAG_VNODE_OVERFLOW))
        return fail(e, MCS_E_STATE, "cluster states of a DELAY trading run that a slot-pool overflow or a "
                                    "virtual-node overflow (MCS_FLAG_VNODE_OVERFLOW) cut short");
    if ((flags & MCS_FLAG_LOG_OVERFLOW) || ctl.n_foreign > d->a.foreign_cap || ctl.n_trades > d->a.trade_cap)
        return fail(e, MCS_E_STATE, "cluster states of a DELAY trading run whose Foreign or contract log "
                                    "overflowed (MCS_FLAG_LOG_OVERFLOW): records were dropped");
    return MCS_OK;
}

extern "C" {

// The ClusterState record and the wait statistics of a DELAY trading run: the third
// form of the state kernels (mcs_state.hip, dt_*) over the placements, the virtual-node table and the
// Foreign log, and the wait_*_kernels over the placements.
int mcs_dtrade_state_series(mcs_engine* e, uint32_t t0_s, uint32_t period_s, uint32_t n_samples,
                            mcs_cluster_sample* out, mcs_wait_sample* wait, mcs_cluster_state* first,
                            uint32_t n_clusters, double* kernel_ms) {
    if (int st = check_engine(e)) return st;
    if (int st = mcs::refuse_trade_session(e, "mcs_dtrade_state_series")) return st;
    if (e->segmented)
        return fail(e, MCS_E_STATE, "cluster states are rebuilt from batch runs (not after mcs_append_jobs; "
                                    "in an online session: mcs_online_state_series)");
    if (!e->has_run) return fail(e, MCS_E_STATE, "mcs_run first");
    if (!e->dtrade_run || !e->dtd)
        return fail(e, MCS_E_STATE, "mcs_dtrade_state_series reads a DELAY trading run (MCS_POLICY_DELAY with "
                                    "cfg.trader); after any other run: mcs_cluster_state_series and "
                                    "mcs_wait_time_series (mcs.h)");
    if (e->world != 1)
        return fail(e, MCS_E_STATE, "cluster states of a sharded DELAY trading run: the placements of the other "
                                    "ranks' clusters live there (run the system on one engine)");
    return dt_state_series(e, t0_s, period_s, n_samples, out, wait, first, n_clusters, kernel_ms, false, MCS_TIME_NONE);
}

}  // extern "C"

// A session's call compacts the Foreign log (dt_foreign_live_kernel) when the direct scan it replaces is at
// least this many scan rounds: a workgroup reads the log in rounds of 256 records, once per tile of the call.
// The pre-pass (a 4-byte fill and a launch) costs 3.6 us and a round 0.2 us, so it pays from 18 rounds on:
// a one-tile call over a log of 4353 records, or 18 tiles over a log of up to 256 (DESIGN.md §14 has the
// measurement; below the break-even the direct scan was faster by more than the spread between rounds).
// The two costs are a model fitted to calls of 1, 8 and 40 tiles over logs of at most 232 records, one
// round per tile: the pre-pass lost at 8 rounds and won at 40, nothing was measured between them or with
// several rounds per tile, so the 4353 records are an extrapolation.  A heuristic: it takes the tile
// count of the widest cluster (max_nn) for all, and either choice returns the same bytes.
static constexpr uint64_t kDtForeignFilterMinRounds = 18;

// The body of mcs_dtrade_state_series behind its state checks.  seg: a trading session
// (mcs_trade_session_state_series): the SEG kernels over the session's segments, the virtual-node table
// and the Foreign log as the last mcs_run left them; hor is then the decided frontier (MCS_TIME_NONE
// after a drain, and for a batch run), checked after the argument checks of mcs_cluster_state_series.
static int dt_state_series(mcs_engine* e, uint32_t t0_s, uint32_t period_s, uint32_t n_samples,
                           mcs_cluster_sample* out, mcs_wait_sample* wait, mcs_cluster_state* first,
                           uint32_t n_clusters, double* kernel_ms, bool seg, uint32_t hor) {
    mcs::DtradeDev* d = e->dtd;
    std::vector<mcs::DtCluster> cl;
    if (int st = mcs::dt_clusters(e, cl)) return st;
    const mcs::DtCtl ctl = *d->h_ctl;
    if (int st = dt_flags_check(e, cl)) return st;
    if (!out || n_clusters > e->C) return fail(e, MCS_E_INVALID, "bad output");
    if (period_s == 0 || n_samples == 0) return fail(e, MCS_E_INVALID, "period_s and n_samples must be positive");
    if ((uint64_t)t0_s + (uint64_t)(n_samples - 1) * period_s > 0xFFFFFFFEull)
        return fail(e, MCS_E_INVALID, "the last sample lies past second 0xFFFFFFFE");
    if (ctl.n_foreign > 0xFFFFFFFEull) return fail(e, MCS_E_INVALID, "more than 2^32 - 2 Foreign jobs");
    if (hor != MCS_TIME_NONE && (uint64_t)t0_s + (uint64_t)(n_samples - 1) * period_s >= hor)
        return fail(e, MCS_E_INVALID, "the last sample lies at or past the last horizon " + std::to_string(hor) +
                                          ": only samples below it are decided");
    if (int st = mcs::ensure_job_records(e)) return st;
    if (n_clusters == 0) {
        if (kernel_ms) *kernel_ms = 0.0;
        return MCS_OK;
    }
    double total_ms = 0.0;
    if (wait) {  // (its own argument checks repeat the ones above and add the per-cluster job limit)
        double ms = 0.0;
        if (int st = mcs::wait_series(e, t0_s, period_s, n_samples, wait, n_clusters, &ms, seg)) return st;
        total_ms += ms;
    }
    const uint32_t V = d->a.V;
    std::vector<uint32_t> nv(e->C);
    uint32_t max_nn = 1;
    for (uint32_t k = 0; k < e->C; ++k) {
        nv[k] = std::min(cl[k].nv, V);
        max_nn = std::max(max_nn, e->node_off[k + 1] - e->node_off[k] + nv[k]);
    }
    // samples per launch: the device buffer stays within 256 MiB (MCS_SERIES_CHUNK overrides the count)
    uint64_t chunk = (256ull << 20) / (sizeof(mcs_cluster_sample) * (uint64_t)n_clusters);
    if (const char* env = getenv("MCS_SERIES_CHUNK"))
        if (atoll(env) > 0) chunk = (uint64_t)atoll(env);
    if (chunk < 1) chunk = 1;
    if (chunk > n_samples) chunk = n_samples;
    uint32_t* d_nv = nullptr;
    mcs_cluster_sample* d_out = nullptr;
    mcs_cluster_state* d_first = nullptr;
    uint2* d_summ = nullptr;
    mcs_foreign_rec* d_live = nullptr;  // a session's call: the Foreign records that can hold at one of its samples
    uint32_t* d_live_n = nullptr;
    const uint32_t n_foreign = (uint32_t)ctl.n_foreign;
    const uint64_t scan_rounds = ((uint64_t)n_foreign + 255u) / 256u *
                                 (((uint64_t)n_samples + mcs::dt_series_tile(max_nn) - 1u) / mcs::dt_series_tile(max_nn));
    const bool filter = seg && n_foreign > 0 &&
                        (e->dt_foreign_filter < 0 ? scan_rounds >= kDtForeignFilterMinRounds : e->dt_foreign_filter != 0);
    hipError_t st = hipMalloc(&d_nv, e->C * sizeof(uint32_t));
    if (st == hipSuccess) st = hipMemcpy(d_nv, nv.data(), e->C * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (st == hipSuccess) st = hipMalloc(&d_out, (size_t)n_clusters * chunk * sizeof(mcs_cluster_sample));
    // (over segments with slack the summaries are indexed by capacity: series_summ_size)
    const uint64_t rows = seg ? e->job_off[e->C] : e->total_jobs;
    if (st == hipSuccess) st = hipMalloc(&d_summ, mcs::series_summ_size(rows, e->C) * sizeof(uint2));
    if (st == hipSuccess && first) st = hipMalloc(&d_first, n_clusters * sizeof(mcs_cluster_state));
    if (st == hipSuccess && filter) st = hipMalloc(&d_live, (size_t)n_foreign * sizeof(mcs_foreign_rec));
    if (st == hipSuccess && filter) st = hipMalloc(&d_live_n, sizeof(uint32_t));
    mcs::DtSeriesArgs a{};
    a.d.s.node_off = e->d_node_off;
    a.d.s.cap = e->d_cap;
    a.d.s.free0 = e->d_free0;
    a.d.s.jobs = e->d_jobs;
    a.d.s.job_off = e->d_job_off;
    a.d.s.out_node = e->d_out_node;
    a.d.s.out_start = e->d_out_start;
    a.d.s.out_finish = e->d_out_finish;
    a.d.s.out = d_first;
    a.d.s.t = t0_s;
    a.d.s.n_clusters = n_clusters;
    a.d.s.job_cnt = seg ? e->d_job_cnt : nullptr;
    a.d.vcap = d->vcap;
    a.d.nv = d_nv;
    a.d.flog = d->foreign;
    a.d.n_foreign = n_foreign;
    a.d.V = V;
    a.summ = d_summ;
    a.out = d_out;
    a.period = period_s;
    a.magic = period_s > 1 ? ~0ull / period_s + 1ull : 0ull;
    for (uint64_t k0 = 0; st == hipSuccess && k0 < n_samples; k0 += chunk) {
        const uint32_t nk = (uint32_t)(n_samples - k0 < chunk ? n_samples - k0 : chunk);
        a.t0 = (uint32_t)(t0_s + k0 * period_s);
        a.n_samples = nk;
        st = hipEventRecord(e->ev0, e->stream);
        if (st == hipSuccess && k0 == 0) {
            // the stream's first message: a plain scan at t0_s, independent of the tile walk
            if (first) st = mcs::launch_dt_state(a.d, max_nn, e->stream);
            if (st == hipSuccess) st = mcs::launch_dt_series_summary(a, e->stream);
            if (st == hipSuccess && filter) {  // once per call: the bounds are those of all its chunks
                st = mcs::launch_dt_foreign_live(d->foreign, n_foreign, t0_s,
                                                 (uint32_t)(t0_s + (uint64_t)(n_samples - 1) * period_s), d_live,
                                                 d_live_n, e->stream);
                a.live = d_live;
                a.live_n = d_live_n;
            }
        }
        if (st == hipSuccess) st = mcs::launch_dt_state_series(a, max_nn, e->stream);
        if (st == hipSuccess) st = hipEventRecord(e->ev1, e->stream);
        if (st == hipSuccess) st = hipStreamSynchronize(e->stream);
        float ms = 0.0f;
        if (st == hipSuccess) st = hipEventElapsedTime(&ms, e->ev0, e->ev1);
        total_ms += ms;
        if (st == hipSuccess)  // the chunk's columns of every cluster's row
            st = hipMemcpy2D(out + k0, (size_t)n_samples * sizeof(mcs_cluster_sample), d_out,
                             (size_t)nk * sizeof(mcs_cluster_sample), (size_t)nk * sizeof(mcs_cluster_sample),
                             n_clusters, hipMemcpyDeviceToHost);
    }
    if (st == hipSuccess && first)
        st = hipMemcpy(first, d_first, n_clusters * sizeof(mcs_cluster_state), hipMemcpyDeviceToHost);
    (void)hipFree(d_nv);
    (void)hipFree(d_out);
    (void)hipFree(d_summ);
    if (d_first) (void)hipFree(d_first);
    if (d_live) (void)hipFree(d_live);
    if (d_live_n) (void)hipFree(d_live_n);
    if (st != hipSuccess) return fail(e, MCS_E_HIP, std::string("DELAY trading state series: ") + hipGetErrorString(st));
    if (kernel_ms) *kernel_ms = total_ms;
    return MCS_OK;
}

// what both calls of a trading session check before their arguments: a session whose rows are as its
// last mcs_run left them
static int trade_session_series_check(mcs_engine* e, const char* call) {
    const std::string c(call);
    if (!mcs::is_trade_session(e))
        return fail(e, MCS_E_STATE, c + " reads a trading session (online mode with MCS_POLICY_DELAY and "
                                        "cfg.trader: mcs_run with a horizon, mcs_append_jobs); there is no trading "
                                        "session (after a batch DELAY trading run: mcs_dtrade_state_series, "
                                        "mcs_level1_series; in a session without trading: mcs_online_state_series, "
                                        "mcs_online_level1_series)");
    if (e->ts_failed)
        return fail(e, MCS_E_STATE, c + ": the trading session failed (capacity exhausted, MCS_E_CAPACITY): "
                                        "mcs_rewind or submit again, then run");
    if (!e->has_run || !e->dtrade_run || !e->dtd || !e->d_job_cnt)
        return fail(e, MCS_E_STATE, c + " reads the session as its last mcs_run left it: run first (no run since "
                                        "the session began or since mcs_rewind)");
    if (!e->on_series_ok)
        return fail(e, MCS_E_STATE, c + " reads the session as its last mcs_run left it: run first (the last run "
                                        "failed, or jobs were appended behind a drain and no run has seen them)");
    return MCS_OK;
}

extern "C" {

// The Start stream of a trading session (DESIGN.md §14 "The Start stream of a trading session"): the
// record of mcs_dtrade_state_series read from the session as its last mcs_run left it.  Nothing is kept
// between calls: the summaries, the wait records and the compacted Foreign list are rebuilt by every
// call and freed with it.
int mcs_trade_session_state_series(mcs_engine* e, uint32_t t0_s, uint32_t period_s, uint32_t n_samples,
                                   mcs_cluster_sample* out, mcs_wait_sample* wait, mcs_cluster_state* first,
                                   uint32_t n_clusters, double* kernel_ms) {
    if (int st = check_engine(e)) return st;
    if (int st = trade_session_series_check(e, "mcs_trade_session_state_series")) return st;
    return dt_state_series(e, t0_s, period_s, n_samples, out, wait, first, n_clusters, kernel_ms, true,
                           e->on_series_hor);
}

// ProvideJobs' view of a trading session: mcs_online_level1_series' kernels over the session's rows
// (Level1 depends on arrivals, starts and max_wait_s alone), under the same frontier.
int mcs_trade_session_level1_series(mcs_engine* e, uint32_t t0_s, uint32_t period_s, uint32_t n_samples,
                                    mcs_level1_sample* out, uint32_t n_clusters, double* kernel_ms) {
    if (int st = check_engine(e)) return st;
    if (int st = trade_session_series_check(e, "mcs_trade_session_level1_series")) return st;
    {  // the run's flags refuse as they do for the state series
        std::vector<mcs::DtCluster> cl;
        if (int st = mcs::dt_clusters(e, cl)) return st;
        if (int st = dt_flags_check(e, cl)) return st;
    }
    if (int st = mcs::series_args_check(e, t0_s, period_s, n_samples, out, n_clusters)) return st;
    const uint32_t h = e->on_series_hor;
    if (h != MCS_TIME_NONE && (uint64_t)t0_s + (uint64_t)(n_samples - 1) * period_s >= h)
        return fail(e, MCS_E_INVALID, "the last sample lies at or past the last horizon " + std::to_string(h) +
                                          ": only samples below it are decided");
    return mcs::level1_series(e, t0_s, period_s, n_samples, out, n_clusters, kernel_ms, true);
}

int mcs_approve_trade(mcs_engine* e, const mcs_approve_query* q, uint32_t n, int32_t* out) {
    if (int st = check_engine(e)) return st;
    if (n && (!q || !out)) return fail(e, MCS_E_INVALID, "null query or output");
    if (!n) return MCS_OK;
    mcs_approve_query* dq = nullptr;
    int32_t* dout = nullptr;
    hipError_t st = hipMalloc(&dq, n * sizeof(mcs_approve_query));
    if (st == hipSuccess) st = hipMalloc(&dout, n * sizeof(int32_t));
    if (st == hipSuccess) st = hipMemcpy(dq, q, n * sizeof(mcs_approve_query), hipMemcpyHostToDevice);
    if (st == hipSuccess) st = mcs::launch_approve(dq, n, dout, e->stream);
    if (st == hipSuccess) st = hipStreamSynchronize(e->stream);
    if (st == hipSuccess) st = hipMemcpy(out, dout, n * sizeof(int32_t), hipMemcpyDeviceToHost);
    if (dq) (void)hipFree(dq);
    if (dout) (void)hipFree(dout);
    if (st != hipSuccess) return fail(e, MCS_E_HIP, std::string("approve_trade: ") + hipGetErrorString(st));
    return MCS_OK;
}

}  // extern "C"
