// mcs_trade_dev.h — device code of the FIFO lock-step trading tick shared by its four
// loops: the replayed kernels (mcs_trade.hip), the one-workgroup resident tick (mcs_trade_res.hip),
// the workgroup-resident tick (mcs_trade_mw.hip) and the one-launch tick (mcs_trade_rk.hip).  The
// tick restates three Go functions, each written once here: Scheduler.Fifo's step over the Wait /
// Ready / Lent queues (tr_fifo_step), RequestPolicyMonitor's trader rounds (tr_trader_rounds, one lane
// per cluster; tr_trader_rounds_lds past 64 clusters) and the next tick's clock (tr_next_tick).  A
// kernel supplies what differs per form: where a job record, a fitting node, a running slot and the
// LentQueue head come from, and where a lent run's record goes.
#pragma once
#include "mcs_trade_internal.h"
#include "mcs_trader_dev.h"
#include "mcs_wave.h"

namespace mcs {
namespace {

// ---- phase A's cluster state ----
// The register-resident forms hold word f of the cluster's TrCluster in lane f of one VGPR: uniform
// reads are v_readlane, writes a lane select (never under a lane-divergent branch).
constexpr uint32_t kStWords = sizeof(TrCluster) / 4u;
static_assert(sizeof(TrCluster) % 4u == 0u && kStWords <= (uint32_t)kWave, "TrCluster in one VGPR");
struct LaneWord {
    uint32_t& v;
    uint32_t f, lane;
    __device__ __forceinline__ operator uint32_t() const { return readlane(v, f); }
    __device__ __forceinline__ LaneWord& operator=(uint32_t x) {
        v = lane == f ? x : v;
        return *this;
    }
    __device__ __forceinline__ LaneWord& operator=(const LaneWord& o) { return *this = (uint32_t)o; }
    __device__ __forceinline__ LaneWord& operator+=(uint32_t x) { return *this = (uint32_t)*this + x; }
    __device__ __forceinline__ LaneWord& operator-=(uint32_t x) { return *this = (uint32_t)*this - x; }
    __device__ __forceinline__ LaneWord& operator|=(uint32_t x) { return *this = (uint32_t)*this | x; }
    __device__ __forceinline__ LaneWord& operator++() { return *this += 1u; }
    __device__ __forceinline__ LaneWord& operator--() { return *this -= 1u; }
    __device__ __forceinline__ uint32_t operator++(int) {
        const uint32_t o = *this;
        *this = o + 1u;
        return o;
    }
};
// the two views TR_ST reads a field through: the VGPR above, or a plain TrCluster in registers
// (tr_step_kernel); `st` names the view in scope
struct TrLaneState {
    uint32_t& v;
    uint32_t lane;
    template <typename M>
    __device__ __forceinline__ LaneWord f(M TrCluster::*, uint32_t w) const {
        return LaneWord{v, w, lane};
    }
};
struct TrRegState {
    TrCluster& s;
    __device__ __forceinline__ uint32_t& f(uint32_t TrCluster::*m, uint32_t) const { return s.*m; }
};
#define TR_ST(field) (st.f(&TrCluster::field, (uint32_t)(offsetof(TrCluster, field) / 4u)))

// ---- arrivals up to T join the ReadyQueue (jobs are sorted by arrival) ----
// awin holds the arrival seconds of the W jobs from `na` on (kEmpty past J) in lanes wl .. wl + W - 1,
// loaded ahead; a burst past a full window loads the records it passes directly.  Returns the first
// job not yet queued and its arrival second (kEmpty: none).
struct TrArrivals {
    uint32_t next_arr, nat;
};
template <uint32_t W>
__device__ __forceinline__ TrArrivals tr_arrivals(uint32_t T, uint32_t lane, uint32_t wl, uint32_t na,
                                                  uint32_t awin, const uint4* __restrict__ jobs, uint32_t J) {
    unsigned long long in = __ballot(awin <= T && na + (lane & (W - 1u)) < J);
    if constexpr (W < (uint32_t)kWave) in = (in >> wl) & ((1ull << W) - 1ull);
    const uint32_t n = (uint32_t)__builtin_popcountll(in);
    na += n;
    if (n < W) return TrArrivals{na, readlane(awin, wl + n)};
    while (na < J) {
        const uint32_t i = na + lane;
        const bool ok = i < J && jobs[i].x <= T;
        const uint32_t m = (uint32_t)__builtin_popcountll(__ballot(ok));
        na += m;
        if (m < (uint32_t)kWave) break;
    }
    return TrArrivals{na, na < J ? jobs[na].x : kEmpty};
}

// ---- the cluster's scheduler step at tick T (Scheduler.Fifo, scheduler.go:216-296) ----
// ops, the per-form part:
//   job(j)                      -> uint4 record {arrival, dur, c, m} of the cluster's job j
//   first_fit(c, m)             -> ScheduleJob's node (kEmpty: none fits)
//   commit(node, c, m, finish)  -> Node.RunJob + the running-slot insert; false on slot overflow
//   lent_head()                 -> the LentQueue head entry
//   lent_run(b, j, node, fin)   -> the lent run's record: logged at once, or kept for the log index
//                                  the exchange gives it
struct TrLent {
    uint32_t borrower, job, c, m, dur;
};
template <typename J, typename F, typename C, typename H, typename R>
struct TrStepOps {
    J job;
    F first_fit;
    C commit;
    H lent_head;
    R lent_run;
};
template <typename J, typename F, typename C, typename H, typename R>
__device__ __forceinline__ TrStepOps<J, F, C, H, R> tr_step_ops(J job, F first_fit, C commit, H lent_head, R lent_run) {
    return TrStepOps<J, F, C, H, R>{job, first_fit, commit, lent_head, lent_run};
}
struct TrStepOut {
    TrRecA req;  // the tick's borrow request (job == kEmpty: none)
    bool lent;   // a lent job started this tick
};
template <typename St, typename Ops>
__device__ __forceinline__ TrStepOut tr_fifo_step(const TradeArgs& a, uint32_t T, uint32_t lane, uint64_t j0, St st,
                                                  Ops& ops) {
    auto place_own = [&](uint32_t j, uint32_t k, uint4 jb) -> bool {
        const uint32_t fin = T + jb.y;
        if (jb.y != 0u && !ops.commit(k, jb.z, jb.w, fin)) return false;
        if (lane == 0) {
            a.out_node[j0 + j] = (int32_t)k;
            a.out_start[j0 + j] = T;
            a.out_finish[j0 + j] = fin;
        }
        ++TR_ST(placed);
        ++TR_ST(decided);
        return true;
    };
    TrStepOut o{TrRecA{kEmpty, 0u, 0u, 0u}, false};
    for (;;) {
        if (TR_ST(has_w)) {  // WaitQueue head (scheduler.go:219-251)
            const uint4 jb = ops.job(TR_ST(w));
            const uint32_t k = ops.first_fit(jb.z, jb.w);
            if (k != kEmpty) {
                if (!place_own(TR_ST(w), k, jb)) {
                    TR_ST(flags) |= MCS_FLAG_OVERFLOW;
                    break;
                }
                TR_ST(has_w) = 0u;
            } else if (a.borrow) {
                o.req = TrRecA{TR_ST(w), jb.z, jb.w, jb.y};  // BorrowResources (:234)
            }
            break;  // time.Sleep(1 s), :250
        }
        if (TR_ST(rq_head) < TR_ST(next_arr)) {  // ReadyQueue head (:255-272), no sleep
            const uint32_t j = TR_ST(rq_head)++;
            const uint4 jb = ops.job(j);
            const uint32_t k = ops.first_fit(jb.z, jb.w);
            if (k != kEmpty) {
                if (!place_own(j, k, jb)) {
                    TR_ST(flags) |= MCS_FLAG_OVERFLOW;
                    break;
                }
            } else {
                TR_ST(has_w) = 1u;
                TR_ST(w) = j;
                ++TR_ST(waited);
            }
            continue;
        }
        if (TR_ST(lq_len) > 0u) {  // LentQueue head (:277-290)
            const TrLent e = ops.lent_head();
            const uint32_t k = ops.first_fit(e.c, e.m);
            if (k != kEmpty) {
                const uint32_t fin = T + e.dur;
                if (e.dur != 0u && !ops.commit(k, e.c, e.m, fin)) {
                    TR_ST(flags) |= MCS_FLAG_OVERFLOW;
                    break;
                }
                ops.lent_run(e.borrower, e.job, k, fin);
                o.lent = true;
                ++TR_ST(lent_runs);
                TR_ST(lq_head) = TR_ST(lq_head) + 1u == a.LQ ? 0u : TR_ST(lq_head) + 1u;
                --TR_ST(lq_len);
            }
            break;  // sleep 1 s (:289)
        }
        break;  // idle sleep (:294)
    }
    return o;
}

// the LentQueue head entry as the resident forms prefetch it: lanes 0-2 of lqw hold its first
// three 8-byte words {borrower | job << 32, c | m << 32, dur}
__device__ __forceinline__ TrLent tr_lent_from_lanes(unsigned long long lqw) {
    const uint32_t lo = (uint32_t)lqw, hi = (uint32_t)(lqw >> 32);
    return TrLent{readlane(lo, 0), readlane(hi, 0), readlane(lo, 1), readlane(hi, 1), readlane(lo, 2)};
}

__device__ __forceinline__ void tr_log_trade(const TradeArgs& a, unsigned long long at, uint32_t T, uint32_t q,
                                             uint32_t winner, uint32_t napp) {
    mcs_trade_rec rec;
    rec.t_s = T;
    rec.requester = q;
    rec.winner = winner == kEmpty ? -1 : (int32_t)winner;
    rec.approvals = napp;
    a.trade_log[at] = rec;
}

// ---- the trader rounds of tick T, one lane per cluster of the system (at most 64) ----
// Lane g holds cluster g's trader state t and its utilization sample, fixed for the tick (`in`:
// g < C_t).  A due requester that is not over the utilization threshold only moves its own due time
// (all of them at once); the others run their RequestResource rounds in index order, each a ballot
// over the responders' lock states.  The counters and lflags stay wave-uniform; the wave with `log`
// writes the trade log.
struct TrSample {
    float cu, mu;
    uint32_t total_c, total_m;
};
__device__ __forceinline__ void tr_trader_rounds(const TradeArgs& a, uint32_t T, uint32_t g, bool in,
                                                 const TrSample& s, bool log, TrTrader& t,
                                                 unsigned long long& n_trades, unsigned long long& n_won,
                                                 uint32_t& lflags) {
    const bool due = in && t.next_due <= T;
    // policies [WaitTime, Utilization] (trader.go:55-62): WaitTime never breaks under FIFO (its
    // average is only fed by /delay); Utilization (trader.go:127-130)
    const bool broken = s.cu > 0.8f || s.mu > 0.8f;
    if (due && !broken) t.next_due = T + a.period;
    // ApproveTrade (trader.go:141-167) of the contract {cores 0, mem 0, time 0 s, price 0} that every
    // FIFO trade carries (the small-node contract over an empty Level1), by this lane as a responder
    const bool appr = in && approve_trade_dev(s.total_c, s.total_m, s.cu, s.mu, 0u, 0u, 0u);
    unsigned long long pend = __ballot(due && broken);
    while (pend) {  // RequestPolicyMonitor of requester q (trader.go:282-324), index order
        const uint32_t q = (uint32_t)__builtin_ctzll(pend);
        pend &= pend - 1ull;
        bool app = false;
        if (in && g != q) {  // Trade (trader.go:193-278): RequestResource to every other trader
            if (t.lock_id != 0u && T >= t.lock_until) t.lock_id = 0u;  // 20 s expiry
            if (t.lock_id == 0u) {  // else Approve:false (server.go:35-40)
                app = appr;
                t.lock_id = t.next_id++;  // set even when not approving (:44-46)
                t.lock_until = T + a.lock_s;
            }
        }
        // every response echoes the requester's price (server.go:44): the Go heap of equal keys pops
        // the first push first (Appendix C), whose lock still matches (nothing intervenes), and the
        // zero allocation cannot fail -> first approver
        const unsigned long long ab = __ballot(app);
        const uint32_t napp = (uint32_t)__builtin_popcountll(ab);
        const uint32_t winner = ab ? (uint32_t)__builtin_ctzll(ab) : kEmpty;
        if (winner != kEmpty) {
            if (g == winner) t.lock_id = 0u;  // ApproveContract resets currentContract (:83)
            if (g == q) t.vnodes += 1u;       // AddVirtualNode(0 cores, 0 memory)
            ++n_won;
        }
        if (g == q) t.next_due = T + (winner != kEmpty ? a.ok_sleep : a.fail_sleep) + a.period;
        if (n_trades >= a.trade_cap) lflags |= MCS_FLAG_LOG_OVERFLOW;
        else if (log && g == 0u) tr_log_trade(a, n_trades, T, q, winner, napp);
        ++n_trades;
    }
}

// The same rounds for a system of more than 64 clusters (tr_trader_kernel, one wave, up to
// kTrMaxClusters): the trader state and the samples in LDS, requesters and responders 64 at a time.
__device__ __forceinline__ void tr_trader_rounds_lds(const TradeArgs& a, uint32_t T, uint32_t lane, TrTrader* trs,
                                                     const TrRecC* rcs, unsigned long long& n_trades,
                                                     unsigned long long& n_won, uint32_t& lflags) {
    const uint32_t Ct = a.Ct;
    for (uint32_t q0 = 0; q0 < Ct; q0 += kWave) {
        const uint32_t ql = q0 + lane;
        unsigned long long due = __ballot(ql < Ct && trs[ql].next_due <= T);
        while (due) {  // RequestPolicyMonitor of requester q, index order
            const uint32_t q = q0 + (uint32_t)__builtin_ctzll(due);
            due &= due - 1ull;
            const TrRecC rq = rcs[q];
            const bool broken = rq.cu > 0.8f || rq.mu > 0.8f;
            if (!broken) {
                if (lane == 0) trs[q].next_due = T + a.period;
                __syncthreads();
                continue;
            }
            uint32_t napp = 0, winner = kEmpty;
            for (uint32_t r0 = 0; r0 < Ct; r0 += kWave) {  // RequestResource, index order
                const uint32_t r = r0 + lane;
                bool app = false;
                if (r < Ct && r != q) {
                    TrTrader t = trs[r];
                    if (t.lock_id != 0u && T >= t.lock_until) t.lock_id = 0u;
                    if (t.lock_id == 0u) {
                        const TrRecC rr = rcs[r];
                        app = approve_trade_dev(rr.total_c, rr.total_m, rr.cu, rr.mu, 0u, 0u, 0u);
                        t.lock_id = t.next_id++;
                        t.lock_until = T + a.lock_s;
                    }
                    trs[r] = t;
                }
                const unsigned long long ab = __ballot(app);
                napp += (uint32_t)__builtin_popcountll(ab);
                if (winner == kEmpty && ab) winner = r0 + (uint32_t)__builtin_ctzll(ab);  // first approver
            }
            __syncthreads();
            if (lane == 0) {
                if (winner != kEmpty) {
                    trs[winner].lock_id = 0u;
                    trs[q].vnodes += 1u;
                    ++n_won;
                }
                if (n_trades < a.trade_cap) tr_log_trade(a, n_trades, T, q, winner, napp);
                else lflags |= MCS_FLAG_LOG_OVERFLOW;
                trs[q].next_due = T + (winner != kEmpty ? a.ok_sleep : a.fail_sleep) + a.period;
            }
            ++n_trades;
            __syncthreads();
        }
    }
}

// ---- the next tick: T + 1 while any queue is busy, else the next arrival or trader round ----
// flags: the run's flags with this tick's; nxt: the earliest next arrival or trader round (kEmpty:
// none).  tmax_now: this tick raised MCS_FLAG_T_MAX.
struct TrNext {
    uint32_t Tn, done, flags, tmax_now;
};
__device__ __forceinline__ TrNext tr_next_tick(uint32_t T, uint32_t t_max, bool done_all, bool busy_any,
                                               uint32_t nxt, uint32_t flags) {
    const uint32_t fatal = MCS_FLAG_OVERFLOW | MCS_FLAG_LENT_OVERFLOW;
    if (done_all || (flags & fatal)) return TrNext{T, 1u, flags, 0u};
    if (T >= t_max || (!busy_any && nxt == kEmpty)) return TrNext{T, 1u, flags | MCS_FLAG_T_MAX, 1u};
    return TrNext{(busy_any || nxt <= T + 1u) ? T + 1u : nxt, 0u, flags, 0u};
}

// ---- host: the resident kernels' launch ----
// the <4> / <8> / <16> slot-row instantiation for S running slots per cluster, with its dynamic LDS
template <typename... P, typename... Args>
inline hipError_t launch_by_rows(void (*k4)(P...), void (*k8)(P...), void (*k16)(P...), uint32_t S, dim3 grid,
                                 dim3 block, size_t lds, hipStream_t s, Args... args) {
    void (*const fn)(P...) = S == 4u * kWave ? k4 : S == 8u * kWave ? k8 : k16;
    const hipError_t st = hipFuncSetAttribute(reinterpret_cast<const void*>(fn),
                                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (st != hipSuccess) return st;
    hipLaunchKernelGGL(fn, grid, block, lds, s, args...);
    return hipGetLastError();
}

}  // namespace
}  // namespace mcs
