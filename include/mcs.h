/*
 * mcs.h — C ABI of the MI355X batched FIFO placement engine (libmcs.so).
 *
 * Drop-in boundary for the data-parallel hot path of hamzalsheikh/multi-cluster-simulator
 * (reference snapshot 2024-10-16).  The reference has no FFI: the path is a set of Go methods on
 * a global singleton.  Each entry point below names the reference symbol it replaces
 * (path:line relative to the reference root).  A Go cgo binding is shown in INTEGRATION.md.
 *
 * Rules of the ABI:
 *   - plain C99, no C++ types, no callbacks; every call is blocking;
 *   - the caller owns every host array; the engine copies inputs in during the call and never
 *     keeps host pointers; the engine owns all device memory and frees it in mcs_engine_destroy;
 *   - a handle is NOT thread-safe: one host thread (one cgo goroutine) per handle, one handle per GPU;
 *   - status codes are ints (mcs_status); details via mcs_last_error(); no exception crosses the ABI.
 *
 * Units: every time is a whole number of SECONDS in a uint32 (deviation D8 of SURVEY Appendix A:
 * the reference only produces whole seconds — pkg/client/client.go:98 and all sleeps).
 */
#ifndef MCS_H
#define MCS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MCS_ABI_VERSION 7

/* ---- status codes --------------------------------------------------------------------------- */
typedef enum mcs_status {
    MCS_OK = 0,
    /* ScheduleJob's error "not enough resources in cluster" (pkg/scheduler/scheduler.go:138) */
    MCS_NO_FIT = 1,
    MCS_E_INVALID = -1,  /* bad argument / inconsistent sizes                                     */
    MCS_E_CAPACITY = -2, /* running-slot pool overflow that survived capacity escalation          */
    MCS_E_HIP = -3,      /* a HIP runtime call failed                                             */
    MCS_E_RCCL = -4,     /* an RCCL call failed                                                   */
    MCS_E_STATE = -5,    /* call out of order (e.g. mcs_run before mcs_load_clusters)             */
    MCS_E_NOMEM = -6,    /* host or device allocation failed                                      */
    MCS_E_RANGE = -7     /* a cluster's simulated clock left the uint32 seconds range (D8): the run
                            stopped there; MCS_FLAG_CLOCK_OVERFLOW marks it and its undecided jobs
                            read MCS_NODE_UNPLACED / MCS_TIME_NONE                                 */
} mcs_status;

/* Node index written for a job that is never placed (head-of-line deadlock: the wait-queue head
 * cannot fit even on an empty cluster, so the reference's Fifo loop retries it forever,
 * scheduler.go:219-251).  start/finish are then MCS_TIME_NONE. */
#define MCS_NODE_UNPLACED (-1)
/* Node index written for a job moved to the BorrowedQueue (scheduler.go:237-242; mcs_trade.h):
 * start = the borrow tick, finish = MCS_TIME_NONE; the lender's run is in mcs_read_lent. */
#define MCS_NODE_BORROWED (-2)
#define MCS_TIME_NONE 0xFFFFFFFFu

/* per-cluster flag bits (mcs_cluster_stats.flags) */
#define MCS_FLAG_DEADLOCK 0x1u /* head-of-line job can never fit; rest of the stream unplaced     */
#define MCS_FLAG_OVERFLOW 0x2u /* running-slot pool overflow (engine re-runs with a larger pool)   */
#define MCS_FLAG_CLOCK_OVERFLOW 0x4u /* the uint32 seconds clock would wrap; results after it invalid */
#define MCS_FLAG_LENT_OVERFLOW 0x8u  /* a LentQueue exceeded lent_queue_cap (lock-step runs)          */
#define MCS_FLAG_LOG_OVERFLOW 0x10u  /* lent/trade log capacity exceeded: records dropped, counts kept */
#define MCS_FLAG_T_MAX 0x20u         /* lock-step run stopped at t_max_s with work left               */
#define MCS_FLAG_VNODE_OVERFLOW 0x40u /* DELAY trading: a cluster received more virtual nodes than the
                                         engine holds (engine re-runs with more)                      */

/* ---- configuration ------------------------------------------------------------------------- */
typedef enum mcs_policy {
    MCS_POLICY_FIFO = 0,  /* Scheduler.Fifo (scheduler.go:216-296); selected by config (D4)       */
    MCS_POLICY_DELAY = 1  /* Scheduler.Delay (scheduler.go:298-369), the reference default (:116);
                             serialized semantics SDELAY; ABI v3                   */
} mcs_policy;

typedef struct mcs_config {
    uint32_t policy;         /* mcs_policy                                                         */
    uint32_t borrow;         /* FIFO cross-cluster borrow (server.go:160-248; mcs_trade.h)          */
    uint32_t trader;         /* trader offer exchange (trader.go:193-325; mcs_trade.h)              */
    uint32_t wait_sleep_s;   /* sleep after a wait-queue attempt, scheduler.go:250 (must be 1)     */
    uint32_t idle_sleep_s;   /* sleep when all queues are empty, scheduler.go:294 (must be 1)      */
    uint32_t slot_pool;      /* running-slot pool per cluster in units of 64 (0 = auto)            */
    /* lock-step trading cadences (used when borrow or trader is set; mcs_trade.h) */
    uint32_t trader_period_s;    /* 10: time.Sleep(10 s) per monitor pass, trader.go:323            */
    uint32_t trade_ok_sleep_s;   /* 240: after a successful trade, trader.go:297                    */
    uint32_t trade_fail_sleep_s; /* 120: after a failed trade, trader.go:300                        */
    uint32_t lock_s;             /* 20: responder contract lock, pkg/trader/server.go:48-57         */
    uint32_t sample_period_s;    /* 5: scheduler state stream period, trader_server.go:44           */
    uint32_t lent_queue_cap;     /* LentQueue entries per cluster (0 = 4096)                        */
    uint32_t t_max_s;            /* stop the lock-step clock after this tick (0 = 0xFFFFFFFE)       */
    uint32_t max_wait_s;         /* DELAY: Policy.MaxWaitTime, 10 s (scheduler.go:115,353)          */
    uint32_t unchecked_horizon;  /* 0 (default): mcs_submit_jobs / mcs_generate_jobs / mcs_append_jobs
                                    reject streams whose clock bound (last arrival + sum of (dur + 1
                                    [+ max_wait_s under DELAY])) leaves the uint32 range.  1: skip that
                                    check (tests of the device-side guard: the kernels then stop the
                                    cluster with MCS_FLAG_CLOCK_OVERFLOW and mcs_run returns
                                    MCS_E_RANGE).  Not allowed with borrow or trader (the lock-step
                                    kernels have no such guard): mcs_engine_create returns
                                    MCS_E_INVALID                                                    */
    uint32_t reserved[1];
} mcs_config;

/* Fills the reference defaults (FIFO, no borrow, no trader, 1 s sleeps, trader cadences above). */
void mcs_config_default(mcs_config* cfg);

/* ---- synthetic job stream (input synthesis; restates pkg/client/client.go:85-147) ----------- */
typedef enum mcs_arrival_mode {
    MCS_ARRIVAL_REF = 0,    /* per minute n ~ Poisson(lambda), spacing floor(60/n) s (client.go:107-125);
                               n == 0 is an idle minute of 60 s (D5)                                 */
    MCS_ARRIVAL_SCALED = 1, /* per second n ~ Poisson(lambda) arrivals at that second               */
    MCS_ARRIVAL_WEIBULL = 2 /* the client's "weibull" mode (client.go:131-145): after each job a sleep of
                               floor(X) s, X ~ Weibull(scale lambda, shape weibull_k); the reference
                               uses Lambda 10, K 3 (gonum distuv.Weibull)                          */
} mcs_arrival_mode;

typedef struct mcs_gen_params {
    uint64_t seed;        /* base seed; cluster k uses key = mix(seed ^ k)                           */
    uint32_t arrival_mode;/* mcs_arrival_mode                                                        */
    uint32_t max_dur_s;   /* durations U{0..max_dur_s-1}; 600 = rand.Intn(600) (client.go:98)        */
    double lambda;        /* Poisson mean per minute (REF, 10 in client.go:108) or per second (SCALED);
                             WEIBULL: the scale (Lambda: 10, client.go:133)                          */
    uint32_t max_cores;   /* 0 = per-cluster max node Cores (setMaxCluster, client.go:68-83)          */
    uint32_t max_mem;     /* 0 = per-cluster max node Memory                                          */
    uint32_t fused;       /* 1: no job records in HBM; the FIFO/DELAY kernels synthesise each 64-job
                             batch in registers, bit-identical to the records;
                             mcs_read_jobs and the trading paths materialise them on demand      */
    float weibull_k;      /* WEIBULL: the shape (K: 3, client.go:134); 0 = 3                          */
    uint32_t reserved[2];
} mcs_gen_params;

void mcs_gen_params_default(mcs_gen_params* p);

/* Host generator (same arithmetic as the device generator, bit-identical output).  Generates the
 * jobs of ONE cluster (index `cluster`) with the given max cores/mem. */
int mcs_gen_cluster_host(const mcs_gen_params* p, uint32_t cluster, uint32_t max_cores,
                         uint32_t max_mem, uint64_t n_jobs, uint32_t* arrival_s, uint32_t* dur_s,
                         uint32_t* cores, uint32_t* mem);

/* Per-second lambda giving `load` offered memory load for n_nodes nodes of node_mem memory
 * (SCALED mode): lambda = load * n_nodes * node_mem / (E[mem] * E[dur]). */
double mcs_gen_scaled_lambda(uint32_t n_nodes, uint32_t node_mem, uint32_t max_mem,
                             uint32_t max_dur_s, double load);

/* ---- engine ---------------------------------------------------------------------------------- */
typedef struct mcs_engine mcs_engine;

typedef struct mcs_stats {
    uint64_t jobs;          /* jobs in the submitted streams                                     */
    uint64_t placed;        /* jobs placed on a node                                             */
    uint64_t waited;        /* jobs that entered the wait queue (scheduler.go:264-268)           */
    uint64_t unplaced;      /* jobs never placed (deadlocked clusters)                           */
    uint32_t clusters;
    uint32_t deadlocked;    /* clusters with MCS_FLAG_DEADLOCK                                   */
    uint32_t escalations;   /* slot-pool re-runs performed                                       */
    uint32_t slot_pool;     /* largest slot pool used (x64)                                      */
    double kernel_ms;       /* device time of the placement kernel(s), HIP events on the engine stream */
    double wall_ms;         /* host wall time of the whole mcs_run call                           */
    uint64_t pending;       /* online runs: jobs not decided yet (queued, or arriving later)       */
    uint32_t t_horizon;     /* online runs: the horizon reached (MCS_TIME_NONE after a drain)      */
    uint32_t online;        /* 1 if this run continued an online session (finite horizons)         */
    uint32_t handed_over;   /* DELAY, ABI v6: clusters the hand-scheduled loop handed to the compiled
                               delay_kernel (re-run from t = 0: Level1 past its LDS slice, the clock
                               range after a move, or a runaway guard of the loop)                           */
    uint32_t reserved;
} mcs_stats;

typedef struct mcs_cluster_stats {
    uint32_t t_end;         /* simulated clock when the cluster's queues drained (seconds)       */
    uint32_t placed;
    uint32_t waited;
    uint32_t peak_running;  /* peak jobs holding resources (dur > 0)                              */
    uint32_t flags;         /* MCS_FLAG_*                                                         */
    uint32_t pool;          /* slot pool (x64) the final result was produced with                */
    uint32_t iterations;    /* diagnostics: decision-loop passes (the hand-scheduled loop counts the
                               passes without a decision only with MCS_FIFO_DIAG=1 in the env)     */
    uint32_t release_scans; /* diagnostics: clock advances that released running jobs (ditto)    */
} mcs_cluster_stats;

/* DELAY-policy statistics of one cluster (MCS_POLICY_DELAY runs; mcs_read_delay_stats). */
typedef struct mcs_delay_cluster_stats {
    int64_t total_wait_ms;  /* WaitTime.TotalTime at t_end (scheduler.go:48-54,309-312,338-341):
                               1000 * (start - arrival) per placed job, 1000 * (t_end - arrival)
                               per job left in Level1                                             */
    int64_t jobs_count;     /* WaitTime.JobsCount: jobs received by "/delay" (server.go:72)         */
    uint32_t moved_l1;      /* Level0 -> Level1 moves after MaxWaitTime (scheduler.go:353-359)      */
    uint32_t placed_l1;     /* placements made by the Level1 pass (scheduler.go:302-329)           */
    uint32_t peak_l1;       /* peak len(Level1)                                                    */
    uint32_t l1_left;       /* Level1 jobs that can never fit (MCS_FLAG_DEADLOCK)                  */
} mcs_delay_cluster_stats;

/* scheduler.Run (scheduler.go:101-124) builds a Scheduler; here one engine batches many clusters
 * on ONE GPU (`device` = HIP ordinal). */
int mcs_engine_create(const mcs_config* cfg, int device, mcs_engine** out);
int mcs_engine_destroy(mcs_engine* eng);
const char* mcs_last_error(const mcs_engine* eng);
int mcs_abi_version(void);
/* Name of the placement kernel the last mcs_run launched first ("mcs::fifo_asm_kernel",
 * "mcs::fifo_kernel", "mcs::delay_kernel"; "" before any run): lets a caller match its timings
 * to a rocprofv3 kernel trace.  Owned by the engine. */
const char* mcs_last_kernel(const mcs_engine* eng);

/* Cluster specs (assets/cluster_*.json, Cluster/Node in pkg/scheduler/cluster.go:14-24,127-138):
 * nodes of cluster c are [node_offsets[c], node_offsets[c+1]) in JSON array order; free_* are the
 * JSON CoresAvailable/MemoryAvailable, kept as-is by Run (scheduler.go:101-109, KAT5).
 * At most 1024 nodes per cluster in ABI v1. */
int mcs_load_clusters(mcs_engine* eng, const uint32_t* cap_c, const uint32_t* cap_m,
                      const uint32_t* free_c, const uint32_t* free_m,
                      const uint32_t* node_offsets, uint32_t n_clusters);

/* Job streams (the ReadyQueue filled by the "/" handler, server.go:23-51): jobs of cluster c are
 * [job_offsets[c], job_offsets[c+1]), sorted by arrival (non-decreasing); job id = index. */
int mcs_submit_jobs(mcs_engine* eng, const uint32_t* arrival_s, const uint32_t* dur_s,
                    const uint32_t* cores, const uint32_t* mem, const uint64_t* job_offsets);

/* Same as mcs_submit_jobs but synthesises n_jobs per cluster on the device (bit-identical to
 * mcs_gen_cluster_host for every cluster).  With p->fused the records are never stored: every
 * FIFO/DELAY run regenerates them inside the placement kernels. */
int mcs_generate_jobs(mcs_engine* eng, const mcs_gen_params* p, uint64_t jobs_per_cluster);

/* Copies the (submitted or generated) job streams back to the host (sizes from the offsets). */
int mcs_read_jobs(mcs_engine* eng, uint32_t* arrival_s, uint32_t* dur_s, uint32_t* cores,
                  uint32_t* mem);

/* Runs the configured policy loop for every cluster over ScheduleJob (scheduler.go:127-139) and
 * Node.RunJob (cluster.go:141-161):
 *   MCS_POLICY_FIFO  — Scheduler.Fifo (scheduler.go:216-296), serialized semantics SFIFO
 *                      (SURVEY Appendix A); with cfg.borrow or cfg.trader set the clusters instead
 *                      advance in lock-step with the borrow and trade exchanges (mcs_trade.h);
 *   MCS_POLICY_DELAY — Scheduler.Delay (scheduler.go:298-369) with jobs ingested by the "/delay"
 *                      handler (server.go:53-78), serialized semantics SDELAY.
 *                      MCS_FLAG_DEADLOCK marks clusters whose Level1 keeps jobs that can never
 *                      fit; those jobs get MCS_NODE_UNPLACED and every other job is placed.
 *
 * Batch mode (the default after mcs_submit_jobs / mcs_generate_jobs): t_end_s = MCS_TIME_NONE runs
 * every cluster from its loaded spec until every job is decided; repeated calls repeat the run.
 *
 * Online mode (FIFO / DELAY without trading) replaces the reference's infinite loop
 * fed by HTTP POSTs (scheduler.go:216-296, 298-369; server.go:23-78): a finite t_end_s, or any
 * mcs_append_jobs, starts a session that keeps each cluster's state (clock, queues, node counters,
 * running jobs) on the device between calls.  mcs_run(t_end_s) then makes every decision the Go
 * loop makes at simulated seconds t < t_end_s and stops there; mcs_run(MCS_TIME_NONE) continues
 * until every job appended so far is decided (a drain).  Horizons are non-decreasing.  Jobs
 * appended after mcs_run(h) must arrive at or after h (they are POSTed after that moment).  Splitting
 * a run into horizons, with the jobs appended between them, gives bit-for-bit the placements of
 * the batch run over all the jobs.  Between horizons the placements of undecided jobs read
 * MCS_NODE_UNPLACED / MCS_TIME_NONE; the cluster and DELAY statistics are final after a drain.
 * Returns MCS_E_RANGE (results readable) when a cluster's clock leaves the uint32 range.
 *
 * With MCS_POLICY_DELAY and cfg.trader on one engine the session is a trading session (mcs_trade.h,
 * "trading sessions"): mcs_run(t_end_s) executes every lock-step tick T < t_end_s
 * of the trading system, and does not stop at "every job so far decided" (samples and trader rounds go
 * on); a horizon above t_max_s + 1 is MCS_E_INVALID.  FIFO trading (cfg.borrow, or cfg.trader under
 * MCS_POLICY_FIFO) has no online mode: a finite t_end_s is MCS_E_INVALID there. */
int mcs_run(mcs_engine* eng, uint32_t t_end_s, mcs_stats* stats);

/* Online mode: append jobs to the clusters' streams (the "/" or "/delay" handler appending to the
 * ReadyQueue / Level0, server.go:38-41,67-69).  Jobs of cluster c are [job_offsets[c],
 * job_offsets[c+1]) of the given arrays, arrival-sorted, each arrival >= the cluster's last one,
 * >= the last finite horizon run, and >= the cluster's own clock after the last drain (a cluster
 * whose drain ended earlier accepts earlier arrivals than one that ran longer).  Their ids continue the cluster's stream (dense order of
 * mcs_read_placements: per cluster, submitted then appended jobs in order).  Starts an online
 * session (state at t = 0) if none is active.  In a trading session (MCS_POLICY_DELAY with cfg.trader,
 * mcs_trade.h) the lock-step clock is common to all clusters: each arrival must also lie above the
 * last executed tick, so after a drain that ended at tick T_d the floor is T_d + 1 for every cluster.
 * MCS_E_STATE with FIFO trading (cfg.borrow, or cfg.trader under MCS_POLICY_FIFO), and for DELAY
 * trading on a sharded engine or one with a communicator. */
int mcs_append_jobs(mcs_engine* eng, const uint32_t* arrival_s, const uint32_t* dur_s,
                    const uint32_t* cores, const uint32_t* mem, const uint64_t* job_offsets);

/* Online mode: restart the session at t = 0 with every job submitted and appended so far. */
int mcs_rewind(mcs_engine* eng);

/* Dense CSR of the current streams (n_clusters + 1 entries): jobs of cluster c are rows
 * [off[c], off[c+1]) of mcs_read_placements / mcs_read_jobs. */
int mcs_read_job_offsets(mcs_engine* eng, uint64_t* off);

/* Where the streams sit on the device (n_clusters + 1 entries): cluster c's segment starts at row
 * off[c] and has room for off[c + 1] - off[c] jobs, of which mcs_read_job_offsets counts those it
 * holds.  Without an append the segments are the dense streams; an append that does not fit moves
 * every segment, which this call makes visible.  Diagnostic: no other call takes
 * these offsets. */
int mcs_read_segment_offsets(mcs_engine* eng, uint64_t* off);

/* Per-job results of the last mcs_run, indexed like the submitted jobs. */
int mcs_read_placements(mcs_engine* eng, int32_t* node, uint32_t* start_s, uint32_t* finish_s);
int mcs_read_cluster_stats(mcs_engine* eng, mcs_cluster_stats* out, uint32_t n_clusters);
/* DELAY statistics of the last MCS_POLICY_DELAY run (MCS_E_STATE after a FIFO run). */
int mcs_read_delay_stats(mcs_engine* eng, mcs_delay_cluster_stats* out, uint32_t n_clusters);

uint32_t mcs_num_clusters(const mcs_engine* eng);
uint64_t mcs_num_jobs(const mcs_engine* eng);

/* ---- single-job mirrors (live cluster state, initialised from the spec at load time) -------- */
/* Scheduler.ScheduleJob (scheduler.go:127-139) with the commit of Node.RunJob (cluster.go:144-148)
 * done synchronously (D2): first node in order with CoresAvailable >= cores && MemoryAvailable >=
 * mem.  Returns MCS_OK and *node, or MCS_NO_FIT with *node = MCS_NODE_UNPLACED. */
int mcs_schedule_one(mcs_engine* eng, uint32_t cluster, uint32_t cores, uint32_t mem,
                     int32_t* node);
/* The completion half of Node.RunJob (cluster.go:153-157): node gives back cores/mem. */
int mcs_release_one(mcs_engine* eng, uint32_t cluster, uint32_t node, uint32_t cores,
                    uint32_t mem);
/* Scheduler.Lend (scheduler.go:194-202): strict '>' existence test, no commit. */
int mcs_lend_check(mcs_engine* eng, uint32_t cluster, uint32_t cores, uint32_t mem, int32_t* ok);
/* Live free vectors of one cluster (n = node count of the cluster). */
int mcs_read_live_state(mcs_engine* eng, uint32_t cluster, uint32_t* free_c, uint32_t* free_m,
                        uint32_t n);
/* Cluster.GetResourceUtilization (cluster.go:46-63) over the live state: float32 sums in node
 * order divided by float32 totals (SetTotalResources, cluster.go:26-40). */
int mcs_resource_utilization(mcs_engine* eng, uint32_t cluster, float* core_util,
                             float* mem_util);

/* ---- the ClusterState record as a batched reduction ---------------------- */
/* pb.ClusterState (resource-channel.proto:27-34) that each cluster's Start stream
 * (trader_server.go:24-47) would send at simulated second t_s, rebuilt from the last FIFO/DELAY
 * run's placements: the counters after second t_s (jobs with start <= t_s < finish hold their
 * node), GetResourceUtilization over them (cluster.go:46-63, float32 in node order) and the Run
 * totals (cluster.go:26-40).
 * After a FIFO trading run (MCS_POLICY_FIFO with borrow and/or trader; mcs_run or mcs_trade_begin ..
 * mcs_trade_end) the record is defined by the own placements plus the lent runs (mcs_read_lent):
 *   - a node is also held by every lent run whose lender is this cluster and whose
 *     start_s <= t_s < finish_s, with the cores and memory of job `job` of cluster `borrower`
 *     (scheduler.go:277-290); a zero-duration run holds nothing;
 *   - running counts the own jobs and the lent runs holding at t_s;
 *   - a job moved to the BorrowedQueue (MCS_NODE_BORROWED) is never running on its own cluster;
 *   - a node index at or above the physical node count is a zero-capacity virtual node
 *     (AddVirtualNode, cluster.go:65-85), which only a 0-core 0-memory job takes: the record counts
 *     as running and adds to no node.  Utilization sums the physical nodes and divides by the Run
 *     totals: a virtual node's term is float32(0) - float32(0) = +0 and the totals are not
 *     recomputed (cluster.go:79), so virtual nodes change no bit;
 *   - in the lock-step order of a tick (scheduler steps, borrow exchange, state samples, trader
 *     rounds; mcs_trade.h) "the counters after second t_s" is the sample the Start stream sends at a
 *     sample tick t_s.
 * After a plain run an index >= the node count reads as unplaced, as it always did.
 * average_wait_time (trader_server.go:39) is not in this record: under
 * DELAY it is mcs_wait_time_series at t_s (the value at the end of the run: mcs_read_delay_stats),
 * under FIFO it is 0, since only "/delay" feeds WaitTime. */
typedef struct mcs_cluster_state {
    float cores_utilization;
    float memory_utilization;
    uint32_t total_cpu;
    uint32_t total_memory;
    uint32_t running;   /* jobs holding resources at t_s */
    uint32_t t_s;
} mcs_cluster_state;

/* One gfx950 launch over every cluster.  MCS_E_STATE, with the cause in mcs_last_error: before a run;
 * after mcs_append_jobs (an online session is served by mcs_online_state_series, below); after a
 * DELAY trading run (Foreign jobs, wrapped counters and virtual nodes with capacity are not in this
 * record: mcs_dtrade_state_series, mcs_trade.h, returns the record that has them); after a FIFO
 * trading run on a sharded engine (a lent record
 * does not carry the job's cores and memory, and the borrower's job records live on another rank),
 * one whose lent log overflowed (MCS_FLAG_LOG_OVERFLOW: records were dropped) or one cut short by a
 * slot-pool or LentQueue overflow.  The first call after a FIFO trading run sorts the lent log by
 * lender on the device (kept until the next run).  kernel_ms (may be NULL) receives the device time
 * of the launches from HIP events on the engine stream. */
int mcs_cluster_states(mcs_engine* eng, uint32_t t_s, mcs_cluster_state* out, uint32_t n_clusters,
                       double* kernel_ms);

/* ---- the ClusterState time series: the whole Start stream in one call ----------------------- */
/* One sample of the telemetry the reference produces over time: traderServer.Start sends a
 * ClusterState every 5 s (trader_server.go:24-47), RunMetrics samples every 5 s (metrics.go:25-30).
 * queued is the _jobs_in_queue counter of the DELAY path: it rises at "/delay" ingestion
 * (server.go:75) and falls at each placement (scheduler.go:320,348).  The engine reports it with
 * this one definition under FIFO as well; the reference never moves the counter under FIFO.
 * A zero-duration job is queued on [arrival, start) and never running; an unplaced job stays queued
 * for every t_k >= arrival.  average_wait_time, the stream's last field, is a series of its own,
 * mcs_wait_time_series below: WaitTime depends on each pending job's last attempt, which follows
 * from the arrivals and starts of the whole stream up to t, not from the jobs placed at t. */
typedef struct mcs_cluster_sample {   /* 16 B */
    float cores_utilization;          /* as mcs_cluster_state, at t_k                        */
    float memory_utilization;
    uint32_t running;                 /* jobs with start <= t_k < finish (after a FIFO trading run:
                                         own jobs and lent runs, see mcs_cluster_state)       */
    uint32_t queued;                  /* jobs with arrival <= t_k that have not started by t_k:
                                         start > t_k, or never placed (MCS_NODE_UNPLACED).  After a
                                         FIFO trading run: own jobs that have not left the Ready and
                                         Wait queues by t_k.  A borrowed job (MCS_NODE_BORROWED,
                                         start = the borrow tick) is queued on [arrival, start); a
                                         job undecided at t_max_s stays queued; LentQueue entries,
                                         the lender's foreign work, are not counted             */
} mcs_cluster_sample;

/* Every sample t_k = t0_s + k * period_s, k < n_samples, of every cluster from one pass over the
 * last FIFO/DELAY run's placements: sample k is bit for bit what mcs_cluster_states(eng, t_k)
 * returns for cores_utilization, memory_utilization and running (float32 sums in node order).
 * out[c * n_samples + k] is cluster c at t_k.  first (may be NULL) receives the full record at t0_s:
 * the stream's first message, the only one that carries the totals (trader_server.go:28-34).
 * The preconditions are those of mcs_cluster_states (MCS_E_STATE before a run, after
 * mcs_append_jobs, after a DELAY trading run, and after a FIFO trading run that was sharded or
 * overflowed); after a FIFO trading run the samples follow the trading semantics stated there.  MCS_E_INVALID: period_s == 0, n_samples == 0, out == NULL, n_clusters
 * above the engine's count, or a last sample past 0xFFFFFFFE.  kernel_ms (may be NULL) receives
 * the summed device time of the launches. */
int mcs_cluster_state_series(mcs_engine* eng, uint32_t t0_s, uint32_t period_s, uint32_t n_samples,
                             mcs_cluster_sample* out, mcs_cluster_state* first, uint32_t n_clusters,
                             double* kernel_ms);

/* ---- the average wait time series of a DELAY run: the Start stream's last field -------------- */
/* ClusterState.AverageWaitTime (trader_server.go:39), the value the trader's WaitTime policy reads
 * (trader.go:138) and RunMetrics records every 5 s (metrics.go:25-30): the scheduler's WaitTime
 * (scheduler.go:47-63) after the Delay iteration at simulated second t (SDELAY, DESIGN.md §10:
 * releases, arrivals, the Level1 pass, the Level0 head). */
typedef struct mcs_wait_sample {      /* 24 B */
    double average_wait_time;         /* WaitTime.GetAverage() (scheduler.go:56-63), milliseconds:
                                         (double)total_wait_ms / (double)jobs_count, 0 for no jobs */
    int64_t total_wait_ms;            /* WaitTime.TotalTime                                       */
    int64_t jobs_count;               /* WaitTime.JobsCount: arrivals <= t (server.go:72)          */
} mcs_wait_sample;

/* Every sample t_k = t0_s + k * period_s, k < n_samples, of every cluster, rebuilt on the GPU from the
 * last DELAY run's arrivals and starts and the engine's max_wait_s: the Level1
 * removal without i-- (D6) is followed, so an entry stepped over at t_k keeps its earlier value.
 * out[c * n_samples + k] is cluster c at t_k.  The Go loop is continued past the run's end: a cluster
 * whose jobs are all placed keeps its final values, a deadlocked one examines the Level1 jobs it has
 * left every second, so their share keeps growing.  A cluster's sample at its own t_end
 * (mcs_cluster_stats) equals mcs_read_delay_stats in total_wait_ms and jobs_count.
 * MCS_E_STATE: before a run, after a FIFO run, after a trading run, after mcs_append_jobs.
 * MCS_E_INVALID: period_s == 0, n_samples == 0, out == NULL, n_clusters above the engine's count, or
 * a last sample past 0xFFFFFFFE.  kernel_ms (may be NULL) receives the summed device time. */
int mcs_wait_time_series(mcs_engine* eng, uint32_t t0_s, uint32_t period_s, uint32_t n_samples,
                         mcs_wait_sample* out, uint32_t n_clusters, double* kernel_ms);

/* ---- the Start stream of an online session ---------------------------------------------------- */
/* The two series above and the record at t0_s, read from the current online session (mcs_run with a
 * horizon, mcs_append_jobs; FIFO or DELAY without trading) as its last mcs_run left it:
 * after a finite horizon, after a run that followed mcs_append_jobs, on a stream mcs_generate_jobs
 * fused (its records are materialised, as the batch calls do).  The four batch calls
 * (mcs_cluster_states, mcs_cluster_state_series, mcs_wait_time_series, mcs_dtrade_state_series) keep
 * returning MCS_E_STATE after mcs_append_jobs and name this call.
 *   out[c * n_samples + k]   cluster c at t_k = t0_s + k * period_s, as mcs_cluster_state_series
 *   wait (may be NULL)       the same shape, as mcs_wait_time_series; a DELAY session only
 *                            (MCS_E_INVALID under FIFO: only "/delay" feeds WaitTime)
 *   first (may be NULL)      the full record at t0_s, as mcs_cluster_states
 * The decided frontier.  Let h be the horizon of the last mcs_run.  After a finite horizon every t_k
 * must lie below h (MCS_E_INVALID otherwise; mcs_last_error names h).  After a drain
 * (MCS_TIME_NONE) every t_k up to 0xFFFFFFFE is accepted, and the samples describe the streams so
 * far as a batch run over them would, the continued Go loop of the wait statistics included.
 * The guarantee.  A sample below a finite horizon is final: no later append or horizon changes a bit
 * of it, and it equals, bit for bit, the sample the batch calls return after a batch run over all the
 * jobs the session ever receives.  Every start below h is decided by mcs_run(h), and appended jobs
 * arrive at or after h, so an undecided job is exactly one with start >= h > t_k: queued if its
 * arrival <= t_k, never running.  The wait statistics at t_k < h depend on the arrivals and the
 * starts below h alone (DESIGN.md §14 has the derivation).  A session that starts over (mcs_rewind,
 * or a horizon or an append after a batch run) first marks every row undecided, so no result of the
 * earlier pass is read, whatever jobs the restarted session then receives.
 * MCS_E_STATE: without an online session (before any run, after a batch or a trading run); after
 * mcs_rewind until the next run; after a run that failed (MCS_E_RANGE, MCS_E_CAPACITY); after jobs
 * were appended behind a drain, until the next run.  MCS_E_INVALID: as mcs_cluster_state_series, a
 * non-NULL wait under FIFO, a sample at or past a finite horizon.  Each call rebuilds its scratch
 * (batch summaries, wait records) from the session: its cost grows with the history, and nothing is
 * kept that a later run, append, rewind or segment relayout could leave stale (a caller that follows
 * a long session subscribes instead: mcs_stream_open, below).  kernel_ms (may be NULL) receives the
 * summed device time of the launches. */
int mcs_online_state_series(mcs_engine* eng, uint32_t t0_s, uint32_t period_s, uint32_t n_samples,
                            mcs_cluster_sample* out, mcs_wait_sample* wait /* may be NULL */,
                            mcs_cluster_state* first /* may be NULL */, uint32_t n_clusters,
                            double* kernel_ms);

/* ---- a cursor on the Start stream of an online session ---------------------------------------- */
/* mcs_online_state_series keeps nothing between calls, so a live slice's telemetry costs what the
 * session's whole history costs.  A stream is a subscription: it remembers where it is, hands out each
 * decided sample once, and keeps on the device what no later horizon or append can change (DESIGN.md
 * §14), so that a call's cost follows the slice and the jobs still alive.  One stream per engine. */
typedef struct mcs_stream_stats {
    uint32_t n_written;    /* samples per cluster this call wrote                                   */
    uint32_t t_first;      /* second of sample 0 of this call (undefined when n_written == 0)       */
    uint32_t t_next;       /* the stream's next sample second after this call                       */
    uint32_t pending;      /* decided samples not yet taken after this call                         */
    uint64_t rows_scanned; /* distinct rows whose results (node/start/finish) or wait record this
                              call's per-job loops loaded: whole batches of 256, counted on the device
                              from the batch flags and summaries, never estimated                    */
    uint64_t rows_retired; /* rows lying in retired batches after this call                         */
    double kernel_ms;      /* HIP events on the engine stream, summed over the launches             */
} mcs_stream_stats;

/* Subscribes to the current online session (FIFO or DELAY without trading) at the cadence
 * t0_s + k * period_s; with_wait != 0 adds the wait statistics (a DELAY session).  The stream may be
 * opened mid-session with t0_s far below the horizon: the first mcs_stream_next then catches up over
 * the history once.  MCS_E_STATE without an online session, after a run that failed, or when a stream
 * is open; MCS_E_INVALID for period_s == 0 and for with_wait under FIFO. */
int mcs_stream_open(mcs_engine* eng, uint32_t t0_s, uint32_t period_s, uint32_t with_wait);

/* Let h be the horizon of the last successful finite mcs_run.  Writes the samples
 * t_next + k * period_s < h, k < max_samples, to out[c * max_samples + k] (and to wait in the same
 * shape: non-NULL exactly when the stream was opened with_wait) and advances t_next past them.  No
 * sample to write is MCS_OK with n_written == 0.  n_clusters must equal mcs_num_clusters: the frontier
 * is common to all clusters.  Every sample is, bit for bit, what mcs_online_state_series returns for
 * that second on the same session at that moment, hence final (see there).
 * mcs_run(MCS_TIME_NONE) does not move the frontier: after a drain the call still serves what is
 * pending below the last finite horizon, then nothing (the tail of a finished session is
 * mcs_online_state_series's).  The stream is closed by the first mcs_run after a drain, by mcs_rewind
 * and any other restart of the session, by mcs_submit_jobs, mcs_generate_jobs and mcs_load_clusters, and
 * by a run that failed; the call then returns MCS_E_STATE, mcs_last_error names the cause, and the
 * caller reopens.  A segment relayout by mcs_append_jobs does not close it.  MCS_E_INVALID: out == NULL,
 * max_samples == 0, n_clusters != mcs_num_clusters, wait not as the stream was opened.
 * stats may be NULL. */
int mcs_stream_next(mcs_engine* eng, uint32_t max_samples, mcs_cluster_sample* out,
                    mcs_wait_sample* wait /* NULL unless with_wait */, uint32_t n_clusters,
                    mcs_stream_stats* stats /* may be NULL */);

/* Ends the subscription and frees what it kept.  MCS_E_STATE when no stream was opened or the stream
 * was closed already by this call.  Closes a stream of either kind (mcs_stream_open,
 * mcs_stream_open_level1). */
int mcs_stream_close(mcs_engine* eng);

/* ---- the Level1 list over time: what ProvideJobs hands the trader ---------------------------- */
/* The other half of the ResourceChannel service (pkg/scheduler/trader_server.go): ProvideJobs (:69-94,
 * over GetLevel1, scheduler.go:204-214) sends sched.Level1 in batches of 20, the last one padded with
 * zero jobs (D9), and the trader sizes every contract from that list: calculateFastNodeSize and
 * calculateSmallNodeSize (pkg/trader/scheduler_client.go:126-289).  One sample holds the list's length,
 * its first row and the finished ContractRequest of both sizings after the Delay iteration at t_k
 * (SDELAY) — the convention of mcs_wait_time_series, and the point at which a trader
 * round of tick t_k reads Level1 in the lock-step order (scheduler steps, state samples, trader
 * rounds; mcs_trade.h).
 * ContractRequest.Price is not returned: it is always 0.  Both sizings multiply by
 * Trader.MaximimumCoreCost and Trader.MemoryCost, which nothing ever sets (trader.go:34-35), and
 * Budget is -1 (trader.go:53), so no price is positive and the budget never ends a sizing loop. */
typedef struct mcs_level1_sample {   /* 24 B */
    uint32_t len;          /* len(sched.Level1) after the Delay iteration at t_k                     */
    uint32_t cores;        /* ContractRequest.Cores of both sizings: sum of CoresNeeded mod 2^32     */
    uint32_t mem;          /* ... Memory, likewise (both sizings add in uint32 / int32 and wrap; they
                              agree while every single request is at most 2^31: the small-node sizing
                              drops a larger one, :238-250, and this field then is the fast one)     */
    uint32_t fast_time_s;  /* calculateFastNodeSize: max Duration over the list, seconds; 0 if empty */
    uint32_t small_time_s; /* calculateSmallNodeSize over the list padded to a multiple of 20 (D9):
                              each job sets the time to its Duration if the time so far is below it,
                              else to 0 (:263-265), so a padded last batch leaves 0                  */
    uint32_t head;         /* row of Level1[0] in the cluster's stream; MCS_TIME_NONE when empty     */
} mcs_level1_sample;

/* Every sample t_k = t0_s + k * period_s, k < n_samples, of every cluster, rebuilt on the GPU from the
 * last DELAY run's arrivals and starts and the engine's max_wait_s:
 * Level1(t) = { j : m_j <= t < s_j } in stream order, m_j the iteration at which job j, still failing
 * as the Level0 head, moves to Level1 and s_j its start.  out[c * n_samples + k] is cluster c at t_k.
 * The Go loop is continued past the run's end, as mcs_wait_time_series does: a drained cluster reads
 * as empty, a deadlocked one keeps the jobs it has left up to second 0xFFFFFFFE, and a job undecided
 * when a trading run stopped at t_max_s counts as never placed.
 * Accepted after a DELAY run without trading and after a DELAY trading run on one engine (every logged
 * contract of mcs_read_contracts then equals the sample at its (t_s, requester): cores, mem and
 * fast_time_s under policy 0, small_time_s under policy 1).  MCS_E_STATE, with the cause in
 * mcs_last_error: before a run, after a FIFO or FIFO trading run, on a sharded engine
 * (mcs_set_shard with world > 1), after mcs_append_jobs (an online session is served by
 * mcs_online_level1_series).  MCS_E_INVALID as mcs_cluster_state_series: period_s == 0,
 * n_samples == 0, out == NULL, n_clusters above the engine's count, or a last sample past 0xFFFFFFFE.
 * kernel_ms (may be NULL) receives the summed device time of the launches. */
int mcs_level1_series(mcs_engine* eng, uint32_t t0_s, uint32_t period_s, uint32_t n_samples,
                      mcs_level1_sample* out, uint32_t n_clusters, double* kernel_ms);

/* The same samples of the current online session (a DELAY session; MCS_E_INVALID under FIFO, which has
 * no Level1), under the rules of mcs_online_state_series: read as the last mcs_run left the session;
 * after a finite horizon h every t_k must lie below h (MCS_E_INVALID otherwise) and a sample below it
 * is final, equal bit for bit to mcs_level1_series after a batch run over all the jobs the session
 * ever receives (a job undecided at h has m_j exact wherever it lies below h and s_j >= h > t_k);
 * after a drain every t_k up to 0xFFFFFFFE is accepted.  MCS_E_STATE as mcs_online_state_series:
 * without an online session, after mcs_rewind until the next run, after a run that failed, after jobs
 * appended behind a drain.  Nothing is kept between calls. */
int mcs_online_level1_series(mcs_engine* eng, uint32_t t0_s, uint32_t period_s, uint32_t n_samples,
                             mcs_level1_sample* out, uint32_t n_clusters, double* kernel_ms);

/* Level1 samples on the cursor: both halves of ResourceChannel at a slice's cost.  A stream opened with
 * mcs_stream_open_level1 (a DELAY session; MCS_E_INVALID under FIFO, which has no Level1; everything else
 * as mcs_stream_open, with_wait included) also hands out, at its own cadence, the mcs_level1_sample
 * (above) of every second it hands out: mcs_stream_next_level1 fills level1[c * max_samples + k], k <
 * n_written, for the same seconds as out, each bit for bit what mcs_online_level1_series returns for
 * that second on the same session at that moment; out and wait are exactly mcs_stream_next's.  There is
 * still one stream per engine and one cadence: a trader that reads ProvideJobs every 10 s and Start
 * every 5 s subscribes at 5 and ignores every other list.  Between calls the engine then also keeps
 * the per-row records whether or not with_wait is set (16 B per row), one uint32 per batch of 256 rows
 * (the batch's Level1 summary, final once the batch is) and 8 B per cluster (the two scan bounds, which
 * only move up: DESIGN.md §14); a call scans the batches between the bounds that still hold a member.
 * level1 must be non-NULL exactly when the stream was opened with Level1, in either next call
 * (MCS_E_INVALID otherwise: mcs_stream_next on a Level1 stream is refused).  stats and l1stats may be
 * NULL.  Frontier, closing causes and relayouts are the cursor's own. */
typedef struct mcs_level1_stream_stats {
    uint64_t rows_scanned;  /* rows whose record this call's Level1 scans loaded, counted on the device */
    double kernel_ms;       /* device time of the Level1 launches of this call (also inside stats->kernel_ms) */
} mcs_level1_stream_stats;
int mcs_stream_open_level1(mcs_engine* eng, uint32_t t0_s, uint32_t period_s, uint32_t with_wait);
int mcs_stream_next_level1(mcs_engine* eng, uint32_t max_samples, mcs_cluster_sample* out,
                           mcs_wait_sample* wait /* NULL unless with_wait */, mcs_level1_sample* level1,
                           uint32_t n_clusters, mcs_stream_stats* stats, mcs_level1_stream_stats* l1stats);

/* ProvideJobs at one second: the rows of Level1(t_s) of one cluster in list order, as indices into
 * the cluster's stream (row r is job job_offsets[cluster] + r of mcs_read_jobs, which has its
 * CoresNeeded, MemoryNeeded and Duration).  *n receives len(Level1); it may exceed cap, and then the
 * first cap rows are written (rows may be NULL when cap is 0).  The preconditions of
 * mcs_level1_series; MCS_E_INVALID also for a cluster out of range, t_s past 0xFFFFFFFE and n == NULL. */
int mcs_read_level1(mcs_engine* eng, uint32_t cluster, uint32_t t_s, uint32_t* rows, uint32_t cap,
                    uint32_t* n);

#ifdef __cplusplus
}
#endif
#endif /* MCS_H */
