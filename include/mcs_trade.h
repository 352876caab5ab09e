/*
 * mcs_trade.h — lock-step trading extension of the MI355X engine (libmcs.so): the FIFO borrow
 * protocol and the per-cluster trader, batched over many clusters and sharded over GPUs.
 *
 * Replaces (reference snapshot 2024-10-16):
 *   Scheduler.BorrowResources        pkg/scheduler/server.go:160-248  (borrow broadcast)
 *   "/borrow" handler + Lend         pkg/scheduler/server.go:80-113, scheduler.go:194-202
 *   LentQueue service in Fifo        pkg/scheduler/scheduler.go:277-290
 *   Trader.RequestPolicyMonitor      pkg/trader/trader.go:280-325
 *   Trader.Trade + contractResHeap   pkg/trader/trader.go:169-278
 *   traderServer.RequestResource /
 *   ApproveContract                  pkg/trader/server.go:31-85
 *   ApproveTrade                     pkg/trader/trader.go:141-167
 *   Start (state stream)             pkg/scheduler/trader_server.go:24-47
 *   AddVirtualNode /
 *   AllocateVirtualNodeResources     pkg/scheduler/cluster.go:65-125
 * Semantics: the lock-step serialization of DESIGN.md §9 (tick T: scheduler steps, borrow
 * exchange, state samples, trader rounds), bit-identical to oracle/mcs_oracle_trade.c.  With
 * MCS_POLICY_DELAY the schedulers run Scheduler.Delay and the traders size real contracts from
 * Level1 (oracle/mcs_oracle_dtrade.c): Foreign jobs on responders, virtual nodes
 * with capacity on requesters.  DELAY trading shards too: its tick exchanges one block per rank
 * (per-cluster records + node snapshots) and runs the trader rounds replicated on every rank.
 *
 * Sharding: the clusters are split in equal contiguous blocks over `world` engines (one per GPU,
 * usually one process each).  A tick of either policy needs one all-gather of one block per rank
 * (per-cluster records + node snapshots; phase 0 -> 1; phases 2 and 3 move no bytes): the
 * remaining phases run replicated over the whole system on every rank.  Every rank must hold the
 * same number of clusters and the same largest cluster (the block layout).
 * Two transports:
 *   - RCCL (mcs_comm_unique_id on rank 0, shared out of band, then mcs_comm_init on every rank):
 *     mcs_run drives the whole lock-step loop with ncclAllGather over xGMI;
 *   - caller-driven (no communicator): the caller runs the ticks with mcs_trade_phase and moves
 *     the bytes between ranks itself (any transport; tests use torch.distributed gloo).
 * With world == 1 neither is needed: mcs_run keeps the exchange in HBM.
 */
#ifndef MCS_TRADE_H
#define MCS_TRADE_H

#include "mcs.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One lent-job execution: the lender ran the borrower's job (index within the BORROWER's stream)
 * after accepting it on a /borrow request.  Every acceptor runs its own copy (server.go:232-237). */
typedef struct mcs_lent_rec {
    uint32_t lender, borrower; /* global cluster indices */
    uint64_t job;              /* job index in the borrower's stream */
    uint32_t node, start_s, finish_s, pad;
} mcs_lent_rec;

/* One trader round whose request policy broke (trader.go:288-303). */
typedef struct mcs_trade_rec {
    uint32_t t_s;       /* tick of the round */
    uint32_t requester; /* global cluster index */
    int32_t winner;     /* responder whose virtual node was received, -1 = "couldn't acquire resources" */
    uint32_t approvals; /* approving responses pushed on the heap */
} mcs_trade_rec;

/* One trader round of a DELAY system (MCS_POLICY_DELAY + trader), with its contract
 * (calculateFastNodeSize / calculateSmallNodeSize, pkg/trader/scheduler_client.go:126-289). */
typedef struct mcs_contract_rec {
    uint32_t t_s, requester;
    int32_t winner;     /* responder whose AllocateVirtualNodeResources succeeded, -1 = none    */
    uint32_t approvals;
    uint32_t policy;    /* 0 = WaitTime (fast node, trader.go:304-320), 1 = Utilization (small) */
    uint32_t cores, mem, time_s; /* the ContractRequest (trader.proto:20-27); price is 0        */
    uint32_t failed;    /* popped approvals whose ApproveContract failed before the winner       */
    uint32_t pad;
} mcs_contract_rec;

/* One Foreign job launched on a responder by AllocateVirtualNodeResources (cluster.go:87-125):
 * it holds {c, m} of node `node` of cluster `responder` from start_s to finish_s.  c and m are
 * Go uint values (cluster.go:116): they may exceed what the node had (the counter wraps). */
typedef struct mcs_foreign_rec {
    uint32_t requester, responder, node, start_s, finish_s, pad;
    uint64_t c, m;
} mcs_foreign_rec;

typedef struct mcs_trade_stats {
    uint64_t placed;       /* own jobs placed locally */
    uint64_t borrowed;     /* own jobs moved to the BorrowedQueue */
    uint64_t waited;       /* own jobs that entered the WaitQueue */
    uint64_t undecided;    /* own jobs neither placed nor borrowed (t_max reached) */
    uint64_t lent_runs;    /* lent-job executions on this engine's clusters */
    uint64_t lent_pending; /* LentQueue entries never run */
    uint64_t trades;       /* trader rounds with a broken policy (all clusters, replicated) */
    uint64_t trades_won;   /* ... that received a virtual node */
    uint32_t ticks;        /* lock-step ticks executed (fast-forward skips idle seconds) */
    uint32_t t_final;      /* last tick */
    uint32_t flags;        /* OR of MCS_FLAG_* over clusters and logs */
    uint32_t loop_form;    /* tick loop that ran: 0 = one engine, hipGraph-replayed ticks; 1 = RCCL
                              all-gather per tick, eager launches; 2 = RCCL, kernels and all-gathers
                              captured in a hipGraph (MCS_RCCL_GRAPH=0 forces 1); 3 = one
                              engine, the whole system resident in one workgroup; 4 = resident,
                              one workgroup per 4 clusters, exchange written through to memory;
                              5 = the same with every workgroup on one XCD, exchange in its L2;
                              6 = form 0 after a resident exchange timed out (workers not all
                              resident at once: the run was redone on the replayed kernels);
                              7 = RCCL, ONE launch per tick (phases B-D of tick n + A of tick
                              n + 1, mcs_trade_rk.hip) and one all-gather, captured in a hipGraph;
                              8 = the same, eager; 9 = the one-launch tick on the caller-driven
                              phase API (MCS_TRADE_RK=0: the three-kernel forms 0-2) */
    double kernel_ms;      /* device time of the lock-step loop (HIP events) */
    double wall_ms;
    /* ABI v7: the exchange-block layout the run used (equal on every rank) */
    uint64_t block_bytes;  /* bytes of one rank's exchange block (the all-gather's per-rank slice) */
    uint32_t snaps;        /* 1 = the blocks carry node snapshots; 0 = records + G tables only
                              (the one-launch tick when no rank has a node above 64 cores) */
    uint32_t agreed;       /* 1 = the layout was agreed over all ranks (the RCCL loop's shape
                              all-reduce, or mcs_trade_set_shape on the caller-driven path) */
} mcs_trade_stats;

/* ---- sharding and transport ------------------------------------------------------------------- */
typedef struct mcs_comm_id {
    char bytes[128]; /* ncclUniqueId */
} mcs_comm_id;

/* This engine holds clusters [rank*C, rank*C + C) of world*C (C = mcs_num_clusters).  Call after
 * mcs_load_clusters; default is rank 0 of 1. */
int mcs_set_shard(mcs_engine* eng, uint32_t rank, uint32_t world);
/* RCCL transport: ncclGetUniqueId (rank 0) and ncclCommInitRank on this engine's device. */
int mcs_comm_unique_id(mcs_comm_id* out);
int mcs_comm_init(mcs_engine* eng, const mcs_comm_id* id);

/* ---- caller-driven lock-step ---------------------------------------------------------------- */
/* One tick is phases 0..3.  Phase p reads `in` (the all-gather, in rank order, of every rank's
 * `out` of phase p-1; phase 0 takes no input) and writes this rank's slice for the next
 * exchange.  Sizes per phase from mcs_trade_xfer_bytes: today only phase 0 writes (this rank's
 * block) and only phase 1 reads (every rank's blocks); the other sizes are 0 and an empty output
 * need not be gathered.  *done becomes 1 (identically on every rank) after the phase 3
 * that ends the run; keep calling phase 0..3 until then.  mcs_trade_begin resets the lock-step
 * state; mcs_trade_end fills the stats and makes the results readable. */
int mcs_trade_begin(mcs_engine* eng);
/* Agreed block layout (ABI v7).  The RCCL loop agrees on the exchange-block layout with one
 * all-reduce (MAX) before the run.  The caller-driven transport does the same through these two
 * calls, made after mcs_set_shard / mcs_submit_jobs and before mcs_trade_begin:
 * mcs_trade_shape_words writes this rank's MCS_TRADE_SHAPE_WORDS words; the caller takes their
 * element-wise MAX over all ranks and passes the result to mcs_trade_set_shape on every rank.  The
 * agreed shape fixes the snapshot stride (the largest cluster of the system), whether every rank
 * runs the one-launch tick (one rank that cannot, or has MCS_TRADE_RK=0, turns it off for all) and
 * whether the blocks drop the node snapshots (no node above 64 cores on any rank: 320 B per
 * cluster, the layout an 8-GPU RCCL run uses).  A cluster-count mismatch fails (MCS_E_INVALID) on
 * every rank.  Without an agreed shape each rank decides from its own shard and the blocks keep
 * the snapshots.  Every caller-driven phase-0 block ends in a 16-byte layout tag (tick form,
 * snapshots, stride, clusters, policy); phase 1 fails with MCS_E_INVALID when the gathered blocks'
 * tags differ, so ranks that chose different layouts never exchange silently. */
#define MCS_TRADE_SHAPE_WORDS 8
int mcs_trade_shape_words(mcs_engine* eng, uint32_t* out);
int mcs_trade_set_shape(mcs_engine* eng, const uint32_t* agreed);
int mcs_trade_xfer_bytes(mcs_engine* eng, uint32_t phase, uint64_t* in_bytes, uint64_t* out_bytes);
int mcs_trade_phase(mcs_engine* eng, uint32_t phase, const void* in, uint64_t in_bytes, void* out,
                    uint64_t out_bytes, uint32_t* done);
int mcs_trade_end(mcs_engine* eng, mcs_stats* stats);

/* ---- results (after mcs_run or mcs_trade_end) ---------------------------------------------- */
/* Besides the readers below, a FIFO trading run on one engine (rank 0 of world 1) leaves the
 * ClusterState telemetry readable: mcs_cluster_states and mcs_cluster_state_series (mcs.h) rebuild
 * the record from the own placements plus the lent runs, as the Start stream would sample it after
 * the tick's scheduler steps and borrow exchange and before its trader rounds.  They return
 * MCS_E_STATE on a sharded engine, after a lent-log overflow (MCS_FLAG_LOG_OVERFLOW) and after a
 * DELAY trading run. */
int mcs_read_trade_stats(mcs_engine* eng, mcs_trade_stats* out);
/* Lent runs executed by this engine's clusters, sorted by (start_s, lender, borrower, job).
 * *n = total count (may exceed cap: then only cap records are written). */
int mcs_read_lent(mcs_engine* eng, mcs_lent_rec* out, uint64_t cap, uint64_t* n);
/* Trader rounds of ALL clusters in (t_s, requester) order (identical on every rank). */
int mcs_read_trades(mcs_engine* eng, mcs_trade_rec* out, uint64_t cap, uint64_t* n);
/* Virtual nodes received by each of the world*C clusters (AddVirtualNode, cluster.go:65-85):
 * zero-capacity under FIFO, the contract's capacity under DELAY. */
int mcs_read_virtual_nodes(mcs_engine* eng, uint32_t* out, uint32_t n_total);

/* ---- DELAY trading (MCS_POLICY_DELAY with cfg.trader) ----------------------------------------- */
/* Trader rounds of ALL clusters with their contracts, in (t_s, requester) order, identical on
 * every rank; *n = total count. */
int mcs_read_contracts(mcs_engine* eng, mcs_contract_rec* out, uint64_t cap, uint64_t* n);
/* Foreign jobs of ALL clusters in launch order (global indices, identical on every rank). */
int mcs_read_foreign(mcs_engine* eng, mcs_foreign_rec* out, uint64_t cap, uint64_t* n);
/* Capacities {cores, memory} of the virtual nodes local cluster `cluster` received, in order (node
 * index n_physical + i); *n = their count. */
int mcs_read_virtual_node_caps(mcs_engine* eng, uint32_t cluster, uint32_t* cores, uint32_t* mem,
                               uint32_t cap, uint32_t* n);

/* The ClusterState telemetry of a DELAY trading run on one engine (rank 0 of world 1), after
 * mcs_run or mcs_trade_end: what the Start stream (trader_server.go:24-47) would have sent at the
 * seconds t0_s + k * period_s, k < n_samples, sampled after the tick's Delay iteration and before its
 * trader rounds.  out[c * n_samples + k] is cluster c's sample (mcs_cluster_sample, mcs.h), wait (may
 * be NULL) the WaitTime statistics in the same shape (mcs_wait_sample), first (may be NULL) the full
 * record at t0_s from a plain scan, n_clusters of them.  The three calls of mcs.h keep refusing such
 * a run; this call refuses every other run.
 *   - Rows: the cluster's physical nodes, then the virtual nodes it received, in order
 *     (mcs_read_virtual_node_caps), each with capacity = initial free = its contract's {cores, mem}.
 *     A virtual row is present from second 0: it holds nothing before its trade and its term is +0.
 *   - An own job with node >= 0 holds its row (physical or virtual) on start <= t < finish; node -1
 *     (undecided at t_max_s) is never running and stays queued.
 *   - A Foreign job (mcs_foreign_rec, responder == c) holds {c, m} of row `node` on
 *     start_s < t < finish_s: AllocateVirtualNodeResources runs after the sample of tick start_s.
 *   - Counters are Go uint (uint64) and wrap: free = free0 - held (mod 2^64); a row's term is
 *     float32(cap) - float32(free), summed in float32 in row order, divided by float32 of the totals
 *     of the physical nodes (cluster.go:79: never recomputed).  Negative utilization is routine.
 *   - running = own jobs plus Foreign jobs holding at t; queued = own jobs with arrival <= t that have
 *     not started by t.  The wait statistics are those of mcs_wait_time_series over the run's
 *     placements (they depend on no node); past the run's end the Go loop is continued.
 * MCS_E_INVALID as mcs_cluster_state_series.  MCS_E_STATE, with the cause in mcs_last_error: before a
 * run, after anything but a DELAY trading run, on a sharded engine, after a Foreign-log or
 * contract-log overflow (MCS_FLAG_LOG_OVERFLOW), a virtual-node overflow (MCS_FLAG_VNODE_OVERFLOW) or
 * a run cut short by a capacity overflow, and after mcs_append_jobs.  MCS_DTRADE_FOREIGN_LOG_CAP in
 * the environment lowers the Foreign log's capacity (tests).  *kernel_ms (may be NULL): device time. */
int mcs_dtrade_state_series(mcs_engine* eng, uint32_t t0_s, uint32_t period_s, uint32_t n_samples,
                            mcs_cluster_sample* out, mcs_wait_sample* wait, mcs_cluster_state* first,
                            uint32_t n_clusters, double* kernel_ms);

/* ---- trading sessions: online mode of a DELAY trading system ---------------------- */
/* With MCS_POLICY_DELAY, cfg.trader = 1 and cfg.borrow = 0 on one engine (rank 0 of world 1, no
 * communicator) the online calls of mcs.h drive the lock-step system live, as the reference deploys it
 * (scheduler.go:116, pkg/client/server.go:53): the lock-step state stays in HBM between calls.
 *   mcs_run(h), h finite    executes every lock-step tick T < h and stops.  "Every job so far decided"
 *                           does not stop it: the samples keep coming every sample_period_s and the
 *                           trader rounds keep falling due.  Horizons are non-decreasing and at most
 *                           t_max_s + 1 (MCS_E_INVALID otherwise, nothing runs).
 *   mcs_run(MCS_TIME_NONE)  a drain: until every job appended so far is decided; it stops after the tick
 *                           that decides the last one (its samples and rounds included), where the batch
 *                           run stops, or after tick t_max_s with MCS_FLAG_T_MAX; no tick when nothing is
 *                           undecided.
 *   mcs_append_jobs         per cluster, arrival-sorted: each arrival >= the cluster's last arrival, >=
 *                           the last finite horizon and > the last executed tick (the clock is common to
 *                           all clusters: after a drain that ended at tick T_d the floor is T_d + 1
 *                           everywhere).  Starts a session at t = 0 over the submitted jobs if none is
 *                           active.
 *   mcs_rewind              restarts at t = 0 with every job so far.
 * Between calls mcs_read_placements, mcs_read_cluster_stats, mcs_read_delay_stats and every reader of
 * this header work on the session as its last mcs_run left it (undecided rows: MCS_NODE_UNPLACED /
 * MCS_TIME_NONE); mcs_stats reports online = 1, t_horizon, placed = decided so far, pending = jobs -
 * decided and the kernel_ms of the call.
 * The guarantee: slicing never changes a decision.  After mcs_run(h) the readers return, bit for bit,
 * the state of a batch run over all the jobs the session ever receives taken after that run's last tick
 * below h (for as long as the batch run reaches that far); after the final drain they return the whole
 * batch run, ticks and t_final included.  A horizon past the tick that decided the last job executes
 * sample ticks and trader rounds the batch run never reaches: placements cannot change there, the logs
 * and the trader state may grow with records whose t_s exceeds the batch run's t_final.
 * A slot-pool or virtual-node overflow inside a slice escalates as the batch run does and replays the
 * session from t = 0 up to the horizon (restarts counts it); when the capacity is exhausted the call
 * returns MCS_E_CAPACITY and mcs_run returns MCS_E_STATE until mcs_rewind or a new submit.
 * MCS_E_STATE: FIFO trading (borrow, or trader under FIFO), a sharded engine or one with a
 * communicator, mcs_trade_begin during a session, and during a session every telemetry call of
 * batch runs and plain sessions (mcs_dtrade_state_series, mcs_level1_series, mcs_read_level1,
 * mcs_online_state_series, mcs_online_level1_series, mcs_stream_open, mcs_cluster_states,
 * mcs_cluster_state_series, mcs_wait_time_series): a trading session's Start stream is read with
 * mcs_trade_session_state_series and mcs_trade_session_level1_series below, and subscribed to with
 * mcs_trade_stream_open / next / close.
 * External traders (further below): mcs_trade_external switches the built-in trader rounds off, and the
 * caller issues ProvideVirtualNode and ReceiveVirtualNode itself between two slices
 * (mcs_trade_session_provide_vnodes, mcs_trade_session_receive_vnodes).  mcs_run(h), h finite, then always
 * ends with a tick at h - 1, so the guarantee reads: slicing changes no decision and no grant outcome, but
 * it may change ticks_total; and a replay for a capacity escalation re-applies the grants. */
typedef struct mcs_trade_session {
    uint32_t t_horizon;      /* last finite horizon (0: none yet)                                      */
    uint32_t t_last;         /* last executed tick                                                     */
    uint32_t t_next;         /* the tick the session would execute next: the smaller of the tick the
                                next-tick rule chose and the earliest arrival appended since            */
    uint32_t ticks_last_run; /* ticks the last mcs_run executed (after a restart: those of the replay)  */
    uint32_t ticks_total;    /* ticks since t = 0, the batch run's mcs_trade_stats.ticks                */
    uint32_t restarts;       /* replays from t = 0 for a capacity escalation                            */
    uint32_t drained;        /* 1: the last mcs_run was a drain                                         */
    uint32_t failed;         /* 1: capacity exhausted (MCS_E_CAPACITY)                                  */
} mcs_trade_session;
/* MCS_E_STATE without a trading session. */
int mcs_trade_session_info(mcs_engine* eng, mcs_trade_session* out);

/* The Start stream of a trading session (DESIGN.md §14 "The Start stream of a trading session"): the
 * record of mcs_dtrade_state_series, argument for argument, read from the session as its last mcs_run
 * left it.  Rows: the physical nodes, then the virtual nodes the cluster has received so far; own jobs
 * hold on start <= t < finish, Foreign jobs on start_s < t < finish_s; uint64 counters that wrap; float32
 * terms in row order over the physical totals; running, queued and the wait statistics as there.  wait
 * and first may be NULL.
 *   - After mcs_run(h), h finite, every sample second must lie below h (MCS_E_INVALID otherwise; the
 *     message names h).  Such a sample is final: it equals, bit for bit, what mcs_dtrade_state_series
 *     returns for that second after a batch run over all the jobs the session ever receives, as long as
 *     that run reaches the second.
 *   - After a drain any second up to 0xFFFFFFFE is accepted; the samples are those of the batch run over
 *     the jobs held, the Go loop of the wait statistics continued past its end.
 * MCS_E_INVALID otherwise as mcs_cluster_state_series.  MCS_E_STATE, with the cause in mcs_last_error:
 * without a trading session; after mcs_rewind (or the session's begin) until the next mcs_run; after the
 * session failed (MCS_E_CAPACITY); after jobs appended behind a drain until the next mcs_run; and when
 * the run's flags carry a Foreign-log or contract-log overflow (MCS_FLAG_LOG_OVERFLOW) or a virtual-node
 * overflow, as mcs_dtrade_state_series refuses.  Nothing is kept between calls.  The Foreign log, which
 * grows with the session's age, is compacted per call to the records that can hold at one of the call's
 * samples once the log and the call are long enough for that to pay; MCS_DT_FOREIGN_FILTER in the
 * environment at mcs_create forces the choice (0: the log is scanned as it is; any other value: always
 * compacted; A/B runs and tests; the bytes are equal).  A subscriber that wants each decided sample
 * once, at a cost that does not grow with the session's age, uses the cursor below
 * (mcs_trade_stream_open / next / close).  Not available: mcs_read_level1, sharded engines. */
int mcs_trade_session_state_series(mcs_engine* eng, uint32_t t0_s, uint32_t period_s, uint32_t n_samples,
                                   mcs_cluster_sample* out, mcs_wait_sample* wait, mcs_cluster_state* first,
                                   uint32_t n_clusters, double* kernel_ms);
/* What ProvideJobs hands the trader in a trading session: mcs_online_level1_series (mcs.h) over the
 * trading session's rows, under the frontier and the refusals of mcs_trade_session_state_series. */
int mcs_trade_session_level1_series(mcs_engine* eng, uint32_t t0_s, uint32_t period_s, uint32_t n_samples,
                                    mcs_level1_sample* out, uint32_t n_clusters, double* kernel_ms);

/* A cursor on the Start stream of a trading session (DESIGN.md §14 "A cursor on a trading session's Start
 * stream"): mcs_stream_open / next / close (mcs.h) for a trading session.  mcs_trade_stream_next writes
 * the samples t_next + k * period_s below the frontier F* that it has not handed out yet, at most
 * max_samples of them, each bit for bit what mcs_trade_session_state_series returns for that second on the
 * same session at that moment (and therefore final).  Layout, argument checks and `pending` are
 * mcs_stream_next's: out (and wait, given exactly when the stream was opened with_wait) hold n_clusters
 * rows of max_samples columns, of which the first n_written are filled; n_clusters must equal
 * mcs_num_clusters.  Between calls the engine keeps, per batch of 256 rows, a flag word, the summary pair
 * and the sum of start - arrival, per row the wait record (with_wait), per cluster the carries, and the
 * list of the Foreign records that can still hold: the cost of a call follows the slice, the jobs still
 * alive and the Foreign jobs still holding, not the session's age.
 *   The frontier.  The lock-step clock is common to all clusters and appended arrivals must lie above the
 * last executed tick, so a drain that ends at tick T_d decides exactly as mcs_run(T_d + 1) would.
 * F* = max over the session's runs of (a finite horizon h; after a drain, t_last + 1); it never decreases.
 * A drain does not close the stream, nor does the first mcs_run after it, and samples below F* stay
 * servable after jobs were appended behind a drain and before the next run (where
 * mcs_trade_session_state_series refuses).
 *   Restarts.  A capacity escalation that replays the session from t = 0 inside mcs_run
 * (mcs_trade_session.restarts) does not close the stream: it keeps t_next, drops everything it kept, and
 * the next call that writes samples rebuilds once (rebuilt = 1; rows_retired starts again from 0).
 *   Closing.  mcs_rewind and any other restart of the session by the caller, mcs_submit_jobs,
 * mcs_generate_jobs, mcs_load_clusters, a run that failed (MCS_E_CAPACITY), a run whose flags carry a
 * Foreign-log, contract-log or virtual-node overflow, and a device error close the stream:
 * mcs_trade_stream_next then returns MCS_E_STATE, mcs_last_error names the cause, and the caller reopens.
 * A segment relayout by mcs_append_jobs does not close it.  One stream per engine; t0_s may lie far below
 * the frontier, and the first call then catches up once.  MCS_E_STATE without a trading session (a session
 * without trading subscribes with mcs_stream_open, which keeps refusing a trading session).  Level1
 * samples come with a cursor opened by mcs_trade_stream_open_level1 (below); the record at t0_s is not
 * part of a cursor. */
typedef struct mcs_trade_stream_stats {
    uint32_t n_written, t_first, t_next, pending; /* as mcs_stream_stats                                  */
    uint64_t rows_scanned, rows_retired;          /* as mcs_stream_stats, counted on the device           */
    uint32_t foreign_scanned; /* Foreign-log records this call read from the log (new since the last call
                                 that wrote samples)                                                      */
    uint32_t foreign_live;    /* records on the kept list that this call's tiles scanned                  */
    uint32_t rebuilt;         /* 1: this call rebuilt the kept state from the session (the first call that
                                 writes samples; after a replay)                                          */
    uint32_t frontier;        /* F*                                                                       */
    double kernel_ms;
} mcs_trade_stream_stats;
int mcs_trade_stream_open(mcs_engine* eng, uint32_t t0_s, uint32_t period_s, uint32_t with_wait);
int mcs_trade_stream_next(mcs_engine* eng, uint32_t max_samples, mcs_cluster_sample* out,
                          mcs_wait_sample* wait /* NULL unless with_wait */, uint32_t n_clusters,
                          mcs_trade_stream_stats* stats /* may be NULL */);
int mcs_trade_stream_close(mcs_engine* eng);
/* mcs_stream_open_level1 / mcs_stream_next_level1 (mcs.h) for a trading session: the cursor also hands
 * out, for the same seconds as out, the Level1 samples, each bit for bit what
 * mcs_trade_session_level1_series returns for that second on the same session at that moment (below F*
 * also where that call refuses: after jobs appended behind a drain).  level1 must be non-NULL exactly
 * when the stream was opened with Level1, in either next call.  A replay (rebuilt = 1) drops the
 * carried scan bounds with everything else kept; mcs_trade_stream_close closes either kind. */
int mcs_trade_stream_open_level1(mcs_engine* eng, uint32_t t0_s, uint32_t period_s, uint32_t with_wait);
int mcs_trade_stream_next_level1(mcs_engine* eng, uint32_t max_samples, mcs_cluster_sample* out,
                                 mcs_wait_sample* wait /* NULL unless with_wait */, mcs_level1_sample* level1,
                                 uint32_t n_clusters, mcs_trade_stream_stats* stats,
                                 mcs_level1_stream_stats* l1stats);

/* ---- external traders: ProvideVirtualNode and ReceiveVirtualNode in a trading session ------------- */
/* The scheduler's ResourceChannel service (pkg/scheduler/trader_server.go) has four RPCs.  Start and
 * ProvideJobs are the series and cursors above; the other two are how a trader acts on a scheduler:
 * ProvideVirtualNode (trader_server.go:57-67 -> AllocateVirtualNodeResources, cluster.go:87-125) and
 * ReceiveVirtualNode (trader_server.go:49-55 -> AddVirtualNode, cluster.go:65-85).  With the built-in
 * trader rounds switched off (external mode) the caller issues them itself between two slices, in
 * batches, on the GPU (DESIGN.md §14 "External traders").
 *
 * mcs_trade_external(eng, on): on != 0 switches the built-in trader rounds off (the lock-step system
 * without rounds, the oracle's dtrade_run(trader = 0)); 0 switches them back on.  It needs
 * MCS_POLICY_DELAY with cfg.trader = 1 and cfg.borrow = 0 on rank 0 of world 1 without a communicator,
 * after mcs_load_clusters, and is accepted while no lock-step tick of the current session has run
 * (before the first mcs_run, right after mcs_rewind, right after a new submit).  MCS_E_STATE, with the
 * cause in mcs_last_error: once a tick has run, under FIFO or cfg.trader = 0, on a sharded engine, and
 * during a caller-driven run (mcs_trade_begin).  The setting survives mcs_rewind and mcs_submit_jobs;
 * mcs_load_clusters resets it to 0.  With the switch on every run takes the replayed kernels, a batch
 * run included.
 *   The forced last tick.  The lock-step loop skips seconds in which nothing is queued, and a grant acts
 * on the node state the last executed tick left.  In external mode mcs_run(h), h finite, therefore always
 * ends with a tick at h - 1: it does the releases due and, on a multiple of sample_period_s, the sample,
 * and it decides nothing (ticks are consecutive while any job is queued).  Slicing then changes no
 * decision and no grant outcome, but it may change mcs_trade_session.ticks_total.  A drain forces
 * nothing. */
int mcs_trade_external(mcs_engine* eng, uint32_t on);

typedef struct mcs_vnode_request {
    uint32_t responder, requester; /* local cluster indices (world 1: global)                          */
    uint32_t cores, memory, time_s; /* the contract (trader.proto:20-27)                                */
    uint32_t pad;
} mcs_vnode_request;
typedef struct mcs_vnode_result {
    int32_t ok;          /* 1: both halves ended at 0; 0: "couldn't schedule enough resources" (the Foreign
                            jobs launched on the way stay, cluster.go:119-121)                          */
    uint32_t visited;    /* rows walked: a prefix of the responder's rows                               */
    uint32_t left_cores, left_memory; /* what remained of the request                                   */
} mcs_vnode_result;
typedef struct mcs_vnode_stats {
    uint32_t n, n_ok;       /* entries of the call; provide: those with ok = 1 (receive: n)            */
    uint32_t foreign_added; /* Foreign records the call appended                                        */
    uint32_t replayed;      /* 1: the call overflowed a pool and replayed the session from t = 0        */
    double kernel_ms;
} mcs_vnode_stats;
/* AllocateVirtualNodeResources for each request, in array order, as a trader round at the session's last
 * executed tick T = t_last would run it: the walk over the responder's rows (the physical nodes, then
 * the virtual nodes received so far) stops at a row once both halves of the request are 0; the float64
 * absolute differences against the row's free counters (Go uint64: the sign-extended u32 halves); a half
 * becomes 0 when its difference exceeds it, else shrinks by uint32(diff); every visited row gets a
 * Foreign job {uint(core_diff), uint(mem_diff)} from T to T + time_s (time_s = 0: logged, holds nothing,
 * takes no running slot; else the row's counter is reduced and may wrap, and a running slot is taken).
 * The records go to the Foreign log in array order, in row order within a request (mcs_read_foreign, an
 * open cursor's "appended since"); nothing goes to the contract log.  The second of two requests to one
 * responder sees the first one's commits.  n == 0 is MCS_OK.  One upload, two launches, one
 * synchronisation, whatever n is.
 *   MCS_E_INVALID: n > 4096, a null pointer, responder or requester not below mcs_num_clusters, t_last +
 * time_s > 0xFFFFFFFE.  MCS_E_STATE, with the cause in mcs_last_error: no trading session; external mode
 * off; no tick executed yet; the session failed; the run's flags carry a log or virtual-node overflow, as
 * the series calls refuse.  MCS_FLAG_T_MAX does not refuse: the tick at t_max_s raises it, the reference's
 * traders run their rounds at that tick too, and the clock then stays there (the grant reaches the logs
 * and the counters and no later decision).
 *   Capacity.  A call that overflows the running-slot pool (receive: the virtual-node pool) escalates as
 * mcs_run does (slots grow by half, virtual nodes x 4) and replays the session from t = 0: the engine
 * keeps every accepted call with the t_last it acted at, and a replay runs up to t + 1, applies that
 * tick's calls in order, and so on, then applies the call that triggered it (restarts counts the replay,
 * stats->replayed = 1, an open cursor rebuilds once).  With a fixed cfg.slot_pool or at the pools'
 * limits: MCS_E_CAPACITY and the session is failed until mcs_rewind.  mcs_rewind, a new submit and
 * mcs_load_clusters drop the kept calls. */
int mcs_trade_session_provide_vnodes(mcs_engine* eng, const mcs_vnode_request* req, uint32_t n,
                                     mcs_vnode_result* res, mcs_vnode_stats* stats /* may be NULL */);

typedef struct mcs_vnode_grant {
    uint32_t cluster, cores, memory, pad;
} mcs_vnode_grant;
/* AddVirtualNode for each entry, in array order: the cluster gets the row {cores, memory} with capacity
 * = free = the node's, behind its physical nodes and the virtual nodes received so far; {0, 0} is legal
 * (the zero contract).  The row takes part in the next tick's first fit; mcs_read_virtual_node_caps,
 * the series and the cursors show it.  Limits, refusals and capacity as mcs_trade_session_provide_vnodes
 * (MCS_E_CAPACITY at 256 virtual nodes per cluster). */
int mcs_trade_session_receive_vnodes(mcs_engine* eng, const mcs_vnode_grant* node, uint32_t n,
                                     mcs_vnode_stats* stats /* may be NULL */);
/* The live free counters of a cluster's rows (physical, then virtual) as the last executed tick and the
 * grants since left them, as Go uint64 (sign-extended): what an outside trader builds a NodeObject from.
 * *n = the row count (may exceed cap: then only cap rows are written).  Either mode of a trading session;
 * MCS_E_STATE without one, before its first tick and after it failed. */
int mcs_trade_session_read_nodes(mcs_engine* eng, uint32_t cluster, uint64_t* free_cores,
                                 uint64_t* free_memory, uint32_t cap, uint32_t* n);

/* ---- single-call mirror of the approval rule ---------------------------------------------------- */
/* Trader.ApproveTrade (pkg/trader/trader.go:141-167) with the reference's approvePolicy{0.8, 0.8, -1,
 * -1} (trader.go:47-52): a responder whose sample is {core_util, mem_util} and whose totals are
 * {total_cores, total_memory} (SetTotalResources, uint32) asked for the contract {cores, memory,
 * time_s, price 0}.  Evaluated on the GPU by the same device function both trader kernels call
 * (float32 availability T - T*u and float64 incentive in Go's order, no FMA contraction). */
typedef struct mcs_approve_query {
    uint32_t total_cores, total_memory;
    float core_util, mem_util;
    uint32_t cores, memory, time_s, pad;
} mcs_approve_query;

/* out[i] = 1 (approve) or 0 for each of the n queries. */
int mcs_approve_trade(mcs_engine* eng, const mcs_approve_query* q, uint32_t n, int32_t* out);

#ifdef __cplusplus
}
#endif
#endif /* MCS_TRADE_H */
