// mcs_internal.h — device data layout shared by the kernels and the C-ABI engine (libmcs.so).
//
// HBM layout:
//   jobs      uint4  {arrival_s, dur_s, cores, mem} per job, clusters contiguous (CSR job_off)  16 B/job
//   out_node  int32  per job; out_start, out_finish uint32 per job (SoA)                      12 B/job
//   node_free0 uint2 {free_c, free_m} per node (JSON CoresAvailable/MemoryAvailable), CSR node_off
//   node_cap   uint2 {cores, memory} per node; live_c/live_m uint32 per node (single-job mirrors)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mcs_trade.h"

namespace mcs {

constexpr uint32_t kEmpty = 0xFFFFFFFFu;  // empty running slot (finish time never reached)
constexpr int kWave = 64;
constexpr int kMaxNpl = 16;   // nodes per lane -> at most 1024 nodes per cluster in ABI v1
constexpr int kMaxPool = 32;  // running-slot registers per lane -> 2048 slots per cluster
constexpr uint32_t kAsmMaxJobs = (1u << 28) - 128u;  // hand-scheduled loop: 32-bit record offsets
constexpr uint32_t kJobPad = 128;  // records of slack after the job array (unmasked batch loads)

struct Totals {  // device-side accumulation of mcs_stats (only clusters that did not overflow)
    unsigned long long placed;
    unsigned long long waited;
    unsigned long long unplaced;
    unsigned int deadlocked;
    unsigned int overflowed;
    unsigned int clock_overflowed;  // clusters stopped by MCS_FLAG_CLOCK_OVERFLOW (run fails, MCS_E_RANGE)
    unsigned int bailed;            // DELAY clusters the hand-scheduled loop hands to delay_kernel
};

// In-kernel synthesis of the job stream (mcs_gen_dev.h): with `on` the FIFO and
// DELAY kernels generate each 64-job batch in registers and `jobs` is not read (may be null).
struct GenArgs {
    unsigned long long seed;
    double enl;             // exp(-lambda), resolved once on the host like mcs_generate_jobs
    const uint32_t* max_c;  // per-cluster maxima: setMaxCluster (client.go:68-83) or explicit
    const uint32_t* max_m;
    uint32_t mode;          // mcs_arrival_mode
    uint32_t max_dur;
    uint32_t base;          // global index of the engine's cluster 0 (mcs_set_shard)
    uint32_t on;
    const unsigned long long* wthr;  // WEIBULL gap table (mcs_gen.h), resolved on the host
    uint32_t wn;
    uint32_t pad;
};

// Online mode (mcs_run with a finite horizon, mcs_append_jobs): one record per
// cluster carried between horizons, plus the node image (the LDS layout of nodes[]) and the running
// slots.  valid == 0 starts the cluster from its spec at t = 0.
struct OnlineState {
    uint32_t valid;
    uint32_t t;       // the next loop iteration's time (not yet executed)
    uint32_t cursor;  // FIFO: ready cursor r; DELAY: Level0 head h
    uint32_t aux;     // FIFO: have_w (job r is the WaitQueue head); DELAY: len(Level1)
    uint32_t flags;
    uint32_t pool;    // slot rows saved in the slot image (rows >= pool are free)
    uint32_t placed, waited, peak, used, n_iter, n_rel, placed_l1, peak_l1;  // DELAY: waited = moved
    unsigned long long l1_t, mv_a, wsum;  // DELAY WaitTime sums (mcs_delay.hip)
};
constexpr uint32_t kSlotImg = 2u * kMaxPool * kWave;  // u64 words of one cluster's slot image

struct OnlineArgs {  // read only by the HOR kernel variants
    const uint32_t* job_cnt;   // jobs in each cluster's segment (job_off = segment starts)
    const OnlineState* st_in;  // state at the start of this horizon (read only: reruns reuse it)
    OnlineState* st_out;
    const unsigned long long* img_in;  // node image, img_stride words per cluster
    unsigned long long* img_out;
    const unsigned long long* slot_in;  // slot image: kSlotImg words per cluster ([cm rows][nf rows])
    unsigned long long* slot_out;
    uint32_t img_stride;
    uint32_t t_hor;  // stop before any iteration at t >= t_hor; kEmpty = drain
};

struct FifoArgs {
    const uint2* node_free0;
    const uint32_t* node_off;
    const uint4* jobs;
    const uint64_t* job_off;
    const uint32_t* cluster_list;  // grid item -> cluster (nullptr = identity)
    int32_t* out_node;
    uint32_t* out_start;
    uint32_t* out_finish;
    mcs_cluster_stats* cstats;
    Totals* totals;
    GenArgs gen;
    OnlineArgs on;
    uint32_t n_items;
    uint32_t guard_ok;  // bit 0: every node's free values < 2^31 - 1 (the hand-scheduled loop
                        // may run, W32 node format); bit 1: < 2^15 - 1 (W16 node format);
                        // bit 2: every cluster holds at most kAsmMaxJobs jobs
};

struct DelayArgs {
    const uint2* node_free0;
    const uint32_t* node_off;
    const uint4* jobs;
    const uint64_t* job_off;
    const uint32_t* cluster_list;  // grid item -> cluster (nullptr = identity)
    int32_t* out_node;
    uint32_t* out_start;
    uint32_t* out_finish;
    uint64_t* l1_cm;  // Level1 scratch, one entry per job: {cores | mem << 32}
    uint64_t* l1_jd;  //                                    {job | dur << 32}
    mcs_cluster_stats* cstats;
    mcs_delay_cluster_stats* dstats;
    Totals* totals;
    GenArgs gen;
    OnlineArgs on;
    uint32_t max_wait_s;
    uint32_t n_items;
};

// hor: the online variant (OnlineArgs; records streamed, never fused)
hipError_t launch_delay(const DelayArgs& a, int npl, int pool, bool hor, hipStream_t s);  // mcs_delay.hip
// the hand-scheduled DELAY loop (mcs_delay_asm.hip): Level1-empty iterations; a cluster whose head
// moves to Level1 stops with kDelayBail in its cstats flags and is re-run on delay_kernel
constexpr uint32_t kDelayBail = 0x40000000u;
bool delay_asm_eligible(int npl, int pool, uint32_t guard_ok, bool gen_on);
hipError_t launch_delay_asm(const DelayArgs& a, hipStream_t s);

// One lent run as the ClusterState kernels read it (mcs_state.hip, lent_scatter_kernel): the run
// holds {cores, mem} of node `node` of its lender over [start, finish); node >= the lender's
// physical node count is a zero-capacity virtual node (the run counts as running, no node row)
struct LentRun {
    uint32_t node, start, finish, cores;
    uint32_t mem, pad0, pad1, pad2;
};
static_assert(sizeof(LentRun) == 32, "two 16 B loads");

struct StateArgs {  // the ClusterState reduction over a run's placements (mcs_state.hip)
    const uint32_t* node_off;
    const uint2* cap;
    const uint2* free0;
    const uint4* jobs;
    const uint64_t* job_off;
    const int32_t* out_node;
    const uint32_t* out_start;
    const uint32_t* out_finish;
    mcs_cluster_state* out;
    uint32_t t;
    uint32_t n_clusters;
    // the second stream of a FIFO trading run (null after a plain run: the plain kernels never read
    // these): per lender the lent runs [lent_off[c], lent_off[c + 1]) of `lent`, in no promised order
    const uint32_t* lent_off;
    const LentRun* lent;
    const uint2* lent_summ;  // {earliest start from here on, finish_max} per kSeriesBatch lent runs
    // an online session (mcs_online_state_series; the SEG instantiations, which read nothing of the
    // second stream): cluster c's rows are the first job_cnt[c] of the segment that starts at
    // job_off[c].  Null for a batch run: the rows are then [job_off[c], job_off[c + 1]).
    const uint32_t* job_cnt;
};
hipError_t launch_state(const StateArgs& a, uint32_t max_n, hipStream_t s);  // mcs_state.hip

// The pre-pass over a FIFO trading run's lent log (mcs_state.hip): count per chunk and lender,
// exclusive scans, scatter with the borrower's cores and memory, summaries.  One engine holds the whole system
// (base 0): lender and borrower are local indices.
struct LentPrepArgs {
    const mcs_lent_rec* log;  // execution order
    uint64_t n;               // records in the log (below 2^32)
    const uint4* jobs;
    const uint64_t* job_off;
    uint32_t n_clusters;
    uint32_t n_chunks;  // lent_chunks(n)
    uint32_t* cnt;      // [n_chunks][n_clusters]: records per chunk and lender, then their offsets
    uint32_t* off;      // [n_clusters + 1]
    uint32_t* cursor;   // [n_clusters + 1]: the lists' lengths
    LentRun* runs;      // [n]
    uint2* summ;        // lent_summ_size() pairs
};
uint32_t lent_chunks(uint64_t n_lent);  // chunks of the log the pre-pass cuts it in
hipError_t launch_lent_prep(const LentPrepArgs& a, hipStream_t s);

// The ClusterState time series (mcs_state.hip, series_kernel): samples t0 + k * period, k < n_samples.
struct SeriesArgs {
    StateArgs s;              // the run's placements; s.out and s.t are not used
    uint2* summ;              // {arrival_min, end_max} per batch of kSeriesBatch jobs, series_summ_size() pairs
    mcs_cluster_sample* out;  // [s.n_clusters][n_samples], cluster-major
    uint32_t t0, period, n_samples;
    unsigned long long magic; // ceil(2^64 / period) for period >= 2: x / period = hi64(x * magic), x < 2^32
};
constexpr uint32_t kSeriesBatch = 256;        // jobs per summary pair
constexpr uint32_t kSeriesLds = 78u * 1024u;  // difference array budget: two workgroups per CU with the static LDS
constexpr uint32_t kSeriesMaxTile = 127;      // samples per tile at most (two sum lanes per sample)
constexpr uint32_t kSeriesRep = 16;           // copies of the running and the queued counter rows
__host__ __device__ inline uint32_t series_rows(uint32_t n_nodes) { return 2u * n_nodes + 2u * kSeriesRep + 2u; }
// samples per tile of a cluster of n_nodes nodes: series_rows LDS rows of u32; odd, so that the row
// stride puts neither the per-row prefix chains nor the per-sample sums on one bank
__host__ __device__ inline uint32_t series_tile(uint32_t n_nodes) {
    uint32_t ts = kSeriesLds / (4u * series_rows(n_nodes));
    if (ts > kSeriesMaxTile) ts = kSeriesMaxTile;
    return (ts - 1u) | 1u;
}
// cluster c's summaries start at job_off[c] / kSeriesBatch + c.  Over segments with slack the same
// index serves, with total_jobs the summed capacity job_off[n_clusters]: a segment holds at most its
// capacity, so its ceil(job_cnt[c] / kSeriesBatch) pairs end at or before
// floor(job_off[c + 1] / kSeriesBatch) + c + 1, where the next cluster's begin.
inline size_t series_summ_size(uint64_t total_jobs, uint32_t n_clusters) {
    return (size_t)(total_jobs / kSeriesBatch) + n_clusters + 1;
}
// lender c's lent-run summaries start at lent_off[c] / kSeriesBatch + c
inline size_t lent_summ_size(uint64_t n_lent, uint32_t n_clusters) {
    return (size_t)(n_lent / kSeriesBatch) + n_clusters + 1;
}
hipError_t launch_series_summary(const SeriesArgs& a, hipStream_t s);
hipError_t launch_state_series(const SeriesArgs& a, uint32_t max_n, hipStream_t s);

// The record after a DELAY trading run (mcs_state.hip, dt_state_kernel / dt_series_kernel; world 1,
// so global and local cluster indices coincide).  Cluster c has its N physical rows and then nv[c]
// virtual rows with cap = free0 = vcap[c * V + i]; counters are Go uint64.  The Foreign log is read
// as it is: launch order, every responder's records interleaved.
struct DtStateArgs {
    StateArgs s;                  // the run's placements (lent_* stay null)
    const uint2* vcap;            // [s.n_clusters][V]
    const uint32_t* nv;           // [s.n_clusters], each at most V
    const mcs_foreign_rec* flog;  // n_foreign records
    uint32_t n_foreign;
    uint32_t V;
};
struct DtSeriesArgs {
    DtStateArgs d;            // d.s.out and d.s.t are not used
    uint2* summ;              // as SeriesArgs::summ (the TRADE summaries: end = finish of every placed job)
    mcs_cluster_sample* out;  // [d.s.n_clusters][n_samples], cluster-major
    uint32_t t0, period, n_samples;
    unsigned long long magic;
    // a trading session's call (d.s.job_cnt set) with the pre-pass: dt_foreign_live_kernel's list of the
    // Foreign records that can hold at one of the call's samples, scanned in place of d.flog, and its
    // length on the device (at most d.n_foreign).  Null: the log is scanned as it is.
    const mcs_foreign_rec* live;
    const uint32_t* live_n;
};
// samples per tile of a cluster of nn = N + nv rows: 2 nn LDS rows of u64, then the u32 rows of
// series_rows(0); odd, as series_tile.  nn <= 1280 leaves a tile of 3 samples.
__host__ __device__ inline uint32_t dt_series_bytes(uint32_t nn) { return 16u * nn + 4u * series_rows(0); }
__host__ __device__ inline uint32_t dt_series_tile(uint32_t nn) {
    uint32_t ts = kSeriesLds / dt_series_bytes(nn);
    if (ts > kSeriesMaxTile) ts = kSeriesMaxTile;
    return (ts - 1u) | 1u;
}
hipError_t launch_dt_state(const DtStateArgs& a, uint32_t max_nn, hipStream_t s);
hipError_t launch_dt_series_summary(const DtSeriesArgs& a, hipStream_t s);
hipError_t launch_dt_state_series(const DtSeriesArgs& a, uint32_t max_nn, hipStream_t s);
hipError_t launch_dt_foreign_live(const mcs_foreign_rec* flog, uint32_t n_foreign, uint32_t t_first, uint32_t t_last,
                                  mcs_foreign_rec* live, uint32_t* live_n, hipStream_t s);
// The Foreign take of a trading session's stream (mcs_state.hip, dt_stream_foreign_kernel; once per
// mcs_trade_stream_next call that writes samples): the list the call's tiles scan, built from the list
// the last call kept (its records with finish_s > t_first) and the log records appended since, at
// [seen, n_log) (those with start_s != finish_s and finish_s > t_first).  t_first is the call's first
// sample second: a record holds on start_s < t < finish_s, so none with finish_s <= t_first is seen at or
// after it.  Two lists in ping-pong, each with room for `cap` >= n_log records, so that the new one
// cannot overflow (the store is guarded all the same).  The kernel also writes the call's row counts:
// nv_out[c] = min(nv_src[c * nv_stride], V), the value dt_series_kernel and stream_retire_kernel read.
struct DtStreamForeignArgs {
    const mcs_foreign_rec* flog;
    const mcs_foreign_rec* old_list;
    mcs_foreign_rec* new_list;
    uint32_t* new_n;          // zeroed by the launcher; afterwards the new list's length
    uint32_t old_n;           // the old list's length (the host read it back after the last call)
    uint32_t seen, n_log;     // log positions
    uint32_t t_first;
    uint32_t cap;             // records either list has room for
    const uint32_t* nv_src;   // DtCluster::nv of cluster 0
    uint32_t nv_stride;       // words between two clusters' nv
    uint32_t V, n_clusters;
    uint32_t* nv_out;         // [n_clusters]
};
hipError_t launch_dt_stream_foreign(const DtStreamForeignArgs& a, hipStream_t s);

// The average wait time series of a DELAY run (mcs_wait.hip): WaitTime after the Delay iteration at
// the seconds t0 + k * period, k < n_samples, of the first n_clusters clusters.
struct WaitArgs {
    const uint4* jobs;
    const uint64_t* job_off;
    const uint32_t* job_cnt;  // an online session: the rows of each segment (StateArgs::job_cnt); else null
    const int32_t* out_node;
    const uint32_t* out_start;
    uint4* rec;            // per job {h, m, s, arrival}: wait_prep_kernel
    uint2* ev;             // per job {the entry its Level1 placement steps over, that entry's run}: wait_skip_kernel
    mcs_wait_sample* out;  // [n_clusters][n_samples], cluster-major
    uint32_t max_wait, t0, period, n_samples, n_clusters;
    uint64_t rec_off;      // rec[0] is row rec_off of the job array (0: rec covers every row; ev always does)
};
hipError_t launch_wait_rec(const WaitArgs& a, hipStream_t s);     // rec alone: the clamp scan (mcs_level1.hip reads it)
hipError_t launch_wait_prep(const WaitArgs& a, hipStream_t s);    // rec and ev: once per call
hipError_t launch_wait_series(const WaitArgs& a, hipStream_t s);  // one chunk of samples
hipError_t launch_wait_finish(const WaitArgs& a, hipStream_t s);  // wait_finish_kernel alone (mcs_stream.hip)

// The start-stream cursor of an online session (mcs_stream.hip, mcs_stream_next): what
// is kept per cluster between calls.  The unit is the batch of kSeriesBatch rows counted from the
// cluster's first row; per batch the engine keeps a flag word, the summary pair of SeriesArgs::summ and
// the batch's sum of s - a, all indexed as the summaries are (job_off[c] / kSeriesBatch + c), and per
// row the wait record {h, m, s, a} of WaitArgs::rec (a stream with wait statistics only).
struct StreamCluster {
    long long d_carry;                // d of row p - 1 of wait_prep's recurrence (-1 before row 0)
    unsigned long long a_base;        // sum of s - a over the rows of the retired batches (mod 2^64)
    uint32_t p;                       // rows whose d is final (d below the horizon): a prefix
    uint32_t first_live;              // every batch below this one is retired
};
constexpr uint32_t kStreamFinal = 1u;    // a full batch whose rows are all decided: summary, records and sum stay
constexpr uint32_t kStreamRetired = 2u;  // final, and every finish below the frontier: no per-job loop reads it
constexpr uint32_t kStreamLoaded = 4u;   // stream_prep_kernel read its rows in this call
struct StreamArgs {
    StateArgs s;               // the session's segments (job_cnt set); s.out and s.t are not used
    StreamCluster* cl;         // [s.n_clusters]
    uint32_t* flags;           // per batch
    uint2* summ;               // per batch: SeriesArgs::summ
    unsigned long long* bsum;  // per final batch: sum of s - a over its rows
    uint4* rec;                // per row {h, m, s, arrival}; null without the wait statistics and Level1
    mcs_wait_sample* wout;     // [s.n_clusters][n_samples] accumulators (stream_accum_kernel)
    unsigned long long* tot;   // [0] rows this call loaded, [1] rows in retired batches
    uint32_t hor;              // the last finite horizon: d below it is final
    uint32_t max_wait;
    uint32_t t0, period, n_samples;  // accum: the chunk; retire: the whole call
    uint32_t chunk;            // retire: samples per chunk of the call's series launches
    uint32_t frontier;         // retire: the stream's next sample second after this call
};
// A trading session's stream (mcs_trade_stream_next): the TRADE instantiation of the retire kernel takes
// the plain arguments and, behind them, per cluster the virtual rows of this call, min(nv, V), on the
// device.  The plain kernels' parameter keeps its layout (as DtArgsCore / DtArgs).
struct TradeStreamArgs : StreamArgs {
    const uint32_t* nv;
};
hipError_t launch_stream_prep(const StreamArgs& a, hipStream_t s);    // summaries, records, final flags
hipError_t launch_stream_accum(const StreamArgs& a, hipStream_t s);   // the live batches into wout
hipError_t launch_stream_retire(const StreamArgs& a, hipStream_t s);  // retire against the frontier, count
hipError_t launch_trade_stream_prep(const StreamArgs& a, hipStream_t s);  // the TRADE forms of both
hipError_t launch_trade_stream_retire(const TradeStreamArgs& a, hipStream_t s);
// the kept arrays after a segment relayout: cluster c's batches and rows move from the old layout
// (old_off) to the new one (s.job_off); s.job_cnt are the rows before the append
struct StreamMoveArgs {
    const uint64_t* old_off;
    const uint64_t* new_off;
    const uint32_t* job_cnt;
    const uint32_t* flags_o;
    uint32_t* flags_n;
    const uint2* summ_o;
    uint2* summ_n;
    const unsigned long long* bsum_o;
    unsigned long long* bsum_n;
    const uint4* rec_o;  // null without the records (neither wait statistics nor Level1)
    uint4* rec_n;
    const uint32_t* l1s_o;  // null without Level1: StreamLevel1Args::l1s
    uint32_t* l1s_n;
    uint32_t n_clusters;
};
hipError_t launch_stream_move(const StreamMoveArgs& a, hipStream_t s);
// Level1 samples on a cursor (mcs_stream_open_level1; DESIGN.md §14 "Level1 on the cursors"): per batch
// the kept Level1 summary (the largest s among the rows that move, as level1_summary_kernel defines it;
// a final batch keeps it), per cluster the scan bounds {lo, hi} of level1_series_kernel carried from the
// call's last sample to the next call's first.  The records are the stream's kept ones.
struct StreamLevel1Args {
    const uint4* jobs;
    const uint64_t* job_off;
    const uint32_t* job_cnt;
    const StreamCluster* cl;   // first_live: every batch below it is retired and holds no member
    const uint32_t* flags;     // summary refresh: the batches prep loaded in this call (kStreamLoaded)
    const uint4* rec;
    uint32_t* l1s;             // per batch, indexed as the other kept arrays
    uint2* carry;              // [n_clusters] {lo, hi}
    mcs_level1_sample* out;    // [n_clusters][n_samples], cluster-major
    unsigned long long* rows;  // rows with lo <= j < hi inside the scanned batches, added per wave
    uint32_t t0, period, n_samples, n_clusters;
    uint32_t fresh;            // 1: nothing is carried (after open or a rebuild): hi by bisection from row 0
};
hipError_t launch_stream_level1_summ(const StreamLevel1Args& a, hipStream_t s);  // once per call, after prep
hipError_t launch_stream_level1(const StreamLevel1Args& a, hipStream_t s);       // one chunk of samples

// The Level1 list over time (mcs_level1.hip): len(Level1), both contract sizes and the head row after
// the Delay iteration at the seconds t0 + k * period, k < n_samples, of the first n_clusters clusters,
// from wait_prep_kernel's records; and the member rows of one cluster at one second.
struct Level1Args {
    const uint4* jobs;
    const uint64_t* job_off;
    const uint32_t* job_cnt;  // an online session: the rows of each segment (WaitArgs::job_cnt); else null
    const uint4* rec;         // WaitArgs::rec
    uint64_t rec_off;         // WaitArgs::rec_off
    uint32_t* summ;           // per kSeriesBatch jobs the largest s among the jobs that move to Level1,
                              // indexed as SeriesArgs::summ (series_summ_size words); the list kernel reads none
    mcs_level1_sample* out;   // [n_clusters][n_samples], cluster-major
    uint32_t t0, period, n_samples, n_clusters;
    uint32_t n_tiles;         // ceil(n_samples / kLevel1Tile)
    // the list kernel: cluster 0 of job_off at second t0
    uint32_t cap;             // rows has room for cap entries
    uint32_t* rows;
    uint32_t* n_out;          // len(Level1), whatever cap is
};
constexpr uint32_t kLevel1Tile = 32;  // samples one workgroup walks, its scan bounds carried along
hipError_t launch_level1_summary(const Level1Args& a, hipStream_t s);  // summ: once per call
hipError_t launch_level1_series(const Level1Args& a, hipStream_t s);   // one chunk of samples
hipError_t launch_level1_list(const Level1Args& a, hipStream_t s);

// Launchers (mcs_kernels.hip).  Return hipSuccess or the launch error.
hipError_t launch_fifo(const FifoArgs& a, int npl, int pool, bool hor, hipStream_t s);
uint32_t cu_count();  // CUs of the current device (256 on MI355X)
// the low-occupancy forms are picked for grids of at most this many cluster waves per CU
constexpr uint32_t kLatWavesPerCu = 4;
bool fifo_variant_exists(int npl, int pool);
// the hand-scheduled decision loop (mcs_fifo_asm.hip): NPL 4 / P 8 or NPL 1 / P 2, streamed
// batch runs; MCS_FIFO_ASM=0 turns it off
bool fifo_asm_eligible(const FifoArgs& a, int npl, int pool, bool hor);
// the kernel a FIFO batch run takes (the numbers are the form codes of DESIGN.md and profiles/; 21,
// the duo loop, and 22, the one-job lookahead, are retired)
enum FifoForm : int {
    kFormCompiled = 0,    // fifo_kernel (mcs_kernels.hip)
    kFormW16 = 16,        // 16-bit node format, running slots in LDS (MCS_FIFO_ASM=16 only)
    kFormW16R = 17,       // 16-bit node format, running slots in registers: NPL 4 / P 8
    kFormW16S = 18,       // W16R for clusters of at most 64 nodes: NPL 1 / P 2
    kFormW16RFused = 19,  // W16R / W16S on a fused job stream
    kFormW16SFused = 20,
    kFormW32 = 32,        // 32-bit node format, running slots in LDS
};
FifoForm fifo_asm_form(const FifoArgs& a, int npl, int pool, bool hor);
const char* fifo_form_name(FifoForm form);  // what mcs_last_kernel reports for it
hipError_t launch_fifo_asm(const FifoArgs& a, int npl, int pool, hipStream_t s);
hipError_t launch_gen_attrs(uint4* jobs, const uint64_t* job_off, const uint32_t* max_c,
                            const uint32_t* max_m, uint32_t n_clusters, uint64_t seed,
                            uint32_t max_dur, uint32_t cluster_base, hipStream_t s);
hipError_t launch_gen_arrivals(uint4* jobs, const uint64_t* job_off, uint32_t n_clusters, const GenArgs& g,
                               hipStream_t s);
// whole records through GenStream, one wave per cluster (every cluster below 2^32 jobs)
hipError_t launch_gen_stream(uint4* jobs, const uint64_t* job_off, uint32_t n_clusters, const GenArgs& g,
                             hipStream_t s);
hipError_t launch_gen_bound(const uint64_t* job_off, uint32_t n_clusters, const GenArgs& g,
                            unsigned long long* last, hipStream_t s);
hipError_t launch_schedule_one(uint32_t* live_c, uint32_t* live_m, uint32_t n, uint32_t c,
                               uint32_t m, int32_t* out_node, hipStream_t s);
hipError_t launch_lend_check(const uint32_t* live_c, const uint32_t* live_m, uint32_t n,
                             uint32_t c, uint32_t m, int32_t* out_ok, hipStream_t s);
hipError_t launch_utilization(const uint2* cap, const uint32_t* live_c, const uint32_t* live_m,
                              uint32_t n, float* out2, hipStream_t s);

}  // namespace mcs
