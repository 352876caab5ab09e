"""GPU parity of the ClusterState record and its time series after a FIFO trading run (policy FIFO with
borrow and/or trader; csrc/mcs_state.hip, the TRADE instantiations and the lent-run pre-pass).

The record at second t of a cluster (include/mcs.h):
  - a node is held by every own job placed on it with start <= t < finish and by every lent run of
    this lender with start <= t < finish, which holds the cores and memory of the borrower's job;
  - running = own jobs plus lent runs holding at t;
  - queued = own jobs with arrival <= t that have not left the Ready and Wait queues by t: a borrowed
    job (node -2, start = the borrow tick) is queued on [arrival, start), a job undecided at t_max_s
    (node -1) stays queued, LentQueue entries are not counted;
  - a node index at or above the physical node count is a zero-capacity virtual node: the record
    counts as placed and running and adds nothing to any node.

trade_series_ref builds that record by brute force per sample from the oracle's trade run
(oracle/mcs_oracle_trade.c): it subtracts the own and the lent usage from the free vectors and calls
the oracle's GetResourceUtilization.  Every comparison is bit for bit (NaNs equal)."""
import json
import os

import numpy as np
import pytest

import oracle_ref as O
from kat_util import GOLDEN, seeded_workload
from mcs_amd import CLUSTER_SAMPLE_DTYPE, ClusterArrays, Engine, JobStreams, MCSError, replicate, uniform_cluster
from mcs_amd import _lib as L
from mcs_amd.shard import run_lockstep
from test_gpu_state_series import assert_matches_single_call, assert_samples_equal, concat, tile
from test_trade_oracle import kat_inputs, lent_rows

pytestmark = pytest.mark.gpu

T_MAX = 20_000_000  # a stuck clock ends the run (flagged) instead of spinning


# ---- the host reference ---------------------------------------------------------------------------
def trade_series_ref(arrays, streams, res, t0, period, n, with_lent=True, borrowed_leaves=True):
    """res: node, start, finish of the own jobs and the lent log (LENT_DTYPE, `job` a global job
    index) of O.trade_run.  with_lent=False leaves the lent runs out; borrowed_leaves=False keeps a
    borrowed job queued for good: the two wrong readings the tests tell from the right one."""
    node, start, fin, lent = res["node"], res["start"], res["finish"], res["lent"]
    out = np.zeros((arrays.n_clusters, n), CLUSTER_SAMPLE_DTYPE)
    for c in range(arrays.n_clusters):
        ns, js = arrays.nodes_of(c), streams.of(c)
        nn = ns.stop - ns.start
        nd, st, fi = node[js].astype(np.int64), start[js].astype(np.int64), fin[js].astype(np.int64)
        arr = streams.arrival[js].astype(np.int64)
        cores, mem = streams.cores[js].astype(np.float64), streams.mem[js].astype(np.float64)
        lr = lent[lent["lender"] == c] if with_lent else lent[:0]
        ln, ls, lf = lr["node"].astype(np.int64), lr["start"].astype(np.int64), lr["finish"].astype(np.int64)
        lj = lr["job"].astype(np.int64)
        lc, lm = streams.cores[lj].astype(np.float64), streams.mem[lj].astype(np.float64)
        left = (nd >= 0) | (nd == -2) if borrowed_leaves else nd >= 0
        for k in range(n):
            t = t0 + k * period
            run = (nd >= 0) & (st <= t) & (fi > t)
            lrun = (ls <= t) & (lf > t)
            p, lp = run & (nd < nn), lrun & (ln < nn)  # a virtual node has no counters
            uc = (np.bincount(nd[p], weights=cores[p], minlength=nn) +
                  np.bincount(ln[lp], weights=lc[lp], minlength=nn)).astype(np.uint64)
            um = (np.bincount(nd[p], weights=mem[p], minlength=nn) +
                  np.bincount(ln[lp], weights=lm[lp], minlength=nn)).astype(np.uint64)
            cu, mu = O.resource_utilization(arrays.cap_c[ns], arrays.cap_m[ns], arrays.free_c[ns].astype(np.uint64) - uc,
                                            arrays.free_m[ns].astype(np.uint64) - um)
            queued = (arr <= t) & (~left | (st > t))
            out[c, k] = (np.float32(cu), np.float32(mu), int(run.sum()) + int(lrun.sum()), int(queued.sum()))
    return out


def oracle_trade(arrays, streams, borrow=True, trader=True, **kw):
    return O.trade_run(arrays, streams, borrow=borrow, trader=trader, **kw)


def local_lent_rows(res, streams):
    """The oracle's lent log with the job as an index within the borrower's stream (the ABI's)."""
    rows = lent_rows(res["lent"])
    for r in rows:
        r[2] -= int(streams.job_off[r[1]])
    return sorted(rows)


def assert_run_is_the_oracles(eng, streams, o):
    node, start, fin = eng.placements()
    np.testing.assert_array_equal(node, o["node"])
    np.testing.assert_array_equal(start, o["start"])
    np.testing.assert_array_equal(fin, o["finish"])
    assert lent_rows(eng.lent()) == local_lent_rows(o, streams)


def trading_engine(arrays, streams, borrow=True, trader=True, **cfg):
    cfg.setdefault("t_max_s", T_MAX)
    eng = Engine(0, borrow=borrow, trader=trader, **cfg)
    eng.load_clusters(arrays)
    eng.submit_jobs(streams)
    return eng


# ---- 1. parity at every second ---------------------------------------------------------------------
def workload_p():
    """A hot borrowing system: six 64-node clusters at 120 % load, 250 jobs each."""
    arrays, streams, _ = seeded_workload("n64_hot", 6, 250)
    return arrays, streams


def parity_conditions(arrays, streams, o, n):
    """The four properties that make the parity test tell the record from its wrong readings, from
    the oracle alone.  Returns the reference series."""
    lent = o["lent"]
    assert (lent["finish"] > lent["start"]).any()  # a lent run that holds something
    assert (o["node"] == -2).any()  # a borrowed job
    ref = trade_series_ref(arrays, streams, o, 0, 1, n)
    no_lent = trade_series_ref(arrays, streams, o, 0, 1, n, with_lent=False)
    assert (ref["cores_utilization"].view(np.uint32) != no_lent["cores_utilization"].view(np.uint32)).any()
    stay = trade_series_ref(arrays, streams, o, 0, 1, n, borrowed_leaves=False)
    assert (ref["queued"] != stay["queued"]).any()
    return ref


@pytest.fixture(scope="module")
def run_p():
    arrays, streams = workload_p()
    o = oracle_trade(arrays, streams)
    n = int(o["t_final"]) + 6  # [0, t_final + 5]
    ref = parity_conditions(arrays, streams, o, n)
    with trading_engine(arrays, streams) as eng:
        eng.run()
        assert_run_is_the_oracles(eng, streams, o)
        yield eng, arrays, streams, o, n, ref


def test_trade_series_matches_host_reference_every_second(run_p):
    eng, arrays, streams, o, n, ref = run_p
    samples, first = eng.cluster_state_series(0, 1, n)
    assert_samples_equal(samples, ref)
    assert_matches_single_call(eng, samples, 0, 1, range(0, n, 37))
    assert first.tobytes() == eng.cluster_states(0).tobytes()


def test_trade_series_at_the_reference_cadence(run_p):
    eng, arrays, streams, o, n, ref = run_p
    samples, first = eng.cluster_state_series(0, 5, (n + 4) // 5)
    assert_samples_equal(samples, ref[:, ::5])


def test_wire_start_stream_takes_a_trading_row(run_p):
    from mcs_amd import wire

    eng, arrays, streams, o, n, ref = run_p
    samples, first = eng.cluster_state_series(0, 5, 8)
    msgs = wire.start_stream(samples[1], first[1])
    assert len(msgs) == 8


# ---- 2. a hand-built system, fixed answers ---------------------------------------------------------
def load_state_kat():
    with open(os.path.join(GOLDEN, "kats_trade_state.json")) as f:
        return json.load(f)["kats"][0]


def kat_expected(k):
    """(n_clusters, n) samples from the fixture's per-second rows [cu, mu, running, queued]."""
    rows = np.array(k["expect"]["samples"], np.float64)
    out = np.zeros(rows.shape[:2], CLUSTER_SAMPLE_DTYPE)
    out["cores_utilization"], out["memory_utilization"] = rows[..., 0].astype(np.float32), rows[..., 1].astype(np.float32)
    out["running"], out["queued"] = rows[..., 2].astype(np.uint32), rows[..., 3].astype(np.uint32)
    return out


def test_hand_built_borrow():
    k = load_state_kat()
    arrays, streams = kat_inputs(k)
    want = kat_expected(k)
    with trading_engine(arrays, streams, borrow=True, trader=False) as eng:
        eng.run()
        node, start, fin = eng.placements()
        assert node.tolist() == k["expect"]["node"] and start.tolist() == k["expect"]["start"]
        samples, first = eng.cluster_state_series(0, 1, want.shape[1])
        assert_samples_equal(samples, want)
        assert_matches_single_call(eng, samples, 0, 1, range(want.shape[1]))


# ---- 3. tile and chunk edges -----------------------------------------------------------------------
PERIOD = 5


def workload_e():
    """Lenders of 256 nodes (tiles of 35 samples) and of 320 nodes (tiles of 29, below a wave), and one
    5-node borrower whose nodes are filled, so that every later job of its stream is borrowed on arrival
    and run by both lenders from the next second.  Arrivals and durations put the lent runs' starts on
    a tile's last sample, their ends on a tile's first sample, and one run across several tiles."""
    small = seeded_workload("small", 1, 1)[0]
    ts = (tile(256), tile(320))
    assert ts == (35, 29)
    jobs = [(0, 20000, int(c), int(m)) for c, m in zip(small.cap_c, small.cap_m)]  # every node full
    for t in ts:
        e = t * PERIOD  # second of tile 1's first sample
        jobs.append((e - PERIOD - 1, PERIOD + 1, 1, 1))      # runs on [e - 5, e + 1): starts on tile 0's last sample
        jobs.append((e - 3 * PERIOD - 1, 3 * PERIOD, 2, 3))  # runs on [e - 15, e): over at tile 1's first sample
        jobs.append((e + 7, 3 * e, 3, 2))                    # spans more than one tile
    jobs.sort()
    own = JobStreams(*(np.array([j[f] for j in jobs], np.uint32) for f in (0, 1, 2, 3)), np.array([0, len(jobs)], np.uint64))
    none = JobStreams(*(np.zeros(0, np.uint32) for _ in range(4)), np.zeros(2, np.uint64))
    return concat([(replicate(uniform_cluster(256), 1), none), (replicate(uniform_cluster(320), 1), none), (small, own)])


def test_tile_and_chunk_edges(monkeypatch):
    arrays, streams = workload_e()
    o = oracle_trade(arrays, streams, borrow=True, trader=False)
    lent = o["lent"]
    assert (o["node"] == -2).sum() == 6 and len(lent) == 12  # both lenders run every borrowed job
    n = int(lent["finish"].max()) // PERIOD + 4
    for c, ts in ((0, 35), (1, 29)):
        lr = lent[lent["lender"] == c]
        k_s, k_f = -(-lr["start"].astype(np.int64) // PERIOD), -(-lr["finish"].astype(np.int64) // PERIOD)  # first sample at or after
        assert ((k_s % ts == ts - 1) & (k_f > k_s)).any()        # starts on a tile's last sample
        assert ((k_f % ts == 0) & (k_f > k_s)).any()             # ends on a tile's first sample
        assert (k_f // ts - k_s // ts >= 2).any()                # spans more than one tile
    ref = trade_series_ref(arrays, streams, o, 0, PERIOD, n)
    with trading_engine(arrays, streams, borrow=True, trader=False) as eng:
        eng.run()
        assert_run_is_the_oracles(eng, streams, o)
        whole, first = eng.cluster_state_series(0, PERIOD, n)
        assert_samples_equal(whole, ref)
        assert whole["running"][:2].max() >= 2
        monkeypatch.setenv("MCS_SERIES_CHUNK", "7")
        parts, first2 = eng.cluster_state_series(0, PERIOD, n)
        assert parts.tobytes() == whole.tobytes() and first2.tobytes() == first.tobytes()


# ---- 4. trader only, borrow only -------------------------------------------------------------------
def test_trader_only_equals_the_plain_run():
    """The trader alone leaves every placement unchanged and adds zero-capacity virtual nodes: the
    series of the trading run is, bit for bit, the series of the same streams on a plain engine."""
    arrays, streams, _ = seeded_workload("n64_hot", 4, 300)
    with trading_engine(arrays, streams, borrow=False, trader=True) as eng:
        eng.run()
        assert eng.virtual_nodes().sum() > 0 and len(eng.lent()) == 0
        node, start, fin = eng.placements()
        n = int(fin[node >= 0].max()) // 3 + 5
        got = eng.cluster_state_series(0, 3, n)
        one = eng.cluster_states(int(np.median(start)))
    with Engine(0, policy="FIFO") as eng:
        eng.load_clusters(arrays)
        eng.submit_jobs(streams)
        eng.run()
        want = eng.cluster_state_series(0, 3, n)
        assert one.tobytes() == eng.cluster_states(int(np.median(start))).tobytes()
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
    assert got[0]["running"].max() > 0 and got[0]["queued"].max() > 0


def test_borrow_only():
    arrays, streams, _ = seeded_workload("n64_hot", 4, 300)
    o = oracle_trade(arrays, streams, borrow=True, trader=False)
    assert len(o["lent"]) > 0 and (o["node"] == -2).any()
    n = int(o["t_final"]) // 3 + 40
    with trading_engine(arrays, streams, borrow=True, trader=False) as eng:
        eng.run()
        assert_run_is_the_oracles(eng, streams, o)
        samples, first = eng.cluster_state_series(0, 3, n)
        assert_samples_equal(samples, trade_series_ref(arrays, streams, o, 0, 3, n))
        assert_matches_single_call(eng, samples, 0, 3, range(0, n, 23))


def test_lent_lists_of_several_batches_and_log_chunks():
    """16 cluster_small replicas: each lender's list holds several batches of 256 lent runs, the log
    several chunks of the pre-pass (4096 records), and the series 18 tiles of 127 samples, so that the
    cursor over the lent summaries moves from tile to tile."""
    arrays, streams, _ = seeded_workload("small", 16, 300)
    o = oracle_trade(arrays, streams)
    lent = o["lent"]
    per_lender = np.bincount(lent["lender"], minlength=16)
    assert len(lent) > 3 * 4096 and per_lender.max() > 4 * 256 and per_lender.min() > 256
    period = 25
    n = int(lent["finish"].max()) // period + 5
    assert n > 16 * tile(5)
    with trading_engine(arrays, streams) as eng:
        eng.run()
        assert_run_is_the_oracles(eng, streams, o)
        samples, first = eng.cluster_state_series(0, period, n)
        assert_samples_equal(samples, trade_series_ref(arrays, streams, o, 0, period, n))
        assert_matches_single_call(eng, samples, 0, period, range(0, n, 97))
        assert (samples["running"][:, -1] == 0).all()


# ---- 5. t_max_s reached ----------------------------------------------------------------------------
def test_undecided_jobs_stay_queued():
    arrays, streams, _ = seeded_workload("n64_hot", 4, 300)
    t_max = int(np.median(streams.arrival))
    o = oracle_trade(arrays, streams, t_max=t_max)
    undecided = np.array([(o["node"][streams.of(c)] == -1).sum() for c in range(4)])
    assert (undecided > 0).all()
    n = int(streams.arrival.max()) // 7 + 30
    with trading_engine(arrays, streams, t_max_s=t_max) as eng:
        eng.run()
        assert_run_is_the_oracles(eng, streams, o)
        samples, first = eng.cluster_state_series(0, 7, n)
        assert_samples_equal(samples, trade_series_ref(arrays, streams, o, 0, 7, n))
        assert (samples["queued"][:, -1] == undecided).all()
        late = eng.cluster_states(0xFFFFFFF0)
        assert (late["running"] == 0).all()


# ---- 6. caller-driven, world 1 ---------------------------------------------------------------------
def test_caller_driven_equals_run():
    arrays, streams, _ = seeded_workload("n64_hot", 4, 300)
    got = []
    for driven in (False, True):
        with trading_engine(arrays, streams) as eng:
            if driven:
                run_lockstep(eng, lambda b: b)
            else:
                eng.run()
            n = int(eng.trade_stats()["t_final"]) // 5 + 10
            got.append(eng.cluster_state_series(0, 5, n))
    assert got[0][0].tobytes() == got[1][0].tobytes() and got[0][1].tobytes() == got[1][1].tobytes()
    assert got[0][0]["running"].max() > 0


# ---- 7. refusals -----------------------------------------------------------------------------------
def assert_state_refused(eng, word):
    for call in (lambda: eng.cluster_states(10), lambda: eng.cluster_state_series(0, 5, 10)):
        with pytest.raises(MCSError) as ei:
            call()
        assert ei.value.code == L.MCS_E_STATE and word in str(ei.value), str(ei.value)


def test_refused_on_a_sharded_engine():
    """Rank 0 of a world of 2 whose peer is a second engine in this process: the blocks are exchanged
    by hand.  A lent record does not carry the job's cores and memory, and the borrower's job records
    live on the other rank."""
    arrays, streams, _ = seeded_workload("n64_hot", 4, 120)
    half = [(ClusterArrays(*(getattr(arrays, f)[arrays.nodes_of(2 * r).start:arrays.nodes_of(2 * r + 1).stop]
                             for f in ("cap_c", "cap_m", "free_c", "free_m")),
                           (arrays.node_off[2 * r:2 * r + 3] - arrays.node_off[2 * r]).astype(np.uint32)),
             JobStreams(*(getattr(streams, f)[int(streams.job_off[2 * r]):int(streams.job_off[2 * r + 2])]
                          for f in ("arrival", "dur", "cores", "mem")),
                        (streams.job_off[2 * r:2 * r + 3] - streams.job_off[2 * r]).astype(np.uint64)))
            for r in range(2)]
    engs = []
    try:
        for r in range(2):
            eng = Engine(0, borrow=True, trader=True, t_max_s=T_MAX)
            engs.append(eng)
            eng.load_clusters(half[r][0])
            eng.set_shard(r, 2)
            eng.submit_jobs(half[r][1])
        words = np.maximum(engs[0].trade_shape_words(), engs[1].trade_shape_words())
        for eng in engs:
            eng.trade_set_shape(words)
            eng.trade_begin()
        done = False
        for _ in range(100000):
            blocks = np.concatenate([eng.trade_phase(0, None)[0] for eng in engs])
            for eng in engs:
                eng.trade_phase(1, blocks)
                eng.trade_phase(2, None)
            done = [eng.trade_phase(3, None)[1] for eng in engs]
            assert done[0] == done[1]
            if done[0]:
                break
        assert done[0]
        for eng in engs:
            eng.trade_end()
        assert_state_refused(engs[0], "shard")
    finally:
        for eng in engs:
            eng.close()


def test_refused_after_an_overflow(monkeypatch):
    arrays, streams, _ = seeded_workload("n64_hot", 4, 300)
    assert len(oracle_trade(arrays, streams)["lent"]) > 8
    with trading_engine(arrays, streams, lent_queue_cap=1) as eng:  # a LentQueue overflows: the run is cut short
        with pytest.raises(MCSError):
            eng.run()
        assert_state_refused(eng, "overflow")
    monkeypatch.setenv("MCS_TRADE_LENT_LOG_CAP", "8")  # the lent log drops records
    with trading_engine(arrays, streams) as eng:
        eng.run()
        assert eng.trade_stats()["flags"] & 0x10  # MCS_FLAG_LOG_OVERFLOW
        assert_state_refused(eng, "MCS_FLAG_LOG_OVERFLOW")


# ---- 8. a virtual-node index ------------------------------------------------------------------------
def test_cluster_without_physical_nodes():
    """Only a 0-core 0-memory job can take a zero-capacity virtual node, and such a job fits any
    physical node first, so a node index >= N needs a cluster without physical nodes that won a trade.
    That system is accepted, but it never gets there: the utilization of a node-less cluster is
    0 / 0 = NaN, no NaN breaks the request policy (trader.go:127-130), so the cluster never requests
    and its jobs stay undecided up to t_max_s.  What is left to check on the GPU is the record of such
    a cluster after a trading run: NaN utilization, nothing running, its jobs queued.  In the kernels
    the index guard (k < N before any row index) holds by construction."""
    k = {"clusters": [[], [[10, 10]]], "jobs": [[[0, 0, 0, 50], [3, 0, 0, 10]], [[0, 9, 9, 30]]]}
    arrays, streams = kat_inputs(k)
    o = oracle_trade(arrays, streams, borrow=False, trader=True, t_max=40)
    assert o["node"].tolist() == [-1, -1, 0] and o["virtual_nodes"].tolist() == [0, 0] and o["t_final"] == 40
    n = 60
    with trading_engine(arrays, streams, borrow=False, trader=True, t_max_s=40) as eng:
        eng.run()
        assert_run_is_the_oracles(eng, streams, o)
        samples, first = eng.cluster_state_series(0, 1, n)
        assert_samples_equal(samples, trade_series_ref(arrays, streams, o, 0, 1, n))
        assert_matches_single_call(eng, samples, 0, 1, range(n))
        assert np.isnan(samples["cores_utilization"][0]).all() and (samples["running"][0] == 0).all()
        assert samples["queued"][0].tolist() == [1] * 3 + [2] * (n - 3)
