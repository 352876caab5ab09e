"""GPU parity of the average wait time series (csrc/mcs_wait.hip, mcs_wait_time_series).

Every test takes the placements from the engine, asserts them equal to the oracle's, and compares the
samples bit for bit (the double as uint64) with tests/wait_ref.py's replay of the Go loop over those
start seconds.  Before that it asserts on the CPU that its inputs tell the two wrong restatements of
wait_ref (no h_j gate; no D6 skip) from the right one.

The engine refuses max_wait_s = 0 under DELAY (mcs_engine_create), so the smallest MaxWaitTime a GPU
run can have is 1; W = 0 is covered on the CPU (tests/test_wait_ref.py)."""
import ctypes as C

import numpy as np
import pytest

import oracle_ref as O
import wait_ref as R
from kat_util import fuzz_workload, seeded_workload
from mcs_amd import WAIT_SAMPLE_DTYPE, Cluster, ClusterArrays, Engine, GenParams, JobStreams, MCSError, Node, \
    pack_clusters, replicate, uniform_cluster, wire
from mcs_amd import _lib as L
from mcs_amd.engine import scaled_lambda

pytestmark = pytest.mark.gpu

T_MAX = 0xFFFFFFFE


def hot_clusters(sizes, seed, nodes=None):
    """Small hot clusters: 2-6 nodes of 8 cores / 32 memory, gaps from {0, 0, 1, 1, 1, 2}, durations
    0-40, requests up to a node (every job fits an empty node: no deadlock)."""
    rng = np.random.default_rng(seed)
    clusters, parts = [], []
    for k, J in enumerate(sizes):
        nn = int(rng.integers(2, 7)) if nodes is None else nodes[k]
        clusters.append(Cluster(Id=k + 1, Nodes=[Node(Id=i + 1, Cores=8, Memory=32, CoresAvailable=8,
                                                      MemoryAvailable=32) for i in range(nn)]))
        parts.append((np.cumsum(rng.choice([0, 0, 1, 1, 1, 2], J)), rng.integers(0, 41, J), rng.integers(0, 9, J),
                      rng.integers(0, 33, J)))
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    return pack_clusters(clusters), JobStreams(*(np.concatenate([p[f] for p in parts]).astype(np.uint32)
                                                 for f in range(4)), off)


def concat(parts):
    """Single-cluster (arrays, streams) pairs as one system."""
    assert all(a.n_clusters == 1 for a, _ in parts)
    arrays = ClusterArrays(*(np.concatenate([getattr(a, f) for a, _ in parts]) for f in
                             ("cap_c", "cap_m", "free_c", "free_m")),
                           np.concatenate([[0], np.cumsum([int(a.node_off[-1]) for a, _ in parts])]).astype(np.uint32))
    off = np.concatenate([[0], np.cumsum([s.n_jobs for _, s in parts])]).astype(np.uint64)
    return arrays, JobStreams(*(np.concatenate([getattr(s, f) for _, s in parts]) for f in
                                ("arrival", "dur", "cores", "mem")), off)


class Run:
    """A DELAY run on the engine whose placements equal the oracle's, with the replay of every cluster."""

    def __init__(self, eng, arrays, streams, W, stats=None):
        self.eng, self.arrays, self.streams, self.W, self.stats = eng, arrays, streams, W, stats
        self.node, self.start, self.fin, self.ostats = O.delay_run_batch(arrays, streams, n_threads=8, max_wait_s=W)
        gn, gs, gf = eng.placements()
        np.testing.assert_array_equal(gn, self.node)
        np.testing.assert_array_equal(gs, self.start)
        np.testing.assert_array_equal(gf, self.fin)
        self.t_end = self.ostats["t_end"].astype(np.int64)
        self._replays = {}

    def of(self, c):
        js = self.streams.of(c)
        return self.streams.arrival[js], self.start[js]

    def replay(self, c, T, fn=R.replay):
        key = (c, T, fn)
        if key not in self._replays:
            self._replays[key] = fn(*self.of(c), self.W, T)
        return self._replays[key]

    def want(self, t0, period, n, T=None):
        """The samples from the replay; seconds past T (default: the last sample) from the loop's
        fixed point, which the replay must have reached by T."""
        last = t0 + (n - 1) * period
        T = last if T is None else T
        out = np.zeros((self.arrays.n_clusters, n), WAIT_SAMPLE_DTYPE)
        for c in range(self.arrays.n_clusters):
            rep = self.replay(c, T)
            tail = None
            if last > T:
                assert R.steady_after(rep, *self.of(c), T)
                tail = (T, len(rep["level1"]))
            out["total_wait_ms"][c], out["jobs_count"][c] = R.samples(rep, t0, period, n, tail)
        out["average_wait_time"] = R.average(out["total_wait_ms"], out["jobs_count"])
        return out

    def assert_wrong_restatements_differ(self, T, clusters=None):
        gate = skip = False
        for c in range(self.arrays.n_clusters) if clusters is None else clusters:
            right = self.replay(c, T)["total_ms"]
            gate |= bool((self.replay(c, T, R.replay_no_gate)["total_ms"] != right).any())
            skip |= bool((self.replay(c, T, R.replay_no_skip)["total_ms"] != right).any())
        assert gate, "no sample tells the restatement without the h_j gate from the replay"
        assert skip, "no sample tells the restatement without the D6 skip from the replay"


def assert_bits_equal(got, want, tag=""):
    assert got.shape == want.shape and got.dtype == WAIT_SAMPLE_DTYPE
    for f in ("jobs_count", "total_wait_ms", "average_wait_time"):
        bad = np.argwhere(got[f].view(np.uint64) != want[f].view(np.uint64))
        assert bad.size == 0, f"{tag} {f}: {len(bad)} samples differ, first (cluster, k) {bad[:4].tolist()}: " \
                              f"got {got[f][tuple(bad[0])]!r} want {want[f][tuple(bad[0])]!r}"


def delay_engine(arrays, streams, W=10):
    eng = Engine(0, policy="DELAY", max_wait_s=W)
    eng.load_clusters(arrays)
    eng.submit_jobs(streams)
    return eng, eng.run()


@pytest.fixture(scope="module", params=[10, 1], ids=["W10", "W1"])
def hot(request):
    arrays, streams = hot_clusters([300] * 12, 0x484F54)
    eng, st = delay_engine(arrays, streams, request.param)
    with eng:
        yield Run(eng, arrays, streams, request.param, st)


def test_hot_small_clusters_every_second(hot):
    T = int(hot.t_end.max()) + 6
    assert T > int(hot.start[hot.node >= 0].max())
    hot.assert_wrong_restatements_differ(T)
    reps = [hot.replay(c, T) for c in range(12)]
    assert max(r["longest_skip_run"] for r in reps) >= 2
    assert sum(len(r["skips"]) for r in reps) > 12 * 50
    got = hot.eng.wait_time_series(0, 1, T + 1)
    assert_bits_equal(got, hot.want(0, 1, T + 1))
    ds = hot.eng.delay_stats()
    for c in range(12):  # the sample at the cluster's own t_end is the run's final statistics
        k = int(hot.t_end[c])
        assert got["total_wait_ms"][c, k] == ds["total_wait_ms"][c] and got["jobs_count"][c, k] == ds["jobs_count"][c]
        assert (got[c, k:] == got[c, k]).all()  # a drained cluster keeps them
    assert (ds["moved_l1"] > 0).all() and (ds["placed_l1"] > 0).all()


# ---- scan and cursor boundaries: clusters of 257, 1025 and 1300 jobs at odd offsets -----------------

@pytest.fixture(scope="module")
def rounds():
    arrays, streams = hot_clusters([300, 257, 1025, 1300], 0x524E4453, nodes=[3, 2, 4, 5])
    assert [int(o) % 256 for o in streams.job_off[1:4]] == [44, 45, 46]
    eng, st = delay_engine(arrays, streams)
    with eng:
        yield Run(eng, arrays, streams, 10, st)


@pytest.mark.parametrize("t0,period", [(0, 1), (3, 7)])
def test_rounds_of_256_jobs_and_samples(rounds, t0, period, monkeypatch):
    T = int(rounds.t_end.max()) + 9
    rounds.assert_wrong_restatements_differ(T)
    n = (T - t0) // period + 1
    if period == 1:
        assert n > 4 * 256 and n % 256 != 0  # several rounds of samples, the last one partial
    got = rounds.eng.wait_time_series(t0, period, n)
    assert_bits_equal(got, rounds.want(t0, period, n, T))
    # in chunks of 41 (inside a round) or 300 (across rounds) samples per launch: the same series
    monkeypatch.setenv("MCS_SERIES_CHUNK", "41" if period == 7 else "300")
    parts = rounds.eng.wait_time_series(t0, period, n)
    assert parts.tobytes() == got.tobytes()
    monkeypatch.delenv("MCS_SERIES_CHUNK")
    # the first clusters only: those rows, and nothing written behind them
    out = np.zeros((4, n), WAIT_SAMPLE_DTYPE)
    out.view(np.uint8)[...] = 0xA5
    rc = L.lib().mcs_wait_time_series(rounds.eng._h, t0, period, n, out.ctypes.data_as(C.POINTER(L.mcs_wait_sample)),
                                      3, None)
    assert rc == L.MCS_OK
    assert out[:3].tobytes() == got[:3].tobytes() and (out[3:].view(np.uint8) == 0xA5).all()


# ---- a 256-node cluster whose head reaches MaxWaitTime: delay_asm_kernel hands over to delay_kernel --

def level1_pressure(n_clusters=2, J=1500, blocked=660):
    """256 nodes of 2 cores / 4000 memory, every fourth one available, more than two arrivals per
    second: small jobs wait MaxWaitTime and are placed from Level1, and `blocked` requests of 3 cores
    fit no node, so Level1 outgrows the 640 entries the hand-scheduled loop keeps in LDS and the
    cluster is handed to delay_kernel (the stream of test_gpu_delay's capacity test, shorter and
    hotter).  seeded_workload("n256_hot", 2, 1500) does not serve here: the oracle moves none of its
    jobs to Level1, and the loop hands over only once Level1 is past its LDS slice."""
    rng = np.random.default_rng(0x4C31)
    cl = Cluster(Id=1, Nodes=[Node(Id=i + 1, Cores=2, Memory=4000, CoresAvailable=0 if i % 4 else 2,
                                   MemoryAvailable=0 if i % 4 else 4000) for i in range(256)])
    parts = []
    for _ in range(n_clusters):
        cores = rng.integers(0, 3, J)
        cores[rng.choice(J, blocked, replace=False)] = 3
        parts.append((np.cumsum(rng.poisson(0.4, J)), rng.integers(0, 400, J), cores, rng.integers(0, 4001, J)))
    off = np.arange(n_clusters + 1, dtype=np.uint64) * J
    return replicate(cl, n_clusters), JobStreams(*(np.concatenate([p[f] for p in parts]).astype(np.uint32)
                                                   for f in range(4)), off)


def test_256_nodes_handed_over_to_the_level1_kernel():
    arrays, streams = level1_pressure()
    eng, st = delay_engine(arrays, streams)
    with eng:
        run = Run(eng, arrays, streams, 10, st)
        assert st.handed_over > 0
        ds = eng.delay_stats()
        assert (ds["moved_l1"] > 660).all() and (ds["placed_l1"] > 100).all() and (ds["peak_l1"] > 640).all()
        T = int(run.t_end.max()) + 5
        run.assert_wrong_restatements_differ(T)
        n = T // 3 + 1
        assert_bits_equal(eng.wait_time_series(0, 1, T + 1), run.want(0, 1, T + 1))
        assert_bits_equal(eng.wait_time_series(2, 3, n - 1), run.want(2, 3, n - 1, T))


# ---- a deadlocked cluster and a cluster with no jobs -----------------------------------------------

def test_deadlocked_and_empty_clusters():
    fa, fs = fuzz_workload("w16s", 7, n_clusters=5, J=400, blocking=True)
    parts = []
    for c in range(5):
        ns, js = fa.nodes_of(c), fs.of(c)
        parts.append((ClusterArrays(fa.cap_c[ns], fa.cap_m[ns], fa.free_c[ns], fa.free_m[ns],
                                    np.array([0, ns.stop - ns.start], np.uint32)),
                      JobStreams(fs.arrival[js], fs.dur[js], fs.cores[js], fs.mem[js], np.array([0, 400], np.uint64))))
    nothing = JobStreams(*(np.zeros(0, np.uint32) for _ in range(4)), np.zeros(2, np.uint64))
    parts.insert(2, (replicate(uniform_cluster(7), 1), nothing))
    arrays, streams = concat(parts)
    EMPTY = 2
    assert streams.job_off.tolist() == [0, 400, 800, 800, 1200, 1600, 2000]
    eng, st = delay_engine(arrays, streams)
    with eng:
        run = Run(eng, arrays, streams, 10, st)
        dead = np.nonzero(run.ostats["flags"] & 1)[0]
        assert 0 < dead.size < 5 and st.deadlocked == dead.size
        T = int(run.t_end.max()) + 12
        run.assert_wrong_restatements_differ(T)
        got = eng.wait_time_series(0, 1, T + 1)
        assert_bits_equal(got, run.want(0, 1, T + 1))
        ds, cs = eng.delay_stats(), eng.cluster_stats()
        assert (cs["t_end"] == run.t_end).all()
        for c in range(6):
            k = int(run.t_end[c])
            assert got["total_wait_ms"][c, k] == ds["total_wait_ms"][c] and got["jobs_count"][c, k] == ds["jobs_count"][c]
            growth = np.diff(got["total_wait_ms"][c, k:])
            if c in dead:  # every Level1 job left is examined each second
                assert ds["l1_left"][c] > 0 and (growth == 1000 * int(ds["l1_left"][c])).all()
            else:
                assert (growth == 0).all()
        assert (got[EMPTY].view(np.uint64) == 0).all()  # 0, 0, 0.0
        # the top of the clock: the Go loop continued to 0xFFFFFFFE, and a period of 2^31
        for t0, period, n in ((T_MAX - 3 * 7, 7, 4), (5, 0x80000000, 2), (T_MAX, 1, 1)):
            late = eng.wait_time_series(t0, period, n)
            assert_bits_equal(late, run.want(t0, period, n, T), f"t0 {t0:#x}")
            assert (late["total_wait_ms"][dead, -1] > 1 << 32).all()
            assert (late[EMPTY].view(np.uint64) == 0).all()


# ---- a fused DELAY run ------------------------------------------------------------------------------

def test_fused_run_equals_the_materialised_stream():
    arrays = replicate(uniform_cluster(8), 5)
    got = []
    for fused in (False, True):
        gp = GenParams(seed=0xF05ED, arrival_mode=1, max_dur_s=60, lam=scaled_lambda(8, max_dur_s=60, load=1.15),
                       fused=fused)
        with Engine(0, policy="DELAY") as eng:
            eng.load_clusters(arrays)
            eng.generate_jobs(gp, 500)
            st = eng.run()
            if not fused:
                run = Run(eng, arrays, eng.read_jobs(), 10, st)
                T = int(run.t_end.max()) + 3
                n = T // 5 + 3
            got.append(eng.wait_time_series(0, 5, n))
    assert got[0].tobytes() == got[1].tobytes()
    run.assert_wrong_restatements_differ(T)
    assert_bits_equal(got[1], run.want(0, 5, n, T))
    assert got[1]["total_wait_ms"][:, -1].min() > 0


# ---- the reference cadence: the Start stream with its last field ------------------------------------

def test_start_stream_at_the_reference_cadence(hot):
    T = int(hot.t_end.max()) + 6
    hot.assert_wrong_restatements_differ(T)
    n = T // 5 + 2
    waits = hot.eng.wait_time_series(0, 5, n)
    assert_bits_equal(waits, hot.want(0, 5, n, T))
    samples, first = hot.eng.cluster_state_series(0, 5, n)
    ds = hot.eng.delay_stats()
    for c in range(hot.arrays.n_clusters):
        msgs = wire.start_stream(samples[c], first[c], waits["average_wait_time"][c])
        assert len(msgs) == n
        back = [wire.unmarshal(wire.ClusterState, wire.marshal(m)).average_wait_time for m in msgs]
        assert np.array(back).view(np.uint64).tolist() == waits["average_wait_time"][c].view(np.uint64).tolist()
        assert msgs[-1].average_wait_time == int(ds["total_wait_ms"][c]) / int(ds["jobs_count"][c])
        assert msgs[-1].average_wait_time > 0


# ---- refusals ---------------------------------------------------------------------------------------

def test_invalid_arguments(hot):
    eng, n = hot.eng, hot.arrays.n_clusters
    out = np.zeros((n + 1, 4), WAIT_SAMPLE_DTYPE)
    po = out.ctypes.data_as(C.POINTER(L.mcs_wait_sample))
    f = L.lib().mcs_wait_time_series
    assert f(eng._h, 0, 5, 4, po, n, None) == L.MCS_OK
    assert f(eng._h, 0, 0, 4, po, n, None) == L.MCS_E_INVALID           # period_s == 0
    assert f(eng._h, 0, 5, 0, po, n, None) == L.MCS_E_INVALID           # n_samples == 0
    assert f(eng._h, 0, 5, 4, None, n, None) == L.MCS_E_INVALID         # out == NULL
    assert f(eng._h, 0, 5, 4, po, n + 1, None) == L.MCS_E_INVALID       # more clusters than the engine has
    assert f(eng._h, 0xFFFFFFFC, 1, 4, po, n, None) == L.MCS_E_INVALID  # last sample 0xFFFFFFFF
    assert f(eng._h, 0xFFFFFFFB, 1, 4, po, n, None) == L.MCS_OK         # last sample 0xFFFFFFFE
    assert f(eng._h, 3, 0x80000000, 3, po, n, None) == L.MCS_E_INVALID  # 3 + 2 * 2^31 wraps in 32 bits
    assert f(eng._h, 0, 5, 4, po, 0, None) == L.MCS_OK                  # no cluster asked for
    ms = C.c_double(-1.0)
    assert f(eng._h, 0, 5, 4, po, n, C.byref(ms)) == L.MCS_OK and ms.value > 0.0
    with pytest.raises(MCSError) as ei:
        eng.wait_time_series(0, 0, 4)
    assert ei.value.code == L.MCS_E_INVALID
    samples, ms = eng.wait_time_series(0, 5, 4, with_time=True)
    assert samples.tobytes() == out[:n].tobytes() and ms > 0.0


def test_refused_without_a_plain_delay_batch_run():
    arrays, streams, _ = seeded_workload("small", 3, 200)

    def refused(eng):
        with pytest.raises(MCSError) as ei:
            eng.wait_time_series(0, 5, 10)
        return ei.value.code == L.MCS_E_STATE

    with Engine(0, policy="DELAY") as eng:  # before run()
        eng.load_clusters(arrays)
        eng.submit_jobs(streams)
        assert refused(eng)
        eng.run()
        assert eng.wait_time_series(0, 5, 10).shape == (3, 10)
    with Engine(0, policy="DELAY", trader=True) as eng:  # after a trading run
        eng.load_clusters(arrays)
        eng.submit_jobs(streams)
        eng.run()
        assert refused(eng)
    with Engine(0, policy="DELAY") as eng:  # after append_jobs
        eng.load_clusters(arrays)
        eng.append_jobs(streams)
        eng.run()
        assert refused(eng)
    with Engine(0, policy="FIFO") as eng:  # after a FIFO run: "/delay" never fed WaitTime
        eng.load_clusters(arrays)
        eng.submit_jobs(streams)
        eng.run()
        assert refused(eng)
    with pytest.raises(MCSError) as ei:  # MaxWaitTime 0 is no DELAY configuration of the engine
        Engine(0, policy="DELAY", max_wait_s=0)
    assert ei.value.code == L.MCS_E_INVALID
