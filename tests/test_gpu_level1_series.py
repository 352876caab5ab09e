"""GPU parity of the Level1 series (csrc/mcs_level1.hip: mcs_level1_series, mcs_online_level1_series,
mcs_read_level1): what ProvideJobs hands the trader after the Delay iteration at every sample second.

Every batch test takes the placements from the engine, asserts them equal to the oracle's, and
compares the samples bit for bit with tests/level1_ref.py's per-second replay of the Go loop over
those start seconds, sized by the literal contract recurrences.  tests/test_level1_ref.py pins that
reference, and the coverage conditions of the seeds used here, on the CPU.  The online tests compare
a session's samples with a batch engine's over the whole stream.  Run on a real MI355X:
``pytest -m gpu``."""
import ctypes as C

import numpy as np
import pytest

import level1_cases as K
import level1_ref as R
import oracle_ref as O
from kat_util import seeded_workload
from mcs_amd import LEVEL1_SAMPLE_DTYPE, Engine, GenParams, JobStreams, MCSError, replicate, uniform_cluster
from mcs_amd import _lib as L
from mcs_amd.engine import scaled_lambda
from test_gpu_online import horizons_for, slice_streams
from test_level1_ref import contracts_equal_samples, trading_system

pytestmark = pytest.mark.gpu

TIME_NONE = 0xFFFFFFFF
EVER = 1 << 32


def delay_engine(arrays, streams, W=10):
    eng = Engine(0, policy="DELAY", max_wait_s=W)
    eng.load_clusters(arrays)
    eng.submit_jobs(streams)
    return eng, eng.run()


class Run(K.Ref):
    """A DELAY run on the engine whose placements equal the oracle's, with the replay of every cluster."""

    def __init__(self, eng, arrays, streams, W):
        node, start, fin, self.ostats = O.delay_run_batch(arrays, streams, n_threads=8, max_wait_s=W)
        for got, want in zip(eng.placements(), (node, start, fin)):
            np.testing.assert_array_equal(got, want)
        super().__init__(streams, np.where(node >= 0, start, TIME_NONE), W)
        self.eng, self.arrays, self.node = eng, arrays, node
        self.t_end = self.ostats["t_end"].astype(np.int64)


# ---- 1. hot 5-node clusters, every second -----------------------------------------------------------

@pytest.fixture(scope="module", params=[10, 1], ids=["W10", "W1"])
def hot(request):
    arrays, streams = K.hot_five_nodes()
    eng, _ = delay_engine(arrays, streams, request.param)
    with eng:
        yield Run(eng, arrays, streams, request.param)


def test_hot_small_clusters_every_second(hot):
    T = int(hot.t_end.max()) + 6
    want = hot.want(0, 1, T + 1)
    K.assert_coverage(want)
    got = hot.eng.level1_series(0, 1, T + 1)
    K.assert_samples_equal(got, want)
    ds = hot.eng.delay_stats()
    for c in range(hot.C):
        assert got["len"][c].max() == ds["peak_l1"][c] and got["len"][c, int(hot.t_end[c])] == ds["l1_left"][c] == 0
        assert (got["len"][c, int(hot.t_end[c]):] == 0).all()  # a drained cluster reads as empty
    assert (got["head"][got["len"] == 0] == TIME_NONE).all()
    samples, ms = hot.eng.level1_series(0, 5, 40, with_time=True)
    assert samples.tobytes() == np.ascontiguousarray(got[:, 0:200:5]).tobytes() and ms > 0.0


# ---- 2. streams of 255, 256, 257 and 513 jobs: batches, tiles and chunks --------------------------------

@pytest.fixture(scope="module")
def rounds():
    arrays, streams = K.rounds_system()
    assert np.diff(streams.job_off).tolist() == [255, 256, 257, 513]
    eng, _ = delay_engine(arrays, streams)
    with eng:
        yield Run(eng, arrays, streams, 10)


@pytest.mark.parametrize("t0,period", [(0, 1), (3, 7)])
@pytest.mark.parametrize("n", [255, 256, 257])
def test_rounds_of_256_jobs_and_samples(rounds, t0, period, n, monkeypatch):
    T = int(rounds.t_end.max()) + 9
    want = rounds.want(t0, period, n, T)
    if period == 7:
        # a Level1 window across a 256-job batch boundary, at a sampled second (the head moves on by at
        # most one row per second, so row 256 enters Level1 after second 256: past the (0, 1) grid)
        assert all(any(m and m[0] // 256 != m[-1] // 256
                       for t in range(t0, min(t0 + n * period, T + 1), period) for m in [rounds.members(c, t, T)])
                   for c in (2, 3))
    assert (want["len"].max(axis=1) > 20).all()
    got = rounds.eng.level1_series(t0, period, n)
    K.assert_samples_equal(got, want)
    # in chunks of 41 (inside a tile row) or 100 samples per launch: the same series
    monkeypatch.setenv("MCS_SERIES_CHUNK", "41" if period == 7 else "100")
    parts = rounds.eng.level1_series(t0, period, n)
    monkeypatch.delenv("MCS_SERIES_CHUNK")
    assert parts.tobytes() == got.tobytes()
    # the first clusters only: those rows, and nothing written behind them
    out = np.zeros((4, n), LEVEL1_SAMPLE_DTYPE)
    out.view(np.uint8)[...] = 0xA5
    rc = L.lib().mcs_level1_series(rounds.eng._h, t0, period, n, out.ctypes.data_as(C.POINTER(L.mcs_level1_sample)),
                                   3, None)
    assert rc == L.MCS_OK
    assert out[:3].tobytes() == got[:3].tobytes() and (out[3:].view(np.uint8) == 0xA5).all()


# ---- 3. a deadlocked cluster, a cluster without jobs, a cluster in which nothing moves ----------------

def test_deadlocked_empty_and_calm_clusters():
    arrays, streams = K.deadlock_system()
    eng, st = delay_engine(arrays, streams)
    with eng:
        run = Run(eng, arrays, streams, 10)
        assert st.deadlocked == 1 and run.ostats["l1_left"].tolist() == [14, 0, 0]
        assert run.ostats["moved_l1"][K.CALM] == 0
        T = int(run.t_end.max()) + 12
        got = eng.level1_series(0, 1, T + 1)
        K.assert_samples_equal(got, run.want(0, 1, T + 1))
        assert (got[K.EMPTY]["len"] == 0).all() and (got[K.CALM]["len"] == 0).all()
        wrapped = (14 << 30) & 0xFFFFFFFF
        assert wrapped == 1 << 31 and 14 << 30 > 1 << 32
        assert got["len"][K.DEAD, -1] == 14 and got["mem"][K.DEAD, -1] == wrapped and got["cores"][K.DEAD, -1] == 70
        # the top of the clock: the Go loop continued to 0xFFFFFFFE, and a period of 2^31
        for t0, period, n in ((K.T_MAX - 3 * 7, 7, 4), (5, 0x80000000, 2), (K.T_MAX, 1, 1)):
            late = eng.level1_series(t0, period, n)
            K.assert_samples_equal(late, run.want(t0, period, n, T), f"t0 {t0:#x}")
            assert late["len"][K.DEAD, -1] == 14 and late["mem"][K.DEAD, -1] == wrapped
            assert (late[K.EMPTY]["len"] == 0).all() and (late[K.CALM]["len"] == 0).all()


# ---- 4. a 256-node cluster whose head reaches MaxWaitTime: handed over to delay_kernel ----------------

def test_256_nodes_handed_over_to_the_level1_kernel():
    arrays, streams = K.level1_pressure()
    eng, st = delay_engine(arrays, streams)
    with eng:
        run = Run(eng, arrays, streams, 10)
        assert st.handed_over > 0
        ds = eng.delay_stats()
        assert (ds["moved_l1"] > 660).all() and (ds["peak_l1"] > 640).all()
        T = int(run.t_end.max()) + 5
        n = T // 3
        got = eng.level1_series(2, 3, n)
        K.assert_samples_equal(got, run.want(2, 3, n, T))
        assert (got["len"].max(axis=1) > 640).all() and (got["len"][:, -1] == ds["l1_left"]).all()
        mult = (got["len"] > 0) & (got["len"] % 20 == 0)
        assert mult.any()


# ---- 5. a fused DELAY run ---------------------------------------------------------------------------

def test_fused_run_equals_the_materialised_stream():
    arrays = replicate(uniform_cluster(8), 5)
    got = []
    for fused in (False, True):
        gp = GenParams(seed=0xF05ED, arrival_mode=1, max_dur_s=60, lam=scaled_lambda(8, max_dur_s=60, load=1.15),
                       fused=fused)
        with Engine(0, policy="DELAY") as eng:
            eng.load_clusters(arrays)
            eng.generate_jobs(gp, 500)
            eng.run()
            if not fused:
                run = Run(eng, arrays, eng.read_jobs(), 10)
                T = int(run.t_end.max()) + 3
                n = T // 5 + 3
            got.append(eng.level1_series(0, 5, n))
    assert got[0].tobytes() == got[1].tobytes()
    K.assert_samples_equal(got[1], run.want(0, 5, n, T))
    assert got[1]["len"].max() > 0


# ---- 6. ProvideJobs at one second -------------------------------------------------------------------

def test_level1_at_equals_the_reference_list(hot):
    T = int(hot.t_end.max()) + 6
    lens = {}  # length -> (cluster, second)
    for c in range(hot.C):
        for t, m in enumerate(hot.replay(c, T)["lists"]):
            lens.setdefault(len(m), (c, t))
    big = max(lens)
    assert big > 64 and {0, 1, 20} <= set(lens)
    for ln in (0, 1, 20, big):
        c, t = lens[ln]
        want = list(hot.members(c, t, T))
        rows, n = hot.eng.level1_at(c, t)
        assert n == ln and rows.tolist() == want, (ln, c, t)
        for cap in {0, 1, ln // 2, max(ln - 1, 0)}:  # cap below len: *n is the length, cap rows written
            buf = np.full(ln + 2, 0xA5A5A5A5, np.uint32)
            cnt = C.c_uint32(77)
            rc = L.lib().mcs_read_level1(hot.eng._h, c, t, L.ptr(buf, C.c_uint32), cap, C.byref(cnt))
            assert rc == L.MCS_OK and cnt.value == ln
            k = min(cap, ln)
            assert buf[:k].tolist() == want[:k] and (buf[k:] == 0xA5A5A5A5).all(), (ln, cap)
    # the last cluster, at the top of the clock: drained
    rows, n = hot.eng.level1_at(hot.C - 1, K.T_MAX)
    assert n == 0 and rows.size == 0


# ---- 7. a DELAY trading run: every logged contract is the sample at its second -------------------------

@pytest.mark.parametrize("resident,form", [("1", 5), ("0", 0)])
def test_contracts_of_a_trading_run_equal_the_samples(resident, form, monkeypatch):
    monkeypatch.setenv("MCS_DT_RESIDENT", resident)
    arrays, streams = trading_system()
    with Engine(0, policy="DELAY", trader=True) as eng:
        eng.load_clusters(arrays)
        eng.submit_jobs(streams)
        eng.run()
        assert eng.trade_stats()["loop_form"] == form
        trades = eng.contracts()
        assert len(trades) > 0
        T = int(trades["t"].max())
        got = eng.level1_series(0, 1, T + 1)
        seen = contracts_equal_samples(trades, lambda c, t: got[c, t])
        assert seen[0] + seen[1] > 0, seen
        node, start, _ = eng.placements()
        ref = K.Ref(streams, np.where(node >= 0, start, TIME_NONE), 10)
        K.assert_samples_equal(got, ref.want(0, 1, T + 1))
        c, t = int(trades["requester"][0]), int(trades["t"][0])
        rows, n = eng.level1_at(c, t)
        assert rows.tolist() == list(ref.members(c, t, T)) and n == got["len"][c, t]


# ---- 8. online sessions -----------------------------------------------------------------------------

class Batch:
    """The whole stream run as a batch on an engine of its own: every second of [0, T)."""

    def __init__(self, arrays, streams, extra=40):
        eng, _ = delay_engine(arrays, streams)
        with eng:
            self.placements = eng.placements()
            self.T = int(eng.cluster_stats()["t_end"].max()) + extra
            self.level1 = eng.level1_series(0, 1, self.T)

    def check(self, eng, t0, period, n, tag=""):
        got = eng.online_level1_series(t0, period, n)
        K.assert_samples_equal(got, self.level1[:, t0 + period * np.arange(n)], f"{tag} t0 {t0} period {period}")
        return got


def refused(call, code):
    with pytest.raises(MCSError) as ei:
        call()
    assert ei.value.code == code, ei.value
    return str(ei.value)


def test_online_slices_equal_the_batch_series():
    """Five hot clusters in random slices, the jobs appended between them: cluster 2 has no jobs, and
    every job of cluster 3 arrives behind the first horizon, so all of them are appended."""
    arrays, streams = K.hot_clusters([300, 257, 0, 200, 300], 0x4F4E4C31, nodes=[5] * 5)
    rng = np.random.default_rng(0x534C4943)
    top = int(streams.arrival.max()) + 1
    hs = sorted({int(x) for x in rng.integers(5, top, 6)})
    streams.arrival[streams.of(3)] += np.uint32(hs[0] + 2)
    ref = Batch(arrays, streams)
    assert ref.level1["len"].max(axis=1).tolist()[2] == 0 and (ref.level1["len"].max(axis=1)[[0, 1, 3, 4]] > 20).all()
    members = undecided = 0
    with Engine(0, policy="DELAY", max_wait_s=10) as eng:
        eng.load_clusters(arrays)
        eng.submit_jobs(slice_streams(streams, 0, hs[0]))
        prev = 0
        for h in hs:
            if prev:
                eng.append_jobs(slice_streams(streams, prev, h))
            st = eng.run(h)
            assert st.online and st.t_horizon == h
            members += int(ref.check(eng, prev, 1, h - prev, f"h {h}")["len"].sum())
            ref.check(eng, 0, 5, (h + 4) // 5, f"h {h}")
            node, start, _ = eng.placements()
            undecided += int(((node == L.MCS_NODE_UNPLACED) & (start == L.MCS_TIME_NONE)).sum())
            assert str(h) in refused(lambda: eng.online_level1_series(prev, 1, h - prev + 1), L.MCS_E_INVALID)
            refused(lambda: eng.online_level1_series(h, 1, 1), L.MCS_E_INVALID)
            msg = refused(lambda: eng.level1_series(0, 1, 1), L.MCS_E_STATE) if prev else ""
            assert not prev or "mcs_online_level1_series" in msg  # after append_jobs the batch call names it
            prev = h
        eng.append_jobs(slice_streams(streams, prev, EVER))
        refused(lambda: eng.online_level1_series(0, 1, prev + 1), L.MCS_E_INVALID)  # still the horizon's frontier
        eng.run()
        for got, want in zip(eng.placements(), ref.placements):
            np.testing.assert_array_equal(got, want)
        ref.check(eng, 0, 1, ref.T, "drained")  # past t_end: the continued Go loop
        ref.check(eng, 3, 7, (ref.T - 3) // 7, "drained")
        assert eng.online_level1_series(K.T_MAX, 1, 1)["len"].max() == 0
        assert "mcs_online_level1_series" in refused(lambda: eng.level1_at(0, 5), L.MCS_E_STATE)
    assert members > 0 and undecided > 0


def test_online_series_over_segments_with_slack():
    """A 700-job cluster behind a small one, fed by many small appends: its segment starts off a
    multiple of 256, holds several summary batches and moves at every relayout.  Each slice's series
    equals the batch run's and leaves the earlier samples unchanged."""
    arrays, streams = K.hot_clusters([100, 700, 300], 0x534547, nodes=[3, 4, 5])
    ref = Batch(arrays, streams)
    top = int(streams.arrival.max()) + 1
    hs = list(range(9, top, max(1, top // 12)))
    relayouts = odd_starts = 0
    with Engine(0, policy="DELAY", max_wait_s=10) as eng:
        eng.load_clusters(arrays)
        eng.submit_jobs(slice_streams(streams, 0, hs[0]))
        eng.run(hs[0])
        seg = eng.segment_offsets()
        before = ref.check(eng, 0, 1, hs[0])
        prev = hs[0]
        for h in hs[1:]:
            eng.append_jobs(slice_streams(streams, prev, h))
            now, counts = eng.segment_offsets(), np.diff(eng.job_offsets())
            relayouts += now.tolist() != seg.tolist()
            seg = now
            eng.run(h)
            after = ref.check(eng, 0, 1, h, f"h {h}")
            assert after[:, :prev].tobytes() == before.tobytes(), f"h {h}: samples below {prev} changed"
            odd_starts += int(counts[1] >= 257 and int(seg[1]) % 256 != 0)
            before, prev = after, h
        assert (np.diff(seg) > np.diff(eng.job_offsets())).any()  # slack: the segments are not dense
    assert relayouts >= 1 and odd_starts >= 1


@pytest.mark.parametrize("restart", ["rewind", "batch"])
def test_online_restarted_session_with_new_jobs_below_the_horizon(restart):
    """The scenario of tests/test_gpu_online_series.py: one node of two cores; A holds one core on
    [0, 62), B the other on [1, 31); E asks for both and waits in Level1 from second 15.  In the first
    pass E starts at 62.  The added job F (arrival 40, one core, 30 s) takes the core B left, so E
    starts at 70: at h = 64 E's row must read undecided (still in Level1 at 62 and 63), not the earlier
    pass's 62."""
    from mcs_amd import Cluster, Node, pack_clusters

    cl = Cluster(Id=1, Nodes=[Node(Id=1, Cores=2, Memory=8, CoresAvailable=2, MemoryAvailable=8)])
    arrays = pack_clusters([cl, cl])
    first = [(0, 62, 1, 1), (1, 30, 1, 1), (5, 30, 2, 1)]
    added = [(40, 30, 1, 1), (80, 4, 1, 1)]
    h, E = 64, 2

    def two(jobs):  # the same stream in both clusters
        cols = [np.array([j[f] for j in jobs] * 2, np.uint32) for f in range(4)]
        return JobStreams(*cols, np.array([0, len(jobs), 2 * len(jobs)], np.uint64))

    ref = Batch(arrays, two(first + added))
    assert ref.placements[1][E] == 70
    assert ref.level1["len"][0, 14:71].tolist() == [0] + [1] * 55 + [0] and ref.level1["head"][0, 63] == E
    with Engine(0, policy="DELAY", max_wait_s=10) as eng:
        eng.load_clusters(arrays)
        eng.submit_jobs(two(first))
        eng.run()
        assert eng.placements()[1][E] == 62
        assert eng.level1_series(60, 1, 4)["len"][0].tolist() == [1, 1, 0, 0]  # the earlier pass, as a batch run
        if restart == "rewind":
            eng.run(3)  # (a session, so that rewind has one to restart)
            eng.run()
            eng.rewind()
            refused(lambda: eng.online_level1_series(0, 1, 1), L.MCS_E_STATE)  # until the next run
        eng.append_jobs(two(added))
        eng.run(h)
        ref.check(eng, 0, 1, h, restart)
        eng.run()
        ref.check(eng, 0, 1, ref.T, restart + " drained")


# ---- 9. refusals and invalid arguments ----------------------------------------------------------------

def test_invalid_arguments(hot):
    eng, n = hot.eng, hot.C
    out = np.zeros((n + 1, 4), LEVEL1_SAMPLE_DTYPE)
    po = out.ctypes.data_as(C.POINTER(L.mcs_level1_sample))
    f = L.lib().mcs_level1_series
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
    assert refused(lambda: eng.level1_series(0, 0, 4), L.MCS_E_INVALID)
    g = L.lib().mcs_read_level1
    rows, cnt = np.zeros(8, np.uint32), C.c_uint32()
    pr = L.ptr(rows, C.c_uint32)
    assert g(eng._h, 0, 50, pr, 8, C.byref(cnt)) == L.MCS_OK
    assert g(eng._h, n, 50, pr, 8, C.byref(cnt)) == L.MCS_E_INVALID           # cluster out of range
    assert g(eng._h, 0, 50, pr, 8, None) == L.MCS_E_INVALID                   # n == NULL
    assert g(eng._h, 0, 50, None, 8, C.byref(cnt)) == L.MCS_E_INVALID         # no room for cap rows
    assert g(eng._h, 0, 0xFFFFFFFF, pr, 8, C.byref(cnt)) == L.MCS_E_INVALID   # past the last second
    assert g(eng._h, 0, 50, None, 0, C.byref(cnt)) == L.MCS_OK                # the length alone


def test_refusals():
    arrays, streams, _ = seeded_workload("small", 3, 200)
    h = int(np.median(streams.arrival))

    def both(eng, code, word=""):
        for call in (lambda: eng.level1_series(0, 5, 10), lambda: eng.level1_at(0, 5)):
            assert word in refused(call, code)

    with Engine(0, policy="DELAY") as eng:  # before run(); a batch run is no session
        eng.load_clusters(arrays)
        eng.submit_jobs(streams)
        both(eng, L.MCS_E_STATE)
        refused(lambda: eng.online_level1_series(0, 5, 2), L.MCS_E_STATE)
        eng.run()
        assert eng.level1_series(0, 5, 10).shape == (3, 10)
        assert "mcs_level1_series" in refused(lambda: eng.online_level1_series(0, 5, 2), L.MCS_E_STATE)
        eng.run(h)  # a session without an append: the batch calls keep answering, as the wait series does
        assert eng.online_level1_series(0, 1, h).tobytes() == eng.level1_series(0, 1, h).tobytes()
        f = L.lib().mcs_online_level1_series
        out = np.zeros((4, 4), LEVEL1_SAMPLE_DTYPE)
        po = out.ctypes.data_as(C.POINTER(L.mcs_level1_sample))
        assert f(eng._h, 0, 1, 4, po, 3, None) == L.MCS_OK
        assert f(eng._h, 0, 0, 4, po, 3, None) == L.MCS_E_INVALID
        assert f(eng._h, 0, 1, 0, po, 3, None) == L.MCS_E_INVALID
        assert f(eng._h, 0, 1, 4, None, 3, None) == L.MCS_E_INVALID
        assert f(eng._h, 0, 1, 4, po, 4, None) == L.MCS_E_INVALID
        eng.run()  # a drain: every second up to 0xFFFFFFFE
        assert eng.online_level1_series(0xFFFFFFFB, 1, 4).shape == (3, 4)
        refused(lambda: eng.online_level1_series(0xFFFFFFFC, 1, 4), L.MCS_E_INVALID)
        late = JobStreams(*(np.full(3, v, np.uint32) for v in (1 << 20, 5, 1, 1)), np.arange(4, dtype=np.uint64))
        eng.append_jobs(late)
        refused(lambda: eng.online_level1_series(0, 5, 4), L.MCS_E_STATE)  # jobs appended behind a drain
        both(eng, L.MCS_E_STATE, "mcs_online_level1_series")               # after append_jobs: names the online call
    with Engine(0, policy="DELAY", trader=True) as eng:  # a DELAY trading run on one engine is accepted
        eng.load_clusters(arrays)
        eng.submit_jobs(streams)
        both(eng, L.MCS_E_STATE)
        eng.run()
        assert eng.level1_series(0, 5, 10).shape == (3, 10) and eng.level1_at(0, 5)[1] >= 0
    for cfg in (dict(), dict(borrow=True, trader=True)):  # after a FIFO and a FIFO trading run
        with Engine(0, policy="FIFO", **cfg) as eng:
            eng.load_clusters(arrays)
            eng.submit_jobs(streams)
            eng.run()
            both(eng, L.MCS_E_STATE)
    with Engine(0, policy="FIFO") as eng:  # a FIFO session has no Level1
        eng.load_clusters(arrays)
        eng.submit_jobs(streams)
        eng.run(h)
        refused(lambda: eng.online_level1_series(0, 1, 4), L.MCS_E_INVALID)
    with Engine(0, policy="DELAY") as eng:  # a shard of a larger system
        eng.load_clusters(arrays)
        eng.set_shard(1, 2)
        eng.submit_jobs(streams)
        eng.run()
        both(eng, L.MCS_E_STATE, "mcs_set_shard")
