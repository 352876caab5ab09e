"""GPU parity of mcs_online_state_series (include/mcs.h): the ClusterState series, the
wait statistics and the record at t0_s of an online session, read between horizons.

The reference of every comparison is a second engine that runs the whole stream as a batch and answers
through the batch calls (cluster_state_series, wait_time_series), which tests/test_gpu_state_series.py
and tests/test_gpu_wait_series.py pin to host references.  A sample below a finite horizon must equal
the batch run's bit for bit (the wait double as uint64; two NaNs are equal), although
the session has not seen the later jobs yet.  Run on a real MI355X: ``pytest -m gpu``."""
import ctypes as C

import numpy as np
import pytest

from kat_util import seeded_workload
from mcs_amd import CLUSTER_SAMPLE_DTYPE, CLUSTER_STATE_DTYPE, WAIT_SAMPLE_DTYPE, Engine, GenParams, JobStreams, \
    MCSError, replicate, uniform_cluster, wire
from mcs_amd import _lib as L
from mcs_amd.engine import scaled_lambda
from test_gpu_online import horizons_for, slice_streams
from test_gpu_state_series import concat, series_ref, tile
from test_gpu_wait_series import Run, assert_bits_equal, hot_clusters, level1_pressure

pytestmark = pytest.mark.gpu

W = 10
EVER = 1 << 32


def engine(policy, **cfg):
    return Engine(0, policy=policy, max_wait_s=W, **cfg) if policy == "DELAY" else Engine(0, policy=policy, **cfg)


def assert_state_equal(got, want, tag=""):
    """Bit for bit; two NaNs are equal whatever their sign and payload."""
    assert got.shape == want.shape and got.dtype == want.dtype, tag
    for f in got.dtype.names:
        g, w = got[f], want[f]
        same = g.view(np.uint32) == w.view(np.uint32)
        if g.dtype.kind == "f":
            same |= np.isnan(g) & np.isnan(w)
        bad = np.argwhere(~same)
        assert bad.size == 0, f"{tag} {f}: {len(bad)} differ, first {bad[:4].tolist()}: got {g[tuple(bad[0])]} " \
                              f"want {w[tuple(bad[0])]}"


class Batch:
    """The whole stream run as a batch on an engine of its own: every second of [0, T)."""

    def __init__(self, arrays, streams, policy, extra=40):
        self.policy = policy
        with engine(policy) as eng:
            eng.load_clusters(arrays)
            eng.submit_jobs(streams)
            eng.run()
            self.placements = eng.placements()
            self.t_end = eng.cluster_stats()["t_end"].astype(np.int64)
            self.T = int(self.t_end.max()) + extra
            self.state, self.first0 = eng.cluster_state_series(0, 1, self.T)
            self.wait = eng.wait_time_series(0, 1, self.T) if policy == "DELAY" else None
            self.dstats = eng.delay_stats() if policy == "DELAY" else None

    def first(self, t0):
        out = self.first0.copy()
        for f in ("cores_utilization", "memory_utilization", "running"):
            out[f] = self.state[f][:, t0]
        out["t_s"] = t0
        return out

    def check(self, eng, t0, period, n, tag=""):
        """online_state_series over t0 + k * period equals the batch run's samples; returns them."""
        idx = t0 + period * np.arange(n)
        samples, wait, first = eng.online_state_series(t0, period, n)
        assert_state_equal(samples, self.state[:, idx], f"{tag} state t0 {t0} period {period}")
        assert_state_equal(first, self.first(t0), f"{tag} first t0 {t0}")
        if self.policy == "DELAY":
            assert_bits_equal(wait, self.wait[:, idx], f"{tag} wait t0 {t0} period {period}")
        else:
            assert wait is None
        return samples, wait


def run_slices(arrays, streams, policy, hs, ref, submitted_below=None):
    """Submit the jobs below hs[0] (or submitted_below), then append slice [h_{k-1}, h_k) and run(h_k);
    after every run the series over [h_prev, h) at period 1 and over [0, h) at period 5 equal the batch
    run's.  Finally append the rest, drain, and compare every second.  Returns what was non-zero."""
    seen = dict(running=0, queued=0, undecided=0, total_wait_ms=0)
    with engine(policy) as eng:
        eng.load_clusters(arrays)
        cut = hs[0] if submitted_below is None else submitted_below
        eng.submit_jobs(slice_streams(streams, 0, cut))
        prev = 0
        for h in hs:
            if h > cut:
                eng.append_jobs(slice_streams(streams, max(prev, cut), h))
            st = eng.run(h)
            assert st.online and st.t_horizon == h
            s1, w1 = ref.check(eng, prev, 1, h - prev, f"h {h}")
            ref.check(eng, 0, 5, (h + 4) // 5, f"h {h}")
            node, start, _ = eng.placements()
            arr = eng.read_jobs().arrival
            seen["undecided"] += int(((node == L.MCS_NODE_UNPLACED) & (start == L.MCS_TIME_NONE) & (arr < h)).sum())
            seen["running"] += int(s1["running"].sum())
            seen["queued"] += int(s1["queued"].sum())
            if w1 is not None:
                seen["total_wait_ms"] += int(w1["total_wait_ms"].sum())
            with pytest.raises(MCSError) as ei:  # the frontier: the sample at h is not decided
                eng.online_state_series(prev, 1, h - prev + 1)
            assert ei.value.code == L.MCS_E_INVALID and str(h) in str(ei.value)
            prev = h
        eng.append_jobs(slice_streams(streams, max(prev, cut), EVER))
        eng.run()
        for got, want in zip(eng.placements(), ref.placements):
            np.testing.assert_array_equal(got, want)
        ref.check(eng, 0, 1, ref.T, "drained")  # past t_end: the continued Go loop
        ref.check(eng, 3, 7, (ref.T - 3) // 7, "drained")
    return seen


# ---- 1. slices equal the batch series ---------------------------------------------------------------

def workload_small():
    """Five 5-node hot clusters: cluster 2 has no jobs at all, and every job of cluster 3 arrives behind
    the first horizon, so none of them is submitted: all are appended."""
    arrays, streams = hot_clusters([300, 257, 0, 200, 300], 0x4F4E31, nodes=[5] * 5)
    hs = horizons_for(streams, 6)
    streams.arrival[streams.of(3)] += np.uint32(hs[0] + 2)
    return arrays, streams, hs


@pytest.mark.parametrize("policy", ["FIFO", "DELAY"])
def test_slices_of_small_clusters_equal_the_batch_series(policy):
    arrays, streams, hs = workload_small()
    assert streams.job_off[3] == streams.job_off[2]
    assert int(streams.arrival[streams.of(3)].min()) >= hs[0]
    ref = Batch(arrays, streams, policy)
    seen = run_slices(arrays, streams, policy, hs, ref)
    assert seen["running"] > 0 and seen["queued"] > 0 and seen["undecided"] > 0
    if policy == "DELAY":
        assert seen["total_wait_ms"] > 0
        assert (ref.dstats["moved_l1"][[0, 1, 3, 4]] > 0).all()
    assert (ref.state[2]["queued"] == 0).all() and (ref.state[2]["running"] == 0).all()


@pytest.mark.parametrize("policy", ["FIFO", "DELAY"])
def test_slices_of_a_256_node_cluster_equal_the_batch_series(policy):
    """FIFO: a hot 256-node cluster (heavy waiting).  DELAY: the Level1-pressure stream, which the
    hand-scheduled loop hands over and which ends deadlocked: past t_end its Level1 jobs keep being
    examined (the continued Go loop), also in the drained session."""
    if policy == "FIFO":
        arrays, streams, _ = seeded_workload("n256_hot", 1, 1500)
    else:
        arrays, streams = level1_pressure(1, 1500)
    ref = Batch(arrays, streams, policy)
    seen = run_slices(arrays, streams, policy, horizons_for(streams, 4), ref)
    assert seen["running"] > 0 and seen["queued"] > 0 and seen["undecided"] > 0
    if policy == "DELAY":
        assert seen["total_wait_ms"] > 0 and ref.dstats["l1_left"][0] > 0
        k = int(ref.t_end[0])
        assert (np.diff(ref.wait["total_wait_ms"][0, k:]) == 1000 * int(ref.dstats["l1_left"][0])).all()


# ---- 2. segments ------------------------------------------------------------------------------------

def test_series_over_segments_with_slack():
    """A 700-job cluster behind a small one, fed by many tiny appends: its segment starts off a
    multiple of 256, holds several summary batches and moves at every relayout (both read from the
    engine: segment_offsets).  Each slice's series equals the batch run's, agrees with the previous
    slice's on their common samples, and a fresh session that receives the same jobs in one append
    returns the same bytes (nothing stale)."""
    arrays, streams = hot_clusters([100, 700, 300], 0x534547, nodes=[3, 4, 5])
    ref = Batch(arrays, streams, "DELAY")
    top = int(streams.arrival.max()) + 1
    hs = list(range(9, top, max(1, top // 40)))
    relayouts = odd_starts = 0
    with engine("DELAY") as eng:
        eng.load_clusters(arrays)
        eng.submit_jobs(slice_streams(streams, 0, hs[0]))
        eng.run(hs[0])
        seg = eng.segment_offsets()
        assert seg.tolist() == eng.job_offsets().tolist()  # submitted streams have no slack
        before, _, _ = eng.online_state_series(0, 1, hs[0])
        prev = hs[0]
        for h in hs[1:]:
            eng.append_jobs(slice_streams(streams, prev, h))
            now, counts = eng.segment_offsets(), np.diff(eng.job_offsets())
            assert (np.diff(now) >= counts).all()
            relayouts += now.tolist() != seg.tolist()
            seg = now
            eng.run(h)
            after, _ = ref.check(eng, 0, 1, h, f"h {h}")
            assert after[:, :prev].tobytes() == before.tobytes(), f"h {h}: samples below {prev} changed"
            if counts[1] >= 600 and int(seg[1]) % 256 != 0:
                odd_starts += 1
            before, prev = after, h
        last, wait, first = eng.online_state_series(0, 1, prev)
        assert (np.diff(seg) > np.diff(eng.job_offsets())).any()  # slack: the segments are not dense
    assert relayouts >= 3 and odd_starts >= 1
    with engine("DELAY") as fresh:
        fresh.load_clusters(arrays)
        fresh.append_jobs(slice_streams(streams, 0, prev))
        fresh.run(prev)
        s2, w2, f2 = fresh.online_state_series(0, 1, prev)
    assert s2.tobytes() == last.tobytes() and w2.tobytes() == wait.tobytes() and f2.tobytes() == first.tobytes()


# ---- 3. frontier and tiles --------------------------------------------------------------------------

def test_frontier_on_tile_edges_of_a_256_node_cluster(monkeypatch):
    """Horizons whose last sample h - 1 is the last (h = 2 * 35) and then the first (h = 4 * 35 + 1)
    sample of a series tile of the 256-node cluster; at both, one job starts at h - 1 and one arrives
    at h - 1, is still undecided and starts at h.  Fewer clusters than the engine has, and a chunked call."""
    ts = tile(256)
    assert ts == 35
    h1, h2 = 2 * ts, 4 * ts + 1
    big = [(3, 500, 4, 100), (5, 90, 32, 24000), (h1 - 1, 50, 1, 1), (h1 - 1, 10, 1, 1),
           (h2 - 1, 50, 2, 2), (h2 - 1, 10, 1, 1), (h2 + 30, 5, 1, 1)]
    own = JobStreams(*(np.array([j[f] for j in big], np.uint32) for f in range(4)), np.array([0, len(big)], np.uint64))
    arrays, streams = concat([(replicate(uniform_cluster(256), 1), own), hot_clusters([200, 150], 0x54494C, nodes=[5, 4])])
    ref = Batch(arrays, streams, "DELAY")
    rn, rs, _ = ref.placements
    assert rs[2] == h1 - 1 and rs[3] == h1 and rs[4] == h2 - 1 and rs[5] == h2 and (rn[:7] >= 0).all()
    with engine("DELAY") as eng:
        eng.load_clusters(arrays)
        prev = 0
        for h, a_job, b_job in ((h1, 2, 3), (h2, 4, 5)):
            eng.append_jobs(slice_streams(streams, prev, h))
            eng.run(h)
            node, start, _ = eng.placements()
            arr = eng.read_jobs().arrival
            j0 = int(eng.job_offsets()[0])
            assert j0 == 0 and arr[b_job] == h - 1
            assert start[a_job] == h - 1 and node[b_job] == L.MCS_NODE_UNPLACED and start[b_job] == L.MCS_TIME_NONE
            whole, wait = ref.check(eng, 0, 1, h, f"h {h}")
            assert whole["queued"][0, h - 1] >= 1 and whole["running"][0, h - 1] >= 2
            # the first cluster only: its row, nothing behind it
            out = np.zeros((3, h), CLUSTER_SAMPLE_DTYPE)
            wout = np.zeros((3, h), WAIT_SAMPLE_DTYPE)
            fout = np.zeros(3, CLUSTER_STATE_DTYPE)
            for x in (out, wout, fout):
                x.view(np.uint8)[...] = 0xA5
            rc = L.lib().mcs_online_state_series(eng._h, 0, 1, h, out.ctypes.data_as(C.POINTER(L.mcs_cluster_sample)),
                                                 wout.ctypes.data_as(C.POINTER(L.mcs_wait_sample)),
                                                 fout.ctypes.data_as(C.POINTER(L.mcs_cluster_state)), 1, None)
            assert rc == L.MCS_OK
            assert out[:1].tobytes() == whole[:1].tobytes() and wout[:1].tobytes() == wait[:1].tobytes()
            for x in (out, wout, fout):
                assert (x[1:].view(np.uint8) == 0xA5).all()
            monkeypatch.setenv("MCS_SERIES_CHUNK", "7")
            parts, pwait, _ = eng.online_state_series(0, 1, h)
            monkeypatch.delenv("MCS_SERIES_CHUNK")
            assert parts.tobytes() == whole.tobytes() and pwait.tobytes() == wait.tobytes()
            with pytest.raises(MCSError) as ei:
                eng.online_state_series(h, 1, 1)
            assert ei.value.code == L.MCS_E_INVALID
            prev = h


# ---- a session that starts over rows an earlier pass wrote ---------------------------------------------

@pytest.mark.parametrize("restart", ["rewind", "batch"])
def test_restarted_session_with_new_jobs_below_the_horizon(restart):
    """An engine that has decided the first part of every stream (a drained session, or a batch run)
    starts over, receives jobs that arrive below the next horizon h = 64 and runs to h.  One node of
    two cores: A holds one core on [0, 62), B the other on [1, 31); E asks for both and waits in
    Level1.  In the first pass E starts at 62.  The added job F (arrival 40, one core, 30 s) takes the
    core B left, so at 62 E still does not fit and starts at 70.  E's row must read undecided at h,
    not the earlier pass's 62."""
    from mcs_amd import Cluster, Node, pack_clusters

    cl = Cluster(Id=1, Nodes=[Node(Id=1, Cores=2, Memory=8, CoresAvailable=2, MemoryAvailable=8)])
    arrays = pack_clusters([cl, cl])
    first = [(0, 62, 1, 1), (1, 30, 1, 1), (5, 30, 2, 1)]  # A, B, E (row E: Level1 from second 15)
    added = [(40, 30, 1, 1), (80, 4, 1, 1)]                # F, and a job past h
    h, E = 64, 2

    def two(jobs):  # the same stream in both clusters
        cols = [np.array([j[f] for j in jobs] * 2, np.uint32) for f in range(4)]
        return JobStreams(*cols, np.array([0, len(jobs), 2 * len(jobs)], np.uint64))

    whole = two(first + added)
    ref = Batch(arrays, whole, "DELAY")
    rs = ref.placements[1]
    with engine("DELAY") as eng:
        eng.load_clusters(arrays)
        eng.submit_jobs(two(first))
        eng.run()
        old = eng.placements()[1]
        assert old[E] == 62 and rs[E] == 70  # the earlier pass started E below h; the whole run does not
        if restart == "rewind":
            eng.run(3)  # (a session, so that rewind has one to restart)
            eng.run()
            eng.rewind()
        eng.append_jobs(two(added))
        eng.run(h)
        node, start, _ = eng.placements()
        assert node[E] == L.MCS_NODE_UNPLACED and start[E] == L.MCS_TIME_NONE
        ref.check(eng, 0, 1, h, restart)
        eng.run()
        for got, want in zip(eng.placements(), ref.placements):
            np.testing.assert_array_equal(got, want)
        ref.check(eng, 0, 1, ref.T, restart + " drained")


# ---- 5. refusals and unchanged behaviour ------------------------------------------------------------

def refused(call, code):
    with pytest.raises(MCSError) as ei:
        call()
    assert ei.value.code == code, ei.value
    return str(ei.value)


def test_refusals():
    arrays, streams, _ = seeded_workload("small", 3, 200)
    h = int(np.median(streams.arrival))
    with Engine(0, policy="DELAY") as eng:
        eng.load_clusters(arrays)
        refused(lambda: eng.online_state_series(0, 5, 2), L.MCS_E_STATE)  # nothing loaded, no session
        eng.submit_jobs(streams)
        refused(lambda: eng.online_state_series(0, 5, 2), L.MCS_E_STATE)  # before a run
        eng.run()
        refused(lambda: eng.online_state_series(0, 5, 2), L.MCS_E_STATE)  # a batch run is no session
        eng.run(h)                                                         # (starts a session at t = 0)
        assert eng.online_state_series(0, 1, h)[0].shape == (3, h)
        assert "%d" % h in refused(lambda: eng.online_state_series(0, 1, h + 1), L.MCS_E_INVALID)  # a sample at h
        refused(lambda: eng.online_state_series(h, 1, 1), L.MCS_E_INVALID)
        refused(lambda: eng.online_state_series(0, 0, 4), L.MCS_E_INVALID)
        refused(lambda: eng.online_state_series(0, 5, 0), L.MCS_E_INVALID)
        f = L.lib().mcs_online_state_series
        out = np.zeros((4, 4), CLUSTER_SAMPLE_DTYPE)
        po = out.ctypes.data_as(C.POINTER(L.mcs_cluster_sample))
        assert f(eng._h, 0, 1, 4, None, None, None, 3, None) == L.MCS_E_INVALID   # out == NULL
        assert f(eng._h, 0, 1, 4, po, None, None, 4, None) == L.MCS_E_INVALID     # more clusters than the engine has
        assert f(eng._h, 0, 1, 4, po, None, None, 0, None) == L.MCS_OK            # no cluster asked for
        assert f(eng._h, 0, 1, 4, po, None, None, 3, None) == L.MCS_OK            # wait and first may be NULL
        eng.rewind()
        refused(lambda: eng.online_state_series(0, 1, 4), L.MCS_E_STATE)  # after rewind, before a run
        eng.run(h)
        again = eng.online_state_series(0, 1, h)
        eng.run()  # a drain: every second up to 0xFFFFFFFE
        assert eng.online_state_series(0xFFFFFFFB, 1, 4)[0]["running"].max() == 0
        refused(lambda: eng.online_state_series(0xFFFFFFFC, 1, 4), L.MCS_E_INVALID)
        assert eng.online_state_series(0, 1, h)[0].tobytes() == again[0].tobytes()
    with Engine(0, policy="FIFO") as eng:  # wait statistics under FIFO
        eng.load_clusters(arrays)
        eng.append_jobs(slice_streams(streams, 0, h))
        eng.run(h)
        refused(lambda: eng.online_state_series(0, 1, h, with_wait=True), L.MCS_E_INVALID)
        samples, wait, first = eng.online_state_series(0, 1, h)
        assert wait is None and first["t_s"].tolist() == [0, 0, 0]
        # the batch calls keep refusing a session with appended jobs, and name the call that serves it
        for call in (lambda: eng.cluster_states(0), lambda: eng.cluster_state_series(0, 1, 4),
                     lambda: eng.dtrade_state_series(0, 1, 4)):
            assert "mcs_online_state_series" in refused(call, L.MCS_E_STATE)
    with Engine(0, policy="DELAY") as eng:
        eng.load_clusters(arrays)
        eng.append_jobs(streams)
        eng.run()
        assert "mcs_online_state_series" in refused(lambda: eng.wait_time_series(0, 1, 4), L.MCS_E_STATE)
        assert eng.online_state_series(0, 5, 8)[1].shape == (3, 8)
    with Engine(0, policy="DELAY", trader=True) as eng:  # after a trading run
        eng.load_clusters(arrays)
        eng.submit_jobs(streams)
        eng.run()
        refused(lambda: eng.online_state_series(0, 5, 2, with_wait=False), L.MCS_E_STATE)


def test_plain_batch_calls_did_not_move():
    """The plain instantiations share their source with the segmented ones: after a batch run they still
    return what the host references give (series_ref per sample, wait_ref's replay of the Go loop)."""
    arrays, streams = hot_clusters([300, 257, 120], 0x504C4E, nodes=[3, 2, 4])
    with Engine(0, policy="DELAY", max_wait_s=W) as eng:
        eng.load_clusters(arrays)
        eng.submit_jobs(streams)
        st = eng.run()
        run = Run(eng, arrays, streams, W, st)  # (asserts the placements equal the oracle's)
        T = int(run.t_end.max()) + 4
        n = T // 3
        samples, first = eng.cluster_state_series(1, 3, n)
        want = series_ref(arrays, streams, run.node, run.start, run.fin, 1, 3, n)
        assert_state_equal(samples, want)
        assert_state_equal(first[["cores_utilization", "memory_utilization", "running"]],
                           eng.cluster_states(1)[["cores_utilization", "memory_utilization", "running"]])
        assert samples["running"].max() > 0 and samples["queued"].max() > 0
        run.assert_wrong_restatements_differ(T)
        assert_bits_equal(eng.wait_time_series(0, 1, T + 1), run.want(0, 1, T + 1))


# ---- 6. a fused generated stream --------------------------------------------------------------------

def test_fused_session_equals_the_materialised_one():
    arrays = replicate(uniform_cluster(8), 5)
    got = []
    for fused in (False, True):
        gp = GenParams(seed=0xF05ED, arrival_mode=1, max_dur_s=60, lam=scaled_lambda(8, max_dur_s=60, load=1.15),
                       fused=fused)
        with Engine(0, policy="DELAY", max_wait_s=W) as eng:
            eng.load_clusters(arrays)
            eng.generate_jobs(gp, 500)
            if not fused:
                streams = eng.read_jobs()
                ref = Batch(arrays, streams, "DELAY")
                hs = horizons_for(streams, 2)
            parts = []
            for h in hs:
                st = eng.run(h)
                assert st.pending > 0
                parts.append(ref.check(eng, 0, 5, (h + 4) // 5, f"fused {fused} h {h}"))
            eng.run()
            parts.append(ref.check(eng, 0, 5, ref.T // 5, f"fused {fused} drained"))
            got.append(parts)
    for a, b in zip(*got):
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    assert got[1][-1][1]["total_wait_ms"][:, -1].min() > 0


# ---- the Start stream -------------------------------------------------------------------------------

def test_rows_feed_the_start_stream_slice_by_slice():
    """5 s slices, each served at once as the 5 s Start stream: the messages of all slices are the
    batch run's stream."""
    arrays, streams = hot_clusters([120, 90], 0x535452, nodes=[3, 2])
    ref = Batch(arrays, streams, "DELAY")
    top = (int(streams.arrival.max()) // 5 + 2) * 5
    rows = [[] for _ in range(2)]
    with engine("DELAY") as eng:
        eng.load_clusters(arrays)
        for h in range(5, top + 1, 5):
            eng.append_jobs(slice_streams(streams, h - 5, h))
            eng.run(h)
            samples, wait, first = eng.online_state_series(h - 5, 5, 1)
            for c in range(2):
                rows[c] += wire.start_stream(samples[c], first[c], wait["average_wait_time"][c])
    n = top // 5
    assert top <= ref.T
    for c in range(2):
        assert len(rows[c]) == n
        for k in range(n):  # (every slice's message is the first of its call: it carries the totals)
            want = wire.start_stream(ref.state[c, 5 * k:5 * k + 1], ref.first(5 * k)[c],
                                     ref.wait["average_wait_time"][c, 5 * k:5 * k + 1])[0]
            assert wire.marshal(rows[c][k]) == wire.marshal(want), (c, k)
    assert max(m.average_wait_time for m in rows[0]) > 0
