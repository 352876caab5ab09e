"""GPU parity of the start-stream cursor (mcs_stream_open / mcs_stream_next / mcs_stream_close;
include/mcs.h).

The reference of every sample is mcs_online_state_series on the same engine at the same moment, bit for
bit (the wait double as uint64), which tests/test_gpu_online_series.py pins to the batch calls; the
relayout case also compares with a fresh engine run in one batch.  The stream keeps batch summaries,
wait records and carried constants between calls and retires batches, so every case takes its samples
in many calls, between appends and horizons.  Run on a real MI355X: ``pytest -m gpu``."""
import ctypes as C

import numpy as np
import pytest

from mcs_amd import CLUSTER_SAMPLE_DTYPE, WAIT_SAMPLE_DTYPE, Engine, GenParams, JobStreams, replicate, uniform_cluster
from mcs_amd import _lib as L
from mcs_amd.engine import scaled_lambda
from test_gpu_online import horizons_for, slice_streams, truncate_streams
from test_gpu_online_series import EVER, W, Batch, assert_state_equal, engine, refused, workload_small
from test_gpu_wait_series import assert_bits_equal, hot_clusters, level1_pressure

pytestmark = pytest.mark.gpu

BATCH = 256  # kSeriesBatch: the rows of one retired unit


def n_below(t0, period, h):
    """samples t0 + k * period below h"""
    return (h - t0 + period - 1) // period if h > t0 else 0


class Follower:
    """An open stream and what it must hand out next; every call is compared with online_state_series."""

    def __init__(self, eng, t0, period, with_wait=None):
        self.eng, self.t, self.period = eng, t0, period
        eng.stream_open(t0, period, with_wait)
        self.samples, self.wait, self.stats = [], [], []

    def take(self, h, max_samples=None, tag=""):
        """One mcs_stream_next with the last finite horizon h; returns its stats."""
        eng, p = self.eng, self.period
        pend = n_below(self.t, p, h)
        m = max(pend, 1) if max_samples is None else max_samples
        s, w, st = eng.stream_next(m)
        n = min(pend, m)
        assert st["n_written"] == n and s.shape == (eng.num_clusters, n), f"{tag}: {st}"
        assert st["t_next"] == self.t + n * p and st["pending"] == pend - n, f"{tag}: {st}"
        if n:
            assert st["t_first"] == self.t
            want_s, want_w, _ = eng.online_state_series(self.t, p, n)
            assert_state_equal(s, want_s, f"{tag} state t0 {self.t} period {p} n {n}")
            if w is not None:
                assert_bits_equal(w, want_w, f"{tag} wait t0 {self.t} period {p} n {n}")
            self.samples.append(s)
            self.wait.append(w)
        if self.stats:
            assert st["rows_retired"] >= self.stats[-1]["rows_retired"], f"{tag}: retired rows came back"
        self.stats.append(st)
        self.t += n * p
        return st

    def take_all(self, h, piece=None, tag=""):
        st = self.take(h, piece, tag)
        while st["pending"]:
            st = self.take(h, piece, tag)
        return st


def follow_slices(arrays, streams, policy, hs, t0, period, piece=None, cut=None):
    """Submit the jobs below hs[0] (or cut), open the stream, then per horizon: append the slice, run,
    take what is pending (in pieces of `piece` samples).  Returns the follower and the engine's last
    placements."""
    with engine(policy) as eng:
        eng.load_clusters(arrays)
        cut = hs[0] if cut is None else cut
        eng.submit_jobs(slice_streams(streams, 0, cut))
        prev = 0
        fol = None
        for h in hs:
            if h > cut:
                eng.append_jobs(slice_streams(streams, max(prev, cut), h))
            eng.run(h)
            if fol is None:
                fol = Follower(eng, t0, period)
            fol.take_all(h, piece, f"{policy} h {h}")
            prev = h
        assert fol.t >= prev and fol.take(prev)["n_written"] == 0  # nothing is handed out twice
        return fol, eng.placements()


# ---- 1. small hot clusters ---------------------------------------------------------------------------

@pytest.mark.parametrize("t0,period", [(0, 1), (0, 5), (3, 7)])
@pytest.mark.parametrize("policy", ["FIFO", "DELAY"])
def test_small_hot_clusters(policy, t0, period):
    """Five 5-node clusters (one without jobs, one whose jobs are all appended).  The horizons fall on a
    sample second, one below one and one above one; every second slice is taken in pieces of 7."""
    arrays, streams, hs = workload_small()
    on = lambda h: t0 + period * ((h - t0) // period)
    hs = sorted({on(hs[0]), on(hs[1]) - 1, on(hs[2]) + 1, *hs[3:]})
    assert (hs[0] - t0) % period == 0 and (hs[1] + 1 - t0) % period == 0 and (hs[2] - 1 - t0) % period == 0
    with engine(policy) as eng:
        eng.load_clusters(arrays)
        eng.submit_jobs(slice_streams(streams, 0, hs[0]))
        fol, prev = None, 0
        for k, h in enumerate(hs):
            if k:
                eng.append_jobs(slice_streams(streams, prev, h))
            eng.run(h)
            fol = fol or Follower(eng, t0, period)
            fol.take_all(h, 7 if k % 2 else None, f"{policy} h {h}")
            prev = h
        got = np.concatenate(fol.samples, axis=1)
        assert got.shape[1] == n_below(t0, period, prev)
        assert got["running"].max() > 0 and got["queued"].max() > 0
        assert (got[2]["running"] == 0).all() and (got[2]["queued"] == 0).all()  # the cluster without jobs
        if policy == "DELAY":
            assert np.concatenate(fol.wait, axis=1)["total_wait_ms"].max() > 0
        eng.stream_close()


def test_256_node_cluster_that_deadlocks():
    """The Level1-pressure stream: requests that fit no node starve in Level1 all along the stream, so
    no batch of the cluster is ever final; nothing retires, and the samples are right."""
    arrays, streams = level1_pressure(1, 1500)
    fol, _ = follow_slices(arrays, streams, "DELAY", horizons_for(streams, 4), 0, 1)
    assert fol.stats[-1]["rows_retired"] == 0
    assert np.concatenate(fol.wait, axis=1)["total_wait_ms"].max() > 0


# ---- 2. relayouts ------------------------------------------------------------------------------------

@pytest.mark.parametrize("load", ["hot", "light"])
def test_stream_survives_relayouts(load):
    """The 700-job segment off a multiple of 256 of test_series_over_segments_with_slack (overloaded: its
    queue grows, no batch becomes final) and lightly loaded clusters of 100, 700 and 300 jobs (batches retire all
    along): appends between the calls move every segment, the kept arrays with them.  What the stream
    handed out, put together, equals a fresh engine's batch run through the batch calls."""
    if load == "hot":
        arrays, streams = hot_clusters([100, 700, 300], 0x534547, nodes=[3, 4, 5])
    else:
        arrays, full = slice_workload(9, 3, 700)
        streams = truncate_streams(full, [100, 700, 300])
    ref = Batch(arrays, streams, "DELAY")
    top = int(streams.arrival.max()) + 1
    hs = list(range(9, top, max(1, top // 40)))
    relayouts = odd_starts = 0
    with engine("DELAY") as eng:
        eng.load_clusters(arrays)
        eng.submit_jobs(slice_streams(streams, 0, hs[0]))
        eng.run(hs[0])
        fol = Follower(eng, 0, 1)
        fol.take_all(hs[0])
        seg, prev = eng.segment_offsets(), hs[0]
        for h in hs[1:]:
            eng.append_jobs(slice_streams(streams, prev, h))
            now = eng.segment_offsets()
            relayouts += now.tolist() != seg.tolist()
            odd_starts += int(np.diff(eng.job_offsets())[1] >= 600 and int(now[1]) % BATCH != 0)
            seg = now
            eng.run(h)
            fol.take_all(h, None, f"h {h}")
            prev = h
        assert relayouts >= 3 and odd_starts >= 1
        if load == "light":  # retired batches were carried through the relayouts
            assert min(st["rows_retired"] for st in fol.stats[len(fol.stats) // 2:]) >= 2 * BATCH
    got, wait = np.concatenate(fol.samples, axis=1), np.concatenate(fol.wait, axis=1)
    assert got.shape[1] == prev
    assert_state_equal(got, ref.state[:, :prev], "stream against the batch run")
    assert_bits_equal(wait, ref.wait[:, :prev], "stream against the batch run")


# ---- 3. opened mid-session, more than 256 samples, chunked launches ---------------------------------

@pytest.mark.parametrize("chunk", [None, 100])
def test_opened_mid_session_catches_up(monkeypatch, chunk):
    """t0 = 2 far below the horizon: the first call walks the history once and hands out more than 256
    samples (several rounds of wait_finish_kernel, several series tiles; with MCS_SERIES_CHUNK several
    launches), later calls cost the slice."""
    arrays, streams = slice_workload(11, 3, 700)
    hs = horizons_for(streams, 6)
    assert hs[2] > 2 + 256
    if chunk:
        monkeypatch.setenv("MCS_SERIES_CHUNK", str(chunk))
    with engine("DELAY") as eng:
        eng.load_clusters(arrays)
        prev = 0
        for h in hs[:3]:
            eng.append_jobs(slice_streams(streams, prev, h))
            eng.run(h)
            prev = h
        fol = Follower(eng, 2, 1)
        first = fol.take(prev, None, "catch-up")
        assert first["n_written"] == prev - 2 > 256 and first["pending"] == 0
        rows = int(eng.job_offsets()[-1])
        assert first["rows_scanned"] == rows  # the history, once
        for h in hs[3:]:
            eng.append_jobs(slice_streams(streams, prev, h))
            eng.run(h)
            st = fol.take_all(h, 300, f"h {h}")
            prev = h
        assert st["rows_retired"] >= 2 * BATCH
        assert st["rows_scanned"] < int(eng.job_offsets()[-1])  # and no longer the history


# ---- 4. a fused generated stream ----------------------------------------------------------------------

def test_fused_stream():
    arrays = replicate(uniform_cluster(8), 3)
    gp = GenParams(seed=0xF05ED, arrival_mode=1, max_dur_s=60, lam=scaled_lambda(8, max_dur_s=60, load=1.15),
                   fused=True)
    with Engine(0, policy="DELAY", max_wait_s=W) as eng:
        eng.load_clusters(arrays)
        eng.generate_jobs(gp, 500)
        with Engine(0, policy="DELAY", max_wait_s=W) as plain:  # the same stream, materialised: its span
            plain.load_clusters(arrays)
            plain.generate_jobs(GenParams(seed=gp.seed, arrival_mode=1, max_dur_s=60, lam=gp.lam, fused=False), 500)
            hs = horizons_for(plain.read_jobs(), 3)
        fol = None
        for h in hs:
            assert eng.run(h).pending > 0
            fol = fol or Follower(eng, 0, 5)
            fol.take_all(h, None, f"fused h {h}")
        assert np.concatenate(fol.samples, axis=1)["running"].max() > 0


# ---- 5. life cycle -----------------------------------------------------------------------------------

def test_life_cycle():
    arrays, streams = hot_clusters([300, 257, 120], 0x4C4946, nodes=[3, 2, 4])
    h1, h2, h3 = horizons_for(streams, 3)
    with engine("DELAY") as eng:
        eng.load_clusters(arrays)
        assert L.MCS_E_STATE == L.lib().mcs_stream_open(eng._h, 0, 5, 1)   # no session
        refused(lambda: eng.stream_next(4), L.MCS_E_STATE)
        refused(eng.stream_close, L.MCS_E_STATE)
        eng.submit_jobs(slice_streams(streams, 0, h1))
        eng.run()
        refused(lambda: eng.stream_open(0, 5), L.MCS_E_STATE)              # a batch run is no session
        eng.run(h1)
        refused(lambda: eng.stream_open(0, 0), L.MCS_E_INVALID)            # period 0
        fol = Follower(eng, 0, 5)
        assert "open" in refused(lambda: eng.stream_open(0, 5), L.MCS_E_STATE)  # one stream per engine
        f = L.lib().mcs_stream_next
        out, wout = np.zeros((4, 8), CLUSTER_SAMPLE_DTYPE), np.zeros((4, 8), WAIT_SAMPLE_DTYPE)
        po, pw = out.ctypes.data_as(C.POINTER(L.mcs_cluster_sample)), wout.ctypes.data_as(C.POINTER(L.mcs_wait_sample))
        assert f(eng._h, 8, po, pw, 2, None) == L.MCS_E_INVALID            # fewer clusters than the engine has
        assert f(eng._h, 8, po, pw, 4, None) == L.MCS_E_INVALID            # and more
        assert f(eng._h, 8, None, pw, 3, None) == L.MCS_E_INVALID
        assert f(eng._h, 0, po, pw, 3, None) == L.MCS_E_INVALID
        assert f(eng._h, 8, po, None, 3, None) == L.MCS_E_INVALID          # opened with wait statistics
        refused(lambda: eng.run(h1 - 1), L.MCS_E_INVALID)                  # a decreasing horizon: nothing ran
        fol.take(h1, 3)                                                    # (none of these moved the stream)
        # a drain does not move the frontier: what is pending below h1 is served, then nothing
        eng.append_jobs(slice_streams(streams, h1, h2))
        eng.run()
        st = fol.take_all(h1, 4, "after the drain")
        assert st["t_next"] >= h1 and fol.take(h1)["n_written"] == 0
        # the first run after a drain closes it
        eng.append_jobs(slice_streams(streams, max(h2, int(eng.cluster_stats()["t_end"].max())), EVER))
        eng.run(h3 + 1000)
        assert "drain" in refused(lambda: eng.stream_next(4), L.MCS_E_STATE)
        assert "drain" in refused(lambda: eng.stream_next(4), L.MCS_E_STATE)   # until it is reopened
        eng.stream_close()                                                 # acknowledges the close
        refused(eng.stream_close, L.MCS_E_STATE)
        # reopened: right again, from any second
        fol = Follower(eng, 1, 3)
        assert fol.take_all(h3 + 1000, 500, "reopened")["n_written"] > 0
        eng.rewind()
        assert "mcs_rewind" in refused(lambda: eng.stream_next(4), L.MCS_E_STATE)
        eng.run(h2)
        fol = Follower(eng, 0, 5)
        fol.take_all(h2)
        eng.stream_close()
        assert "no stream" in refused(lambda: eng.stream_next(4), L.MCS_E_STATE)
        for name, call in (("mcs_submit_jobs", lambda: eng.submit_jobs(streams)),
                           ("mcs_generate_jobs", lambda: eng.generate_jobs(GenParams(seed=1, max_dur_s=20), 50)),
                           ("mcs_load_clusters", lambda: eng.load_clusters(arrays))):
            eng.load_clusters(arrays)  # a fresh session
            eng.submit_jobs(slice_streams(streams, 0, h1))
            eng.run(h1)
            eng.stream_open(0, 5)
            call()
            assert name in refused(lambda: eng.stream_next(4), L.MCS_E_STATE)
    with engine("FIFO") as eng:  # the wait statistics under FIFO
        eng.load_clusters(arrays)
        eng.append_jobs(slice_streams(streams, 0, h1))
        eng.run(h1)
        refused(lambda: eng.stream_open(0, 5, with_wait=True), L.MCS_E_INVALID)
        fol = Follower(eng, 0, 5)
        assert fol.take_all(h1)["n_written"] > 0 and fol.wait[0] is None


@pytest.mark.parametrize("policy", ["FIFO", "DELAY"])
def test_a_failed_run_closes_the_stream(policy):
    """The clock-range stream of test_clock_overflow_is_an_error_with_unplaced_rows: the horizon that
    reaches the wrap fails with MCS_E_RANGE, and the stream does not outlive it."""
    big = 0xFFFFFF00
    arrays = replicate(uniform_cluster(2, cores=4, memory=10), 2)
    s = JobStreams(np.array([big, big, 5, 6], np.uint32), np.array([0x200, 3, 4, 4], np.uint32),
                   np.array([4, 4, 1, 1], np.uint32), np.array([1, 1, 1, 1], np.uint32), np.array([0, 2, 4], np.uint64))
    with Engine(0, policy=policy, unchecked_horizon=1) as eng:
        eng.load_clusters(arrays)
        eng.submit_jobs(s)
        eng.run(20)
        fol = Follower(eng, 0, 1)
        assert fol.take_all(20)["n_written"] == 20
        rc, _ = eng.run_status(0xFFFFFFFE)
        assert rc == L.MCS_E_RANGE
        assert "failed" in refused(lambda: eng.stream_next(4), L.MCS_E_STATE)
        refused(lambda: eng.stream_open(0, 1), L.MCS_E_STATE)  # until the session starts over
        eng.rewind()
        eng.run(20)
        assert Follower(eng, 0, 1).take_all(20)["n_written"] == 20


# ---- 6. cost follows the slice -----------------------------------------------------------------------

def slice_workload(seed, clusters=4, jobs=8000):
    arrays = replicate(uniform_cluster(5, cores=32, memory=24000), clusters)
    rng = np.random.default_rng(seed)
    parts = []
    for _ in range(clusters):
        arr = np.cumsum(rng.poisson(1.0, jobs))
        parts.append((arr, rng.integers(0, 20, jobs), rng.integers(0, 17, jobs), rng.integers(0, 12001, jobs)))
    off = (np.arange(clusters + 1) * jobs).astype(np.uint64)
    return arrays, JobStreams(*(np.concatenate([p[f] for p in parts]).astype(np.uint32) for f in range(4)), off)


@pytest.mark.parametrize("policy,seed", [("DELAY", 7), ("DELAY", 8), ("FIFO", 7)])
def test_cost_follows_the_slice(policy, seed):
    """40 equal slices of the arrival span, one call per slice at period 5.  A condition, not a timing:
    with R the session's rows, the rows loaded over the 40 calls stay within 5 R (a history rescan loads
    20.7 R; retiring the batches that finished before the previous call's first sample 2.7 - 2.9 R, one
    more live batch per call adds 1.3 R: counted on the oracle's runs of these streams).  The retired
    rows never shrink, and they are exactly the full batches whose rows are all decided and finished
    below the stream's next sample second."""
    arrays, streams = slice_workload(seed)
    R = int(streams.job_off[-1])
    top = int(streams.arrival.max()) + 1
    hs = [top * k // 40 for k in range(1, 41)]
    scanned = 0
    with engine(policy) as eng:
        eng.load_clusters(arrays)
        eng.append_jobs(slice_streams(streams, 0, hs[0]))
        eng.run(hs[0])
        fol = Follower(eng, 0, 5)
        prev = 0
        for k, h in enumerate(hs):
            if k:
                eng.append_jobs(slice_streams(streams, prev, h))
                eng.run(h)
            st = fol.take(h, None, f"slice {k}")
            assert st["pending"] == 0
            scanned += st["rows_scanned"]
            node, _, fin = eng.placements()
            off = eng.job_offsets()
            want = 0
            for c in range(len(off) - 1):
                nd, fn = node[int(off[c]):int(off[c + 1])], fin[int(off[c]):int(off[c + 1])].astype(np.int64)
                full = len(nd) // BATCH * BATCH
                ok = ((nd[:full] >= 0) & (fn[:full] < st["t_next"])).reshape(-1, BATCH).all(axis=1)
                want += BATCH * int(ok.sum())
            assert st["rows_retired"] == want, f"slice {k}: {st['rows_retired']} rows retired, {want} retirable"
            prev = h
        print(f"{policy} seed {seed}: rows_scanned {scanned} = {scanned / R:.2f} R, retired {st['rows_retired']} of {R}")
        assert int(eng.job_offsets()[-1]) == R
        assert scanned <= 5 * R
        assert st["rows_retired"] > R // 2
