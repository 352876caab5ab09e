"""GPU parity of Level1 samples on the start-stream cursors (mcs_stream_open_level1 / mcs_stream_next_level1
and the mcs_trade_stream_* pair; include/mcs.h, include/mcs_trade.h, DESIGN.md §14 "Level1 on the cursors").

The reference of every Level1 sample is mcs_online_level1_series (mcs_trade_session_level1_series in a
trading session) on the same engine at the same moment, bit for bit, which tests/test_gpu_level1_series.py
and tests/test_gpu_dtrade_session_series.py pin to the batch calls and to the replay of the Go loop; the
state and wait samples of the same call are compared with the state series as the cursors' own tests do.
Where the series call refuses (jobs appended behind a drain) the reference is a batch engine over all the
jobs the session ever receives.  The cursor carries its scan bounds and its batch summaries between calls,
so every case takes its samples in many calls, between appends, horizons, drains and replays.  The rows
each call scans are compared with the count tests/test_level1_stream_ref.py derives from the rule.
Run on a real MI355X: ``pytest -m gpu``."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import level1_cases as K
from kat_util import seeded_workload
from mcs_amd import (CLUSTER_SAMPLE_DTYPE, LEVEL1_SAMPLE_DTYPE, WAIT_SAMPLE_DTYPE, Engine, GenParams, JobStreams,
                     replicate, uniform_cluster)
from mcs_amd import _lib as L
from mcs_amd.engine import scaled_lambda
from test_gpu_dtrade_session import concat_streams, raises, session
from test_gpu_dtrade_session import slice_streams as trade_slice
from test_gpu_dtrade_session_series import Batch as TradeBatch
from test_gpu_dtrade_session_stream import frontier_of, n_below
from test_gpu_online import horizons_for, slice_streams, truncate_streams
from test_gpu_online_series import EVER, W, assert_state_equal, engine, refused, workload_small
from test_gpu_online_stream import slice_workload
from test_gpu_wait_series import assert_bits_equal, hot_clusters, level1_pressure
from test_level1_ref import contracts_equal_samples
from test_level1_stream_ref import COST_PERIOD, cost_case, walk_system
from test_online_stream_ref import workload as ref_workload

pytestmark = pytest.mark.gpu

BATCH = 256


class Follower:
    """A stream opened with Level1 and what it must hand out next.  Every call's three arrays are compared
    with the series calls on the same engine, or with `ref` (a TradeBatch at period 1) where they refuse."""

    def __init__(self, eng, t0, period, with_wait=True, trade=False):
        self.eng, self.t, self.period, self.with_wait, self.trade = eng, t0, period, with_wait, trade
        if trade:
            eng.trade_stream_open(t0, period, with_wait, with_level1=True)
            self.F = frontier_of(eng)
        else:
            eng.stream_open(t0, period, with_wait, with_level1=True)
            self.F = 0
        self.state, self.wait, self.level1, self.stats = [], [], [], []

    def ran(self, h=None):
        """after a successful run(h), or a trading session's drain (h None)"""
        if h is None:
            info = self.eng.trade_session_info()
            h = info["t_last"] + 1 if info["ticks_total"] else 0
        self.F = max(self.F, h)

    def take(self, max_samples=None, tag="", ref=None):
        eng, p = self.eng, self.period
        pend = n_below(self.t, p, self.F)
        m = max(pend, 1) if max_samples is None else max_samples
        s, w, l1, st = (eng.trade_stream_next if self.trade else eng.stream_next)(m)
        n = min(pend, m)
        assert st["n_written"] == n and s.shape == l1.shape == (eng.num_clusters, n), f"{tag}: {st}"
        assert st["t_next"] == self.t + n * p and st["pending"] == pend - n, f"{tag}: {st}"
        assert (w is None) == (not self.with_wait) and l1.dtype == LEVEL1_SAMPLE_DTYPE
        if n:
            what = f"{tag} t0 {self.t} period {p} n {n}"
            if ref is not None:
                idx = self.t + p * np.arange(n)
                want_s, want_w, want_l1 = ref.state[:, idx], ref.wait[:, idx], ref.l1[:, idx]
            elif self.trade:
                want_s, want_w, _ = eng.trade_session_state_series(self.t, p, n, with_wait=self.with_wait)
                want_l1 = eng.trade_session_level1_series(self.t, p, n)
            else:
                want_s, want_w, _ = eng.online_state_series(self.t, p, n)
                want_l1 = eng.online_level1_series(self.t, p, n)
            K.assert_samples_equal(l1, np.ascontiguousarray(want_l1), f"{what} level1")
            assert l1.tobytes() == np.ascontiguousarray(want_l1).tobytes(), what
            assert_state_equal(s, want_s, f"{what} state")
            if w is not None:
                assert_bits_equal(w, want_w, f"{what} wait")
            assert 0.0 < st["level1_kernel_ms"] <= st["kernel_ms"], f"{tag}: {st}"
            self.state.append(s), self.wait.append(w), self.level1.append(l1)
        else:
            assert st["level1_rows_scanned"] == 0 and st["level1_kernel_ms"] == 0.0, f"{tag}: {st}"
        self.stats.append(st)
        self.t += n * p
        return st

    def take_all(self, piece=None, tag="", ref=None):
        st = self.take(piece, tag, ref)
        while st["pending"]:
            st = self.take(piece, tag, ref)
        return st

    def all_level1(self):
        return np.concatenate(self.level1, axis=1)


def follow_slices(arrays, streams, hs, t0, period, pieces=(None,), with_wait=True, open_at=0, cut=None):
    """Submit the jobs below hs[0] (or cut); per horizon append the slice, run, take what is pending, slice
    k in pieces of pieces[k % len(pieces)] samples.  The stream is opened after run number open_at."""
    with engine("DELAY") as eng:
        eng.load_clusters(arrays)
        cut = hs[0] if cut is None else cut
        eng.submit_jobs(slice_streams(streams, 0, cut))
        fol, prev = None, 0
        for k, h in enumerate(hs):
            if h > cut:
                eng.append_jobs(slice_streams(streams, max(prev, cut), h))
            eng.run(h)
            prev = h
            if fol is None and k >= open_at:
                fol = Follower(eng, t0, period, with_wait)
            if fol is not None:
                fol.ran(h)
                fol.take_all(pieces[k % len(pieces)], f"h {h}")
        assert fol.t >= prev and fol.take()["n_written"] == 0  # nothing is handed out twice
        eng.stream_close()
    return fol


# ---- 1. plain sessions: periods, horizons, pieces ------------------------------------------------------

@pytest.mark.parametrize("t0,period,with_wait", [(0, 1, True), (0, 5, True), (3, 7, True), (0, 5, False)])
def test_small_hot_clusters(t0, period, with_wait):
    """Five 5-node clusters (one without jobs, one whose jobs are all appended).  The horizons fall on a
    sample second, one below one and one above one; the slices are taken whole, one sample at a time and
    three at a time in turn."""
    arrays, streams, hs = workload_small()
    on = lambda h: t0 + period * ((h - t0) // period)
    hs = sorted({on(hs[0]), on(hs[1]) - 1, on(hs[2]) + 1, *hs[3:]})
    assert (hs[0] - t0) % period == 0 and (hs[1] + 1 - t0) % period == 0 and (hs[2] - 1 - t0) % period == 0
    fol = follow_slices(arrays, streams, hs, t0, period, (None, 1, 3), with_wait)
    got = fol.all_level1()
    assert got.shape[1] == n_below(t0, period, hs[-1])
    assert (got[2]["len"] == 0).all() and (got[2]["head"] == L.MCS_TIME_NONE).all()  # the cluster without jobs
    assert (got["len"].max(axis=1)[[0, 1, 3, 4]] > 0).all()
    assert sum(st["level1_rows_scanned"] for st in fol.stats) > 0


def test_ref_workload_with_the_starved_row():
    """tests/test_online_stream_ref.py's DELAY workload: row 600 of the last cluster starves for good and
    pins the lower bound while the batches behind it finish and retire."""
    arrays, streams = ref_workload("DELAY")
    top = int(streams.arrival.max()) + 1
    hs = list(range(40, top + 600, 97))
    with engine("DELAY") as eng:
        eng.load_clusters(arrays)
        eng.append_jobs(slice_streams(streams, 0, hs[0]))
        fol, prev = None, hs[0]
        for h in hs:
            if h > prev:
                eng.append_jobs(slice_streams(streams, prev, h))
            eng.run(h)
            fol = fol or Follower(eng, 0, 1)
            fol.ran(h)
            st = fol.take_all(None, f"h {h}")
            prev = h
        got = fol.all_level1()
        assert got["head"][1, -1] == 600 and got["len"][1, -1] == 1
        assert st["rows_retired"] >= 4 * BATCH  # batches 0, 1 and 3 of the last cluster among them
        assert 0 < st["level1_rows_scanned"] <= BATCH * st["n_written"]  # the starved row's batch, per sample


def test_windows_across_batches_and_lengths_around_20():
    """Streams of 255, 256, 257 and 513 rows (Level1 windows across a batch), the hot five-node clusters
    whose lists pass 19, 20, 21 and 40 entries, and the list of 20 whose walk-back steps over a batch."""
    for arrays, streams, hs_n in ((*K.rounds_system(), 5), (*K.hot_five_nodes(), 4), (*walk_system(), 3)):
        top = int(streams.arrival.max()) + 1
        hs = horizons_for(streams, hs_n) + [top + 400, top + 1700]
        fol = follow_slices(arrays, streams, hs, 0, 1, (None, 50))
        got = fol.all_level1()
        if streams.n_jobs == 2400:
            K.assert_coverage(got)
        elif streams.n_jobs == 622:
            mult = got["len"] == 20
            assert mult.sum() > 100 and (got["small_time_s"][mult] == 3).any()
        else:
            assert np.diff(streams.job_off).tolist() == [255, 256, 257, 513] and (got["len"].max(axis=1) > 20).all()
            assert (got["head"][3][got["len"][3] > 0] >= BATCH).any()  # a list that begins behind the first batch


def test_256_node_cluster_that_deadlocks():
    """The Level1-pressure stream handed to delay_kernel: requests that fit no node starve in Level1 all
    along the stream, no batch is ever final, and the list outgrows 640 entries."""
    arrays, streams = level1_pressure(1, 1500)
    top = int(streams.arrival.max()) + 1  # the head moves on by one row a second: the queue outlasts the arrivals
    fol = follow_slices(arrays, streams, horizons_for(streams, 4) + [top + 400, top + 800, top + 1200], 0, 1)
    assert fol.stats[-1]["rows_retired"] == 0 and fol.all_level1()["len"].max() > 640


@pytest.mark.parametrize("load", ["hot", "light"])
def test_stream_survives_relayouts(load):
    """The 700-row segment off a multiple of 256: appends between the calls move every segment, the kept
    summaries and records with them, and the carried bounds stay what they were."""
    if load == "hot":
        arrays, streams = hot_clusters([100, 700, 300], 0x534547, nodes=[3, 4, 5])
    else:
        arrays, full = slice_workload(9, 3, 700)
        streams = truncate_streams(full, [100, 700, 300])
    top = int(streams.arrival.max()) + 1
    hs = list(range(9, top, max(1, top // 40)))
    relayouts = odd_starts = 0
    with engine("DELAY") as eng:
        eng.load_clusters(arrays)
        eng.submit_jobs(slice_streams(streams, 0, hs[0]))
        eng.run(hs[0])
        fol = Follower(eng, 0, 1)
        fol.ran(hs[0])
        fol.take_all()
        seg, prev = eng.segment_offsets(), hs[0]
        for h in hs[1:]:
            eng.append_jobs(slice_streams(streams, prev, h))
            now = eng.segment_offsets()
            relayouts += now.tolist() != seg.tolist()
            odd_starts += int(np.diff(eng.job_offsets())[1] >= 600 and int(now[1]) % BATCH != 0)
            seg = now
            eng.run(h)
            fol.ran(h)
            fol.take_all(None, f"h {h}")
            prev = h
        assert relayouts >= 3 and odd_starts >= 1
        if load == "light":
            assert min(st["rows_retired"] for st in fol.stats[len(fol.stats) // 2:]) >= 2 * BATCH
    with engine("DELAY") as eng:  # what the stream handed out, put together, is a batch run's series
        eng.load_clusters(arrays)
        eng.submit_jobs(streams)
        eng.run()
        K.assert_samples_equal(fol.all_level1(), eng.level1_series(0, 1, prev), "stream against the batch run")


def mid_session_main():
    """Run in a child process with MCS_SERIES_CHUNK=7: a stream opened mid-session with more than 256
    pending samples takes them in launches of seven, the bounds carried from launch to launch."""
    assert os.environ["MCS_SERIES_CHUNK"] == "7"
    arrays, streams = slice_workload(11, 3, 700)
    hs = horizons_for(streams, 6)
    with engine("DELAY") as eng:
        eng.load_clusters(arrays)
        prev = 0
        for h in hs[:3]:
            eng.append_jobs(slice_streams(streams, prev, h))
            eng.run(h)
            prev = h
        fol = Follower(eng, 2, 1)
        fol.ran(prev)
        first = fol.take(None, "catch-up")
        assert first["n_written"] == prev - 2 > 256 and first["pending"] == 0
        for h in hs[3:]:
            eng.append_jobs(slice_streams(streams, prev, h))
            eng.run(h)
            fol.ran(h)
            st = fol.take_all(300, f"h {h}")
            prev = h
        assert st["rows_retired"] >= 2 * BATCH and fol.all_level1()["len"].max() > 0
    print("mid-session ok")


def test_opened_mid_session_in_chunks_of_seven():
    env = dict(os.environ, MCS_SERIES_CHUNK="7", PYTHONPATH=os.pathsep.join(p for p in sys.path if p))
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "mid-session"], env=env, capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0 and "mid-session ok" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


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
            fol.ran(h)
            fol.take_all(None, f"fused h {h}")
        assert fol.all_level1()["len"].max() > 0


# ---- 2. trading sessions -------------------------------------------------------------------------------

@pytest.mark.parametrize("system", [("small", 4, 120), ("big", 8, 800)], ids=["small", "big"])
def test_trading_session_drain_append_run(system):
    """run(h), drain, append behind the drain, run, drain.  Below F* the samples stay servable after the
    append, where trade_session_level1_series refuses: those calls are compared with a batch engine's
    level1_series over all jobs.  Every contract logged so far equals the cursor's sample at its second."""
    arrays, streams, _ = seeded_workload(*system)
    cut = int(np.median(streams.arrival))
    first = trade_slice(streams, 0, cut)
    with session(arrays) as eng:
        eng.append_jobs(first)
        h1 = max(cut // 2, 20)
        eng.run(h1)
        fol = Follower(eng, 0, 1, trade=True)
        fol.ran(h1)
        fol.take_all(50 if system[0] == "small" else 997, f"h {h1}")
        eng.run()  # the drain
        td = eng.trade_session_info()["t_last"]
        fol.ran()
        assert fol.F == td + 1 > h1
        fol.take(400, "after the drain")
        rest = trade_slice(streams, cut, EVER)
        shift = td + 1 - int(rest.arrival.min())  # the first appended job arrives at the frontier itself
        rest = JobStreams((rest.arrival.astype(np.int64) + shift).astype(np.uint32), rest.dur, rest.cores, rest.mem,
                          rest.job_off)
        ref = TradeBatch(arrays, concat_streams(first, rest), period=1, oracle=False)
        eng.append_jobs(rest)
        assert "behind a drain" in raises(L.MCS_E_STATE, eng.trade_session_level1_series, 0, 5, 4)
        st = fol.take_all(None, "behind the drain", ref=ref)
        assert st["t_next"] == td + 1 and st["frontier"] == td + 1
        h = td + 700
        eng.run(h)
        fol.ran(h)
        fol.take_all(300, f"h {h}")
        eng.run()
        fol.ran()
        fol.take_all(None, "second drain")
        got = fol.all_level1()
        trades = eng.contracts()
        trades = trades[trades["t"] < got.shape[1]]
        seen = contracts_equal_samples(trades, lambda c, t: got[c, t])
        assert len(trades) > 0 and seen[0] + seen[1] > 0, seen
        eng.trade_stream_close()
    n = min(got.shape[1], int(ref.o["t_final"]))
    K.assert_samples_equal(got[:, :n], np.ascontiguousarray(ref.l1[:, :n]), "the stream against the batch run over all jobs")
    assert got["len"].max() > 0


def test_trading_stream_survives_an_escalation_replay():
    """The slot-pool escalation of test_session_escalation_replays (C5-DELAY, 256 -> 384 slots) replays the
    session from t = 0 inside a slice: the call after it rebuilds (rebuilt = 1), the carried bounds are
    dropped with everything else kept, and the bytes are the series call's."""
    arrays, streams, _ = seeded_workload("small", 64, 2000)
    with session(arrays) as b:
        b.submit_jobs(streams)
        b.run()
        tf = int(b.trade_stats()["t_final"])
    hs = [50 * (int(x) // 50) + 1 for x in np.linspace(0, tf, 12)[1:-1]]
    esc = after = 0
    with session(arrays) as eng:
        eng.append_jobs(trade_slice(streams, 0, hs[0]))
        eng.run(hs[0])
        fol, prev = Follower(eng, 0, 50, trade=True), hs[0]
        assert fol.take_all(None, "first")["rebuilt"] == 1
        for h in hs[1:]:
            eng.append_jobs(trade_slice(streams, prev, h))
            e = eng.run(h).escalations
            fol.ran(h)
            st = fol.take_all(None, f"h {h} after {e} replays")
            assert st["n_written"] > 0 and st["rebuilt"] == (1 if e else 0)
            after += bool(esc and not e)
            esc += e
            prev = h
        eng.append_jobs(trade_slice(streams, prev, EVER))
        e = eng.run().escalations
        fol.ran()
        st = fol.take_all(None, f"drained after {e} replays")
        assert st["rebuilt"] == (1 if e else 0)
        esc += e
        tl = eng.trade_session_info()["t_last"]
        eng.run(tl + 300)  # one more slice: the call after the rebuilding one carries its bounds again
        fol.ran(tl + 300)
        st = fol.take_all(None, "past the end")
        assert st["n_written"] > 0 and st["rebuilt"] == 0
        assert eng.trade_session_info()["restarts"] == esc >= 1
        assert fol.all_level1()["len"].max() > 0


# ---- 3. refusals, closing causes, the old calls --------------------------------------------------------

def buffers(c, m=8):
    out, wout = np.zeros((c, m), CLUSTER_SAMPLE_DTYPE), np.zeros((c, m), WAIT_SAMPLE_DTYPE)
    lout = np.zeros((c, m), LEVEL1_SAMPLE_DTYPE)
    return (out.ctypes.data_as(C.POINTER(L.mcs_cluster_sample)), wout.ctypes.data_as(C.POINTER(L.mcs_wait_sample)),
            lout.ctypes.data_as(C.POINTER(L.mcs_level1_sample)), (out, wout, lout))


def test_refusals_and_closing_causes():
    arrays, streams = hot_clusters([300, 257, 120], 0x4C4946, nodes=[3, 2, 4])
    h1, h2, h3 = horizons_for(streams, 3)
    po, pw, pl, _keep = buffers(3)
    old, new = L.lib().mcs_stream_next, L.lib().mcs_stream_next_level1
    with engine("FIFO") as eng:  # FIFO has no Level1
        eng.load_clusters(arrays)
        eng.append_jobs(slice_streams(streams, 0, h1))
        eng.run(h1)
        assert "Level1" in refused(lambda: eng.stream_open(0, 5, False, with_level1=True), L.MCS_E_INVALID)
        eng.stream_open(0, 5)  # and the refusal left no stream behind
        eng.stream_close()
    with engine("DELAY") as eng:
        eng.load_clusters(arrays)
        assert L.lib().mcs_stream_open_level1(eng._h, 0, 5, 1) == L.MCS_E_STATE  # no session
        eng.submit_jobs(slice_streams(streams, 0, h1))
        eng.run(h1)
        refused(lambda: eng.stream_open(0, 0, with_level1=True), L.MCS_E_INVALID)  # period 0
        fol = Follower(eng, 0, 5)
        fol.ran(h1)
        assert "open" in refused(lambda: eng.stream_open(0, 5, with_level1=True), L.MCS_E_STATE)
        assert new(eng._h, 8, po, pw, None, 3, None, None) == L.MCS_E_INVALID   # level1 NULL on a Level1 stream
        assert old(eng._h, 8, po, pw, 3, None) == L.MCS_E_INVALID                # the old next on a Level1 stream
        assert new(eng._h, 8, po, None, pl, 3, None, None) == L.MCS_E_INVALID   # opened with wait statistics
        assert new(eng._h, 8, None, pw, pl, 3, None, None) == L.MCS_E_INVALID
        assert new(eng._h, 0, po, pw, pl, 3, None, None) == L.MCS_E_INVALID
        assert new(eng._h, 8, po, pw, pl, 2, None, None) == L.MCS_E_INVALID
        fol.take(3)  # (none of these moved the stream)
        assert new(eng._h, 8, po, pw, pl, 3, None, None) == L.MCS_OK            # both stats may be NULL
        fol.t += 8 * 5
        fol.take_all()
        # a drain does not move the frontier; the first run after it closes the stream
        eng.append_jobs(slice_streams(streams, h1, h2))
        eng.run()
        assert fol.take()["n_written"] == 0
        eng.append_jobs(slice_streams(streams, max(h2, int(eng.cluster_stats()["t_end"].max())), EVER))
        eng.run(h3 + 1000)
        assert "drain" in refused(lambda: eng.stream_next(4), L.MCS_E_STATE)
        eng.stream_close()  # acknowledges the close
        fol = Follower(eng, 1, 3, with_wait=False)  # reopened without the wait statistics: records are kept all the same
        fol.ran(h3 + 1000)
        assert fol.take_all(500, "reopened")["n_written"] > 0 and fol.wait[0] is None
        assert new(eng._h, 8, po, pw, pl, 3, None, None) == L.MCS_E_INVALID     # opened without wait statistics
        eng.rewind()
        assert "mcs_rewind" in refused(lambda: eng.stream_next(4), L.MCS_E_STATE)
        eng.run(h2)
        fol = Follower(eng, 0, 5)
        fol.ran(h2)
        fol.take_all()
        eng.stream_close()  # mcs_stream_close closes either kind
        assert "no stream" in refused(lambda: eng.stream_next(4), L.MCS_E_STATE)
        for name, call in (("mcs_submit_jobs", lambda: eng.submit_jobs(streams)),
                           ("mcs_generate_jobs", lambda: eng.generate_jobs(GenParams(seed=1, max_dur_s=20), 50)),
                           ("mcs_load_clusters", lambda: eng.load_clusters(arrays))):
            eng.load_clusters(arrays)  # a fresh session
            eng.submit_jobs(slice_streams(streams, 0, h1))
            eng.run(h1)
            eng.stream_open(0, 5, with_level1=True)
            call()
            assert name in refused(lambda: eng.stream_next(4), L.MCS_E_STATE)
    # a run that fails closes it (the clock-range stream of test_a_failed_run_closes_the_stream)
    big = 0xFFFFFF00
    two = replicate(uniform_cluster(2, cores=4, memory=10), 2)
    s = JobStreams(np.array([big, big, 5, 6], np.uint32), np.array([0x200, 3, 4, 4], np.uint32),
                   np.array([4, 4, 1, 1], np.uint32), np.array([1, 1, 1, 1], np.uint32), np.array([0, 2, 4], np.uint64))
    with Engine(0, policy="DELAY", unchecked_horizon=1) as eng:
        eng.load_clusters(two)
        eng.submit_jobs(s)
        eng.run(20)
        fol = Follower(eng, 0, 1)
        fol.ran(20)
        assert fol.take_all()["n_written"] == 20
        rc, _ = eng.run_status(0xFFFFFFFE)
        assert rc == L.MCS_E_RANGE
        assert "failed" in refused(lambda: eng.stream_next(4), L.MCS_E_STATE)
        refused(lambda: eng.stream_open(0, 1, with_level1=True), L.MCS_E_STATE)


def test_trading_refusals():
    arrays, streams, _ = seeded_workload("small", 4, 120)
    h1 = int(np.median(streams.arrival))
    po, pw, pl, _keep = buffers(4)
    old, new = L.lib().mcs_trade_stream_next, L.lib().mcs_trade_stream_next_level1
    with session(arrays) as eng:
        assert "no trading session" in raises(L.MCS_E_STATE, eng.trade_stream_open, 0, 5, True, True)
        eng.submit_jobs(trade_slice(streams, 0, h1))
        eng.run(h1)
        assert "positive" in raises(L.MCS_E_INVALID, eng.trade_stream_open, 0, 0, True, True)
        raises(L.MCS_E_STATE, eng.stream_open, 0, 5, True, True)  # the plain cursor keeps refusing a trading session
        fol = Follower(eng, 0, 5, trade=True)
        assert new(eng._h, 8, po, pw, None, 4, None, None) == L.MCS_E_INVALID
        assert old(eng._h, 8, po, pw, 4, None) == L.MCS_E_INVALID
        assert new(eng._h, 8, po, None, pl, 4, None, None) == L.MCS_E_INVALID
        fol.take_all()
        eng.rewind()
        assert "mcs_rewind" in raises(L.MCS_E_STATE, eng.trade_stream_next, 4)
        eng.trade_stream_close()  # acknowledges the close; closes either kind
        eng.run(h1)
        eng.trade_stream_open(0, 5)  # the old open: a non-NULL level1 is refused, NULL serves it
        assert new(eng._h, 8, po, pw, pl, 4, None, None) == L.MCS_E_INVALID
        assert new(eng._h, 8, po, pw, None, 4, None, None) == L.MCS_OK
        eng.trade_stream_close()


def test_streams_opened_with_the_old_calls_did_not_move():
    """mcs_stream_open / mcs_stream_next return what the series calls return, as before; a non-NULL level1
    is refused on such a stream and mcs_stream_next_level1 with NULL serves it."""
    arrays, streams, hs = workload_small()
    po, pw, pl, (out, wout, _) = buffers(5, 16)
    new = L.lib().mcs_stream_next_level1
    with engine("DELAY") as eng:
        eng.load_clusters(arrays)
        eng.submit_jobs(slice_streams(streams, 0, hs[0]))
        prev, t = 0, 0
        for k, h in enumerate(hs[:4]):
            if k:
                eng.append_jobs(slice_streams(streams, prev, h))
            eng.run(h)
            if not k:
                eng.stream_open(0, 1)
            while t < h:
                assert new(eng._h, 16, po, pw, pl, 5, None, None) == L.MCS_E_INVALID
                if k % 2:
                    st = L.mcs_stream_stats()
                    assert new(eng._h, 16, po, pw, None, 5, C.byref(st), None) == L.MCS_OK
                    n, s, w = int(st.n_written), out[:, :st.n_written], wout[:, :st.n_written]
                else:
                    s, w, st = eng.stream_next(16)
                    n = st["n_written"]
                assert n == min(16, h - t)
                want_s, want_w, _ = eng.online_state_series(t, 1, n)
                assert_state_equal(np.ascontiguousarray(s), want_s, f"h {h} t {t}")
                assert_bits_equal(np.ascontiguousarray(w), want_w, f"h {h} t {t}")
                t += n
            prev = h


# ---- 4. cost follows the slice -------------------------------------------------------------------------

@pytest.mark.parametrize("seed", [7, 8])
def test_cost_follows_the_slice(seed):
    """40 equal slices of the arrival span, one call per slice at period 5 (4 clusters of 5 nodes, 8000
    jobs each, every 90th a whole node; W = 10).  A condition, not a timing: the rows the Level1 scans
    load equal, call by call, the count the rule gives on the oracle's run
    (tests/test_level1_stream_ref.py: from lo = 0, per sample the rows of [lo, hi(t)) in batches whose
    summary exceeds t, then lo = head or hi), and their sum stays within 3 R: the rule gives 1.59 R for
    both seeds, a per-call rescan of the rows held 20.8 R."""
    arrays, streams, hs, per_call, _ = cost_case(seed)
    R = int(streams.job_off[-1])
    assert sum(per_call) <= 3 * R
    got = []
    with engine("DELAY") as eng:
        eng.load_clusters(arrays)
        eng.append_jobs(slice_streams(streams, 0, hs[0]))
        eng.run(hs[0])
        fol = Follower(eng, 0, COST_PERIOD)
        prev = 0
        for k, h in enumerate(hs):
            if k:
                eng.append_jobs(slice_streams(streams, prev, h))
                eng.run(h)
            fol.ran(h)
            st = fol.take(None, f"slice {k}")
            assert st["pending"] == 0
            got.append(st["level1_rows_scanned"])
            prev = h
    print(f"seed {seed}: level1_rows_scanned {sum(got)} = {sum(got) / R:.2f} R; the rule {sum(per_call) / R:.2f} R")
    assert got == per_call
    assert sum(got) <= 3 * R


if __name__ == "__main__" and sys.argv[1:] == ["mid-session"]:
    mid_session_main()
