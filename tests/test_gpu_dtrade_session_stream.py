"""GPU parity of the cursor on a trading session's Start stream (mcs_trade_stream_open / next / close;
include/mcs_trade.h, DESIGN.md §14 "A cursor on a trading session's Start stream").

The reference of every sample is mcs_trade_session_state_series on the same engine at the same moment,
bit for bit (the wait double as uint64), which tests/test_gpu_dtrade_session_series.py pins to the batch
run over all jobs and to the oracle.  Where that call refuses (jobs appended behind a drain that no run
has seen; seconds between a later, lower horizon and the frontier) the reference is a batch engine over
all the jobs the session ever receives.  The stream keeps batch summaries, wait records, carried
constants and the list of the Foreign records that still hold, so every case takes its samples in many
calls, between appends, horizons, drains and replays.  After every call that writes samples
foreign_live and foreign_scanned are compared with the log read back on the host.
Run on a real MI355X: ``pytest -m gpu``."""
import ctypes as C

import numpy as np
import pytest

from kat_util import fuzz_workload, seeded_workload
from mcs_amd import CLUSTER_SAMPLE_DTYPE, WAIT_SAMPLE_DTYPE, Engine, GenParams, JobStreams
from mcs_amd import _lib as L
from test_gpu_dtrade_session import concat_streams, raises, session, slice_streams
from test_gpu_dtrade_session_series import EVER, Batch, workload_segments
from test_gpu_online_series import assert_state_equal
from test_gpu_wait_series import assert_bits_equal

pytestmark = pytest.mark.gpu

BATCH = 256  # kSeriesBatch: the rows of one retired unit


def n_below(t0, period, h):
    """samples t0 + k * period below h"""
    return (h - t0 + period - 1) // period if h > t0 else 0


def frontier_of(eng):
    """F* of a session whose runs all succeeded, from mcs_trade_session_info"""
    info = eng.trade_session_info()
    return max(info["t_horizon"], info["t_last"] + 1 if info["ticks_total"] else 0)


class Follower:
    """An open stream and what it must hand out next.  Every call is compared with
    trade_session_state_series, or with `ref` (a Batch at period 1) where that call refuses."""

    def __init__(self, eng, t0, period, with_wait=True):
        self.eng, self.t, self.period, self.with_wait = eng, t0, period, with_wait
        eng.trade_stream_open(t0, period, with_wait)
        self.F = frontier_of(eng)
        self.seen = 0  # Foreign-log records the stream has taken
        self.samples, self.wait, self.stats = [], [], []

    def ran(self, h=None):
        """after a successful run(h), or a drain (h None)"""
        info = self.eng.trade_session_info()
        self.F = max(self.F, h if h is not None else (info["t_last"] + 1 if info["ticks_total"] else 0))

    def take(self, max_samples=None, tag="", ref=None):
        eng, p = self.eng, self.period
        pend = n_below(self.t, p, self.F)
        m = max(pend, 1) if max_samples is None else max_samples
        s, w, st = eng.trade_stream_next(m)
        n = min(pend, m)
        assert st["frontier"] == self.F, f"{tag}: {st}"
        assert st["n_written"] == n and s.shape == (eng.num_clusters, n), f"{tag}: {st}"
        assert st["t_next"] == self.t + n * p and st["pending"] == pend - n, f"{tag}: {st}"
        assert (w is None) == (not self.with_wait)
        if n:
            assert st["t_first"] == self.t
            if ref is None:
                want_s, want_w, _ = eng.trade_session_state_series(self.t, p, n, with_wait=self.with_wait)
            else:
                assert ref.period == 1
                idx = self.t + p * np.arange(n)
                want_s, want_w = ref.state[:, idx], ref.wait[:, idx]
            assert_state_equal(s, want_s, f"{tag} state t0 {self.t} period {p} n {n}")
            if w is not None:
                assert_bits_equal(w, want_w, f"{tag} wait t0 {self.t} period {p} n {n}")
            self.samples.append(s)
            self.wait.append(w)
            # the Foreign list: exact, from the log on the host
            f = eng.foreign()
            if st["rebuilt"]:
                self.seen = 0
            live = int(((f["start"] != f["finish"]) & (f["finish"] > self.t)).sum())
            assert st["foreign_live"] == live, f"{tag}: {st}, {live} records still hold"
            assert st["foreign_scanned"] == len(f) - self.seen, f"{tag}: {st}, the log grew by {len(f) - self.seen}"
            self.seen = len(f)
        else:
            assert st["foreign_scanned"] == st["foreign_live"] == st["rebuilt"] == st["rows_scanned"] == 0, f"{tag}: {st}"
        if self.stats and not st["rebuilt"]:
            assert st["rows_retired"] >= self.stats[-1]["rows_retired"], f"{tag}: retired rows came back"
        self.stats.append(st)
        self.t += n * p
        return st

    def take_all(self, piece=None, tag="", ref=None):
        st = self.take(piece, tag, ref)
        while st["pending"]:
            st = self.take(piece, tag, ref)
        return st


def retirable(eng, t_next):
    """256 times the full batches whose rows are all decided with finish below t_next"""
    node, _, fin = eng.placements()
    off = eng.job_offsets()
    want = 0
    for c in range(len(off) - 1):
        nd, fn = node[int(off[c]):int(off[c + 1])], fin[int(off[c]):int(off[c + 1])].astype(np.int64)
        full = len(nd) // BATCH * BATCH
        want += BATCH * int(((nd[:full] >= 0) & (fn[:full] < t_next)).reshape(-1, BATCH).all(axis=1).sum())
    return want


# ---- the systems -------------------------------------------------------------------------------------
def workload_small(jobs=700, h0=53):
    """("small", 4, jobs) with cluster 3's jobs removed and every job of cluster 2 moved behind the first
    horizon h0 (none of them is submitted: all are appended)."""
    arrays, s, _ = seeded_workload("small", 4, jobs)
    parts, off = [[], [], [], []], [0]
    for k in range(3):
        sl = s.of(k)
        parts[0].append(s.arrival[sl].astype(np.int64) + (h0 + 2 if k == 2 else 0))
        for i, f in enumerate(("dur", "cores", "mem")):
            parts[i + 1].append(getattr(s, f)[sl])
        off.append(off[-1] + sl.stop - sl.start)
    off.append(off[-1])
    return arrays, JobStreams(*[np.concatenate(p).astype(np.uint32) for p in parts], np.array(off, np.uint64))


def horizons(streams, k, t0, period, lo=53, end=None):
    """k horizons up to `end` (default: 2000 s behind the last arrival): the first on a sample second,
    the second one below a sample, the third one above a sample"""
    top = int(streams.arrival.max()) + 1
    on = lambda h: t0 + period * ((h - t0) // period)
    hs = [int(x) for x in np.linspace(lo, end or top + 2000, k)]
    hs[0], hs[1], hs[2] = on(hs[0]), on(hs[1]) - 1, on(hs[2]) + 1
    hs = sorted(set(hs))
    assert (hs[0] - t0) % period == 0 and (hs[1] + 1 - t0) % period == 0 and (hs[2] - 1 - t0) % period == 0
    return hs


def follow(arrays, streams, hs, t0, period, with_wait=True, piece=None, open_at=0):
    """Submit the jobs below hs[0]; per horizon append the slice, run, take what is pending (every second
    slice in pieces: six of `piece` samples, then of 997).  The stream is opened after run number open_at."""
    with session(arrays) as eng:
        eng.submit_jobs(slice_streams(streams, 0, hs[0]))
        fol, prev = None, 0
        for k, h in enumerate(hs):
            if k:
                eng.append_jobs(slice_streams(streams, prev, h))
            eng.run(h)
            prev = h
            if fol is None and k >= open_at:
                fol = Follower(eng, t0, period, with_wait)
            if fol is not None:
                fol.ran(h)
                if k % 2 and piece:  # max_samples below pending: a few small pieces, then larger ones
                    for _ in range(6):
                        fol.take(piece, f"h {h}")
                fol.take_all(997 if k % 2 else None, f"h {h}")
        assert fol.t >= prev and fol.take()["n_written"] == 0  # nothing is handed out twice
        info = eng.trade_session_info()
        out = dict(fol=fol, foreign=eng.foreign(), vnodes=[len(eng.virtual_node_caps(c)) for c in range(arrays.n_clusters)],
                   restarts=info["restarts"], placements=eng.placements(), off=eng.job_offsets())
        eng.trade_stream_close()
    return out


# ---- 1. slices -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("system,t0,period", [("small", 0, 1), ("small", 0, 5), ("small", 3, 7), ("big", 0, 5),
                                              ("big", 3, 7), ("tiny", 0, 1)])
def test_slices(system, t0, period):
    """Periods 1, 5 and the off-phase cadence 3 + 7k; horizons on, below and above a sample second; every
    second slice taken in pieces of 7 samples (max_samples below pending).  "small": 4 clusters of 700
    jobs, one empty, one all appended; "big": ("big", 8, 800), three full batches and a tail per cluster,
    virtual nodes and Foreign jobs; "tiny": ("small", 4, 120), where no batch ever fills and nothing ever
    retires.  Both larger systems are overloaded (their queues drain at seconds 12426 and about 22000, long
    after the last arrival), so the horizons go on until everything has finished."""
    end = None
    if system == "big":
        arrays, streams, _ = seeded_workload("big", 8, 800)
        end = 13500
    elif system == "small":
        arrays, streams = workload_small()
        end = 24000
    else:
        arrays, streams, _ = seeded_workload("small", 4, 120)
    r = follow(arrays, streams, horizons(streams, 9, t0, period, end=end), t0, period, piece=7)
    fol = r["fol"]
    got = np.concatenate(fol.samples, axis=1)
    assert got["running"].max() > 0 and got["queued"].max() > 0
    assert np.concatenate(fol.wait, axis=1)["total_wait_ms"].max() > 0
    assert len(r["foreign"]) > 0 and sum(r["vnodes"]) > 0 and r["restarts"] == 0
    if system == "big":  # Foreign jobs with a window (the small systems' log may hold zero-length records only)
        assert max(st["foreign_live"] for st in fol.stats) > 0
        assert any(0 < st["foreign_live"] < len(r["foreign"]) for st in fol.stats)
    if system == "tiny":
        assert all(st["rows_retired"] == 0 for st in fol.stats)
    else:
        assert fol.stats[-1]["rows_retired"] >= 2 * BATCH
    if system == "small":
        assert (got[3]["queued"] == 0).all()  # the cluster without jobs (it may run Foreign jobs)


# ---- 2. virtual nodes ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big():
    arrays, streams, _ = seeded_workload("big", 8, 800)
    return Batch(arrays, streams, period=1, oracle=False)


@pytest.mark.parametrize("with_wait", [True, False])
def test_horizon_between_a_trade_and_its_first_job(big, with_wait):
    """("big", 8, 800): the horizons 121 and 12031 fall between a virtual node's trade (ticks 120 and
    12030) and its first job: the row exists and holds nothing.  The row count of clusters 0 and 4 grows
    between the calls, and with it the tile width the retire kernel's rows_scanned walk has to use."""
    arrays, streams, o = big.arrays, big.streams, big.o
    nphys = np.diff(arrays.node_off)
    with session(arrays) as eng:
        eng.submit_jobs(slice_streams(streams, 0, 2001))
        fol, prev, nv = None, 2001, []
        for h in (121, 1000, 12031, 12371):
            if h > prev:
                eng.append_jobs(slice_streams(streams, prev, h))
                prev = h
            eng.run(h)
            fol = fol or Follower(eng, 0, 1, with_wait)
            fol.ran(h)
            nv.append([len(eng.virtual_node_caps(c)) for c in range(arrays.n_clusters)])
            st = fol.take_all(None if h != 12031 else 4000, f"h {h}")
            assert st["rows_retired"] == retirable(eng, st["t_next"])
        assert nv[0][0] >= 1 and nv[2][4] > nv[1][4]  # a virtual row more than in the call before
        own = o["start"][streams.of(0)][o["node"][streams.of(0)] == nphys[0] + nv[0][0] - 1]
        assert len(own) and int(own.min()) >= 121  # ... that held nothing below the horizon
    got = np.concatenate(fol.samples, axis=1)
    assert_state_equal(got, big.state[:, :got.shape[1]], "the stream against the batch run")


def test_batch_kept_alive_by_a_job_on_a_virtual_node(big):
    """A full batch whose rows are all decided and whose end_max is attained only by a job on a virtual
    node, with the frontier between the batch's largest physical finish and that job's finish: the plain
    summary rule (k < N) would retire it while the job still holds its row."""
    arrays, streams, o = big.arrays, big.streams, big.o
    nphys = np.diff(arrays.node_off)
    hit = None
    for c in range(arrays.n_clusters):
        sl = streams.of(c)
        nd, st_, fn = o["node"][sl], o["start"][sl].astype(np.int64), o["finish"][sl].astype(np.int64)
        for b in range(len(nd) // BATCH):
            s = slice(b * BATCH, (b + 1) * BATCH)
            virt = nd[s] >= nphys[c]
            if (nd[s] < 0).any() or not virt.any() or virt.all():
                continue
            lo = int(max(fn[s][~virt].max(), st_[s].max())) + 1  # every row decided, every physical finish below
            if int(fn[s][virt].max()) > lo and hit is None:
                hit = (c, b, lo, int(fn[s][virt].max()))
    assert hit is not None, "no batch whose last finish is a virtual node's"
    c, b, F, vfin = hit
    with session(arrays) as eng:
        eng.append_jobs(streams)
        eng.run(F)
        fol = Follower(eng, 0, 1)
        fol.ran(F)
        st = fol.take_all(None, f"h {F}")
        assert st["t_next"] == F
        node, _, fin = eng.placements()
        sl = slice(int(streams.job_off[c]) + b * BATCH, int(streams.job_off[c]) + (b + 1) * BATCH)
        phys = node[sl] < nphys[c]
        assert (node[sl] >= 0).all() and fin[sl][phys].max() < F <= fin[sl][~phys].max() == vfin  # the case
        plain = BATCH * sum(1 for cc in range(arrays.n_clusters) for bb in range(800 // BATCH)
                            if all_below(node, fin, streams, nphys, cc, bb, F))
        assert st["rows_retired"] == retirable(eng, F) <= plain - BATCH  # the plain rule retires at least one more
        eng.run(vfin + 3)
        fol.ran(vfin + 3)
        fol.take_all(None, "past the virtual node's job")
    got = np.concatenate(fol.samples, axis=1)
    assert_state_equal(got, big.state[:, :got.shape[1]], "the stream against the batch run")


def all_below(node, fin, streams, nphys, c, b, F):
    """the plain summary rule: a batch retires when every finish on a physical node lies below F"""
    sl = slice(int(streams.job_off[c]) + b * BATCH, int(streams.job_off[c]) + (b + 1) * BATCH)
    nd, fn = node[sl], fin[sl].astype(np.int64)
    return bool((nd >= 0).all() and (fn[nd < nphys[c]] < F).all())


# ---- 4. opening mid-session and chunking ---------------------------------------------------------------
@pytest.mark.parametrize("chunk", [None, 100])
def test_opened_mid_session_catches_up(monkeypatch, chunk):
    """t0 = 2 far below the frontier: the first call walks the history once and hands out more than 256
    samples (several tiles, several rounds of wait_finish_kernel; with MCS_SERIES_CHUNK several launches);
    later calls no longer load the history."""
    arrays, streams = workload_small()
    hs = horizons(streams, 9, 2, 1, end=24000)
    if chunk:
        monkeypatch.setenv("MCS_SERIES_CHUNK", str(chunk))
    with session(arrays) as eng:
        prev = 0
        for h in hs[:5]:
            eng.append_jobs(slice_streams(streams, prev, h))
            eng.run(h)
            prev = h
        fol = Follower(eng, 2, 1)
        first = fol.take(None, "catch-up")
        assert first["n_written"] == prev - 2 > 256 and first["pending"] == 0 and first["rebuilt"] == 1
        assert first["rows_scanned"] == int(eng.job_offsets()[-1])  # the history, once
        assert first["foreign_scanned"] == len(eng.foreign())
        for h in hs[5:]:
            eng.append_jobs(slice_streams(streams, prev, h))
            eng.run(h)
            fol.ran(h)
            st = fol.take_all(300, f"h {h}")
            assert st["rebuilt"] == 0
            prev = h
        assert st["rows_retired"] >= 2 * BATCH
        assert st["rows_scanned"] < int(eng.job_offsets()[-1])


# ---- 5. relayouts --------------------------------------------------------------------------------------
def test_stream_survives_relayouts():
    """Clusters of 100, 700 and 300 jobs fed by many small appends: the 700-job segment starts off a
    multiple of 256 and moves at every relayout, the kept arrays with it.  What the stream handed out,
    put together, equals a fresh engine's batch run."""
    arrays, streams = workload_segments()
    ref = Batch(arrays, streams, period=1, oracle=False)
    top = int(streams.arrival.max()) + 1
    hs = list(range(11, top, max(5, top // 30))) + [ref.n]  # the last one: everything has finished
    assert ref.n > top
    relayouts = odd_starts = 0
    with session(arrays) as eng:
        eng.submit_jobs(slice_streams(streams, 0, hs[0]))
        eng.run(hs[0])
        fol = Follower(eng, 0, 1)
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
        # retired batches were carried through the relayouts: exactly the retirable ones at the end
        assert fol.stats[-1]["rows_retired"] == retirable(eng, fol.stats[-1]["t_next"]) >= BATCH
    got, wait = np.concatenate(fol.samples, axis=1), np.concatenate(fol.wait, axis=1)
    assert got.shape[1] == prev
    assert_state_equal(got, ref.state[:, :prev], "stream against the batch run")
    assert_bits_equal(wait, ref.wait[:, :prev], "stream against the batch run")


# ---- 6. drain ------------------------------------------------------------------------------------------
def test_drain_moves_the_frontier_and_keeps_the_stream_open():
    """Drain, next, append, next, run(h), next.  After the drain the frontier is t_last + 1; the jobs
    appended behind it change no sample below it, although trade_session_state_series refuses until the
    next run: those calls are compared with the batch engine over all jobs.  A horizon past the end of
    everything is covered, and a second drain."""
    arrays, streams, _ = seeded_workload("small", 8, 300)
    first = slice_streams(streams, 0, 600)
    with session(arrays) as eng:
        eng.append_jobs(first)
        eng.run(301)
        fol = Follower(eng, 0, 1)
        fol.ran(301)
        fol.take_all(50, "h 301")
        eng.run()  # the drain
        td = eng.trade_session_info()["t_last"]
        fol.ran()
        assert fol.F == td + 1 > 301
        fol.take(400, "after the drain")  # a part of what the drain decided
        rest = slice_streams(streams, 600, EVER)
        shift = td + 1 - int(rest.arrival.min())  # the first appended job arrives at the frontier itself
        rest = JobStreams((rest.arrival.astype(np.int64) + shift).astype(np.uint32), rest.dur, rest.cores, rest.mem,
                          rest.job_off)
        ref = Batch(arrays, concat_streams(first, rest), period=1, oracle=False)
        eng.append_jobs(rest)
        assert "behind a drain" in raises(L.MCS_E_STATE, eng.trade_session_state_series, 0, 5, 4)
        st = fol.take_all(None, "behind the drain", ref=ref)  # still servable, and final
        assert st["t_next"] == td + 1 and st["frontier"] == td + 1
        h = td + 700
        eng.run(h)  # the first run after a drain does not close the stream
        fol.ran(h)
        fol.take_all(300, f"h {h}")
        eng.run()
        fol.ran()
        fol.take_all(None, "second drain")
        tf = eng.trade_session_info()["t_last"]
        eng.run(tf + 900)  # a horizon past the end
        fol.ran(tf + 900)
        st = fol.take_all(None, "past the end")
        assert st["t_next"] == tf + 900
        assert st["rows_retired"] == retirable(eng, st["t_next"])
    got, wait = np.concatenate(fol.samples, axis=1), np.concatenate(fol.wait, axis=1)
    n = min(got.shape[1], int(ref.o["t_final"]))  # (past it the session ran trader rounds the batch run never reaches)
    assert_state_equal(got[:, :n], ref.state[:, :n], "the stream against the batch run over all jobs")
    assert_bits_equal(wait[:, :n], ref.wait[:, :n], "the stream against the batch run over all jobs")


# ---- 7. escalation -------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["slots", "vnodes"])
def test_stream_survives_an_escalation_replay(case):
    """The systems of test_session_escalation_replays: a slot-pool overflow (C5-DELAY, 256 -> 384 slots) and
    a virtual-node overflow (81 virtual nodes, above the initial 64) replay the session from t = 0 inside a
    slice.  The stream stays open and keeps t_next; the call after the replay rebuilds (rebuilt = 1, the
    whole log taken again), the one after it does not."""
    if case == "slots":
        arrays, streams, _ = seeded_workload("small", 64, 2000)
    else:
        arrays, streams = fuzz_workload("w16s", 2, n_clusters=8, J=1500, blocking=False)
    with session(arrays) as b:  # the span of the whole run
        b.submit_jobs(streams)
        b.run()
        tf = int(b.trade_stats()["t_final"])
    hs = [50 * (int(x) // 50) + 1 for x in np.linspace(0, tf, 12)[1:-1]]
    esc = after = 0
    with session(arrays) as eng:
        eng.append_jobs(slice_streams(streams, 0, hs[0]))
        eng.run(hs[0])
        fol, prev = Follower(eng, 0, 50), hs[0]
        assert fol.take_all(None, "first")["rebuilt"] == 1
        for h in hs[1:]:
            eng.append_jobs(slice_streams(streams, prev, h))
            e = eng.run(h).escalations
            fol.ran(h)
            st = fol.take_all(None, f"{case} h {h} after {e} replays")
            assert st["n_written"] > 0 and st["rebuilt"] == (1 if e else 0)
            if e:
                assert st["foreign_scanned"] == len(eng.foreign())
                assert st["rows_scanned"] == int(eng.job_offsets()[-1])  # the history, once more
            after += bool(esc and not e)
            esc += e
            prev = h
        eng.append_jobs(slice_streams(streams, prev, EVER))
        e = eng.run().escalations
        fol.ran()
        st = fol.take_all(None, f"{case} drained after {e} replays")
        assert st["rebuilt"] == (1 if e else 0)
        esc += e
        tl = eng.trade_session_info()["t_last"]
        eng.run(tl + 300)  # one more slice: the call after the rebuilding one does not rebuild
        fol.ran(tl + 300)
        st = fol.take_all(None, f"{case} past the end")
        assert st["n_written"] > 0 and st["rebuilt"] == 0
        after += bool(esc)
        assert eng.trade_session_info()["restarts"] == esc >= 1 and after >= 1
        assert fol.t > eng.trade_session_info()["t_last"] - 50


# ---- 8. closing and refusals ---------------------------------------------------------------------------
def test_closing_and_refusals(monkeypatch):
    arrays, streams = workload_small()
    h1, h2 = 400, 1200
    nxt = lambda e: (lambda: e.trade_stream_next(4))
    with session(arrays) as eng:
        assert "no trading session" in raises(L.MCS_E_STATE, eng.trade_stream_open, 0, 5)  # nothing submitted yet
        assert "mcs_stream_open" in raises(L.MCS_E_STATE, nxt(eng))
        raises(L.MCS_E_STATE, eng.trade_stream_close)
        eng.submit_jobs(slice_streams(streams, 0, h1))
        eng.run()  # a batch trading run is no session
        assert "mcs_stream_open" in raises(L.MCS_E_STATE, eng.trade_stream_open, 0, 5)
        eng.run(h1)
        assert "positive" in raises(L.MCS_E_INVALID, eng.trade_stream_open, 0, 0)
        msg = raises(L.MCS_E_STATE, eng.stream_open, 0, 5)  # the plain cursor keeps refusing a trading session
        assert "trading session" in msg and "mcs_trade_session_state_series" in msg
        fol = Follower(eng, 0, 5)
        assert "open" in raises(L.MCS_E_STATE, eng.trade_stream_open, 0, 5)  # one stream per engine
        raises(L.MCS_E_STATE, eng.stream_next, 4)  # the plain calls do not serve it
        raises(L.MCS_E_STATE, eng.stream_close)
        f = L.lib().mcs_trade_stream_next
        out, wout = np.zeros((5, 8), CLUSTER_SAMPLE_DTYPE), np.zeros((5, 8), WAIT_SAMPLE_DTYPE)
        po, pw = out.ctypes.data_as(C.POINTER(L.mcs_cluster_sample)), wout.ctypes.data_as(C.POINTER(L.mcs_wait_sample))
        assert f(eng._h, 8, po, pw, 2, None) == L.MCS_E_INVALID  # fewer clusters than the engine has
        assert f(eng._h, 8, po, pw, 5, None) == L.MCS_E_INVALID  # and more
        assert f(eng._h, 8, None, pw, 4, None) == L.MCS_E_INVALID
        assert f(eng._h, 0, po, pw, 4, None) == L.MCS_E_INVALID
        assert f(eng._h, 8, po, None, 4, None) == L.MCS_E_INVALID  # opened with wait statistics
        raises(L.MCS_E_INVALID, eng.run, h1 - 1)  # a decreasing horizon: nothing ran
        fol.take(3)  # (none of these moved the stream)
        assert f(eng._h, 8, po, pw, 4, None) == L.MCS_OK  # stats may be NULL
        fol.t += 8 * 5
        fol.take_all()
        eng.rewind()
        assert "mcs_rewind" in raises(L.MCS_E_STATE, nxt(eng))
        assert "mcs_rewind" in raises(L.MCS_E_STATE, nxt(eng))  # until it is reopened
        eng.trade_stream_close()  # acknowledges the close
        raises(L.MCS_E_STATE, eng.trade_stream_close)
        eng.run(h1)
        fol = Follower(eng, 1, 3, with_wait=False)
        assert fol.take_all(40)["n_written"] > 0 and fol.wait[0] is None
        assert f(eng._h, 8, po, pw, 4, None) == L.MCS_E_INVALID  # opened without wait statistics
        eng.trade_stream_close()
        assert "no stream" in raises(L.MCS_E_STATE, nxt(eng))
        for name, call in (("mcs_submit_jobs", lambda: eng.submit_jobs(slice_streams(streams, 0, h2))),
                           ("mcs_generate_jobs", lambda: eng.generate_jobs(GenParams(seed=1, max_dur_s=20), 50)),
                           ("mcs_load_clusters", lambda: eng.load_clusters(arrays))):
            eng.load_clusters(arrays)  # a fresh session
            eng.submit_jobs(slice_streams(streams, 0, h1))
            eng.run(h1)
            eng.trade_stream_open(0, 5)
            call()
            assert name in raises(L.MCS_E_STATE, nxt(eng))
    # a plain session: the trading calls refuse and name mcs_stream_open
    with Engine(0, policy="DELAY") as eng:
        eng.load_clusters(arrays)
        eng.submit_jobs(slice_streams(streams, 0, h1))
        eng.run(h1)
        assert "mcs_stream_open" in raises(L.MCS_E_STATE, eng.trade_stream_open, 0, 5)
        assert "mcs_stream_open" in raises(L.MCS_E_STATE, nxt(eng))
        eng.stream_open(0, 5)
        raises(L.MCS_E_STATE, eng.trade_stream_close)
        assert eng.stream_next(4)[2]["n_written"] == 4
    # a run that failed: capacity exhausted with a fixed slot pool
    big, bs, _ = seeded_workload("small", 64, 2000)
    with session(big, slot_pool=4) as eng:
        eng.append_jobs(slice_streams(bs, 0, 200))
        eng.run(200)
        fol = Follower(eng, 0, 5)
        fol.take_all()
        eng.append_jobs(slice_streams(bs, 200, EVER))
        raises(L.MCS_E_CAPACITY, eng.run)
        assert "failed" in raises(L.MCS_E_STATE, nxt(eng))
        assert "failed" in raises(L.MCS_E_STATE, eng.trade_stream_open, 0, 5)  # until the session starts over
    # the Foreign log dropped records
    monkeypatch.setenv("MCS_DTRADE_FOREIGN_LOG_CAP", "8")
    with session(arrays) as eng:
        eng.append_jobs(slice_streams(streams, 0, 60))
        eng.run(60)
        fol = Follower(eng, 0, 5)
        fol.take_all()
        eng.append_jobs(slice_streams(streams, 60, EVER))
        eng.run()
        assert eng.trade_stats()["flags"] & 0x10  # MCS_FLAG_LOG_OVERFLOW
        assert "MCS_FLAG_LOG_OVERFLOW" in raises(L.MCS_E_STATE, nxt(eng))
        assert "MCS_FLAG_LOG_OVERFLOW" in raises(L.MCS_E_STATE, eng.trade_stream_open, 0, 5)


# ---- 9. fuzz -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_fuzz_random_slices(seed):
    """fuzz_workload DELAY trading systems in random slices with random max_samples and cadences."""
    rng = np.random.default_rng(0x5452 + seed)
    arrays, streams = fuzz_workload("w16s", seed, n_clusters=int(rng.integers(2, 7)), J=int(rng.integers(300, 900)),
                                    blocking=False)
    top = int(streams.arrival.max()) + 1
    hs = sorted(set(int(x) for x in rng.integers(1, top + 1500, 12)))
    t0, period = int(rng.integers(0, 9)), int(rng.integers(1, 9))
    with session(arrays) as eng:
        prev, fol = 0, None
        for k, h in enumerate(hs):
            eng.append_jobs(slice_streams(streams, prev, h))
            e = eng.run(h).escalations
            prev = h
            if fol is None and k >= seed % 3:
                fol = Follower(eng, t0, period, with_wait=bool(seed % 2))
            if fol is not None:
                fol.ran(h)
                st = fol.take(int(rng.integers(1, 400)), f"seed {seed} h {h}")
                if rng.integers(0, 2):
                    fol.take_all(int(rng.integers(1, 400)), f"seed {seed} h {h}")
                assert not e or st["rebuilt"] or st["n_written"] == 0
        eng.append_jobs(slice_streams(streams, prev, EVER))
        eng.run()
        fol.ran()
        fol.take_all(int(rng.integers(100, 4000)), f"seed {seed} drained")
        assert fol.t > eng.trade_session_info()["t_last"] - period


# ---- 10. cost, as conditions ---------------------------------------------------------------------------
def cost_workload():
    """("small", 4, 4000) with every arrival multiplied by 5.  The seeded stream is overloaded: its last job
    arrives at second 23200 and the queue drains at 120099, so while jobs arrive no batch finishes and
    nothing can retire (a rescan and the cursor then load the same rows).  Stretched, the system keeps up
    (t_final 122449 against the last arrival at 116000) and still trades: 20 Foreign jobs, up to 11
    virtual nodes per cluster (the oracle's run; tests/test_dtrade_session_stream_ref.py)."""
    arrays, s, _ = seeded_workload("small", 4, 4000)
    return arrays, JobStreams((s.arrival.astype(np.int64) * 5).astype(np.uint32), s.dur, s.cores, s.mem, s.job_off)


def test_cost_follows_the_slice():
    """40 equal slices of the arrival span, one call per slice at period 5 with wait statistics.
    Conditions, not timings: rows_retired never shrinks and equals, after every call, 256 times the full
    batches whose rows are all decided with finish below t_next; rows_scanned of a call equals the rows in
    the batches that were not retired when the call began; and over the 40 calls the cursor loads at most
    half of what a rescan per call loads (the rows held at each call).  The CPU test computes the same
    sums by the rule alone over the oracle's run: 93674 of 333546 rows, 0.28."""
    arrays, streams = cost_workload()
    top = int(streams.arrival.max()) + 1
    hs = [top * k // 40 for k in range(1, 41)]
    scanned = held = 0
    with session(arrays) as eng:
        eng.append_jobs(slice_streams(streams, 0, hs[0]))
        eng.run(hs[0])
        fol = Follower(eng, 0, 5)
        prev, retired = 0, 0
        for k, h in enumerate(hs):
            if k:
                eng.append_jobs(slice_streams(streams, prev, h))
                eng.run(h)
                fol.ran(h)
            live_before = int(eng.job_offsets()[-1]) - retired  # the rows in batches not retired as the call begins
            st = fol.take(None, f"slice {k}")
            assert st["pending"] == 0
            assert st["rows_scanned"] == live_before, f"slice {k}: {st}, {live_before} rows in live batches"
            assert st["rows_retired"] == retirable(eng, st["t_next"]), f"slice {k}: {st}"
            scanned += st["rows_scanned"]
            held += int(eng.job_offsets()[-1])
            prev, retired = h, st["rows_retired"]
        assert eng.trade_session_info()["restarts"] == 0
        print(f"rows_scanned {scanned} of {held} rows held over the calls: {scanned / held:.3f}; "
              f"retired {st['rows_retired']} of {int(eng.job_offsets()[-1])}")
        assert 2 * scanned <= held
        assert st["rows_retired"] > int(eng.job_offsets()[-1]) // 2


# ---- 11. rows_scanned of a stream without wait statistics ----------------------------------------------
def dt_series_tile(nn):
    """dt_series_tile (csrc/mcs_internal.h): samples per tile of a cluster of nn rows"""
    ts = min(78 * 1024 // (16 * nn + 4 * (2 * 16 + 2)), 127)
    return (ts - 1) | 1


def test_rows_scanned_without_wait_statistics():
    """Without wait records a call loads the batches stream_prep_kernel read (those that were not final
    when the call began) and, of the final ones that are not retired, those a tile of dt_series_kernel
    hits: arrival_min <= t_last and end_max > t_first of a tile of dt_series_tile(N + nv) samples, nv the
    cluster's virtual rows in this call.  The 8-cluster fuzz system has clusters of 64 and 52 physical
    nodes and one that receives 81 virtual nodes (a replay inside the session: the model starts over
    with the stream), so the tile width is below 127 and changes between calls.  Counted on the host from
    the placements at every call, exactly."""
    arrays, streams = fuzz_workload("w16s", 2, n_clusters=8, J=1500, blocking=False)
    nphys = np.diff(arrays.node_off)
    with session(arrays) as b:
        b.submit_jobs(streams)
        b.run()
        tf = int(b.trade_stats()["t_final"])
    hs = [int(x) for x in np.linspace(0, tf + 40, 16)[1:]]
    period = 3
    final, retired, widths = {}, set(), set()
    with session(arrays) as eng:
        prev, fol = 0, None
        for h in hs:
            eng.append_jobs(slice_streams(streams, prev, h))
            eng.run(h)
            prev = h
            fol = fol or Follower(eng, 1, period, with_wait=False)
            fol.ran(h)
            t0 = fol.t
            st = fol.take(None, f"h {h}")
            n = st["n_written"]
            assert n > 0 and st["pending"] == 0
            if st["rebuilt"]:
                final, retired = {}, set()
            node, _, fin = eng.placements()
            arr, off = eng.read_jobs().arrival, eng.job_offsets()
            want = 0
            for c in range(arrays.n_clusters):
                lo, hi = int(off[c]), int(off[c + 1])
                nv = min(len(eng.virtual_node_caps(c)), 256)
                ts = dt_series_tile(int(nphys[c]) + nv)
                widths.add(ts)
                for bb in range((hi - lo + BATCH - 1) // BATCH):
                    if (c, bb) in retired:
                        continue
                    rows = slice(lo + bb * BATCH, min(lo + (bb + 1) * BATCH, hi))
                    nd, fn = node[rows], fin[rows].astype(np.int64)
                    amin = int(arr[rows].min())
                    emax = int(np.where(nd >= 0, fn, 0xFFFFFFFF).max())
                    loaded = (c, bb) not in final  # stream_prep_kernel read it
                    for k0 in range(0, n, ts):
                        tsa = min(ts, n - k0)
                        t_first = t0 + k0 * period
                        loaded |= amin <= t_first + (tsa - 1) * period and emax > t_first
                    want += (rows.stop - rows.start) if loaded else 0
                    if rows.stop - rows.start == BATCH and (nd >= 0).all() and (fn != 0xFFFFFFFF).all():
                        final[(c, bb)] = True
                        if emax < st["t_next"]:
                            retired.add((c, bb))
            assert st["rows_scanned"] == want, f"h {h}: {st}, {want} rows by the rule"
            assert st["rows_retired"] == BATCH * len(retired)
        assert eng.trade_session_info()["restarts"] >= 1
    assert len(widths) >= 3 and min(widths) < 127, widths
    assert len(retired) >= 8
