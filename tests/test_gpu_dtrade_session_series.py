"""GPU parity of mcs_trade_session_state_series and mcs_trade_session_level1_series (include/mcs_trade.h,
DESIGN.md §14 "The Start stream of a trading session"): the ClusterState series, the wait statistics,
the record at t0_s and the Level1 samples of a trading session, read between horizons
(csrc/mcs_state.hip: the SEG instantiations of dt_state_kernel / dt_series_kernel and
dt_foreign_live_kernel; the SEG wait_* and level1_* kernels).

Every comparison is bit for bit (the wait double as uint64; two NaNs are equal).  A
sample below a finite horizon is compared with both
  - a second engine that runs ALL the jobs the session ever receives as one batch and answers through
    mcs_dtrade_state_series / mcs_level1_series, and
  - tests/dtrade_state_ref.py over the oracle's run of all jobs (the batch engine's run is first
    asserted equal to the oracle's),
although the session has not seen the later jobs, Foreign records and virtual nodes yet
(tests/test_dtrade_session_series_ref.py pins that argument on the oracle alone).  The one exception is
the C5-DELAY escalation case, whose docstring states what it compares instead.  Run on a real MI355X."""
import os
import subprocess
import sys

import numpy as np
import pytest

import dtrade_state_ref as D
import oracle_ref as O
from kat_util import fuzz_workload, seeded_workload
from mcs_amd import Engine, JobStreams
from mcs_amd import _lib as L
from test_gpu_dtrade_session import concat_streams, one_job, raises, session, slice_streams
from test_gpu_dtrade_state import assert_run_is_the_oracles, assert_samples_equal
from test_gpu_online_series import assert_state_equal
from test_gpu_wait_series import assert_bits_equal

pytestmark = pytest.mark.gpu
EVER = 1 << 32


class Batch:
    """All jobs run as one batch on an engine of its own, and the oracle's run of them: the samples at
    the seconds k * period, k < n, from both.  Computed once per workload and never modified."""

    def __init__(self, arrays, streams, period=1, oracle_every=1, oracle=True, **cfg):
        """oracle=False (a system whose oracle run takes half a minute on the host): the reference is
        fed from the batch engine's own readers, which dtrade_state_ref.py is written for as well."""
        self.arrays, self.streams, self.period = arrays, streams, period
        with session(arrays, **cfg) as eng:
            eng.submit_jobs(streams)
            st = eng.run()
            assert not st.online
            if oracle:
                o = O.dtrade_run(arrays, streams)
                assert_run_is_the_oracles(eng, arrays, o)
            else:
                node, start, fin = eng.placements()
                f = eng.foreign()
                o = dict(node=node, start=start, finish=fin, foreign=f, n_foreign=len(f),
                         vnodes=[eng.virtual_node_caps(c) for c in range(arrays.n_clusters)],
                         t_final=eng.trade_stats()["t_final"])
            self.o = o
            last = max(int(o["t_final"]), int(o["foreign"]["finish"].max()) if o["n_foreign"] else 0)
            self.n = (last + 6 + period - 1) // period
            self.state, self.wait, self.first0 = eng.dtrade_state_series(0, period, self.n)
            self.l1 = eng.level1_series(0, period, self.n)
        # the oracle's samples k * period * oracle_every
        self.oracle_every = oracle_every
        self.ref = D.series_ref(arrays, streams, o, 0, period * oracle_every, (self.n + oracle_every - 1) // oracle_every)
        assert_samples_equal(self.state[:, ::oracle_every], self.ref, "the batch engine against the oracle's record")

    def first(self, k):
        out = self.first0.copy()
        for f in ("cores_utilization", "memory_utilization", "running"):
            out[f] = self.state[f][:, k]
        out["t_s"] = k * self.period
        return out

    def check(self, eng, t0, period, n, tag=""):
        """The session's samples t0 + k * period, k < n (seconds on this reference's grid), equal the
        batch engine's and the oracle's; returns (samples, wait, first, level1)."""
        assert t0 % self.period == 0 and period % self.period == 0
        idx = (t0 + period * np.arange(n)) // self.period
        samples, wait, first = eng.trade_session_state_series(t0, period, n)
        l1 = eng.trade_session_level1_series(t0, period, n)
        assert_state_equal(samples, self.state[:, idx], f"{tag} state t0 {t0} period {period}")
        assert_bits_equal(wait, self.wait[:, idx], f"{tag} wait t0 {t0} period {period}")
        assert_state_equal(first, self.first(idx[0]), f"{tag} first t0 {t0}")
        assert l1.tobytes() == self.l1[:, idx].tobytes(), f"{tag} level1 t0 {t0} period {period}"
        on = idx % self.oracle_every == 0
        assert_samples_equal(samples[:, on], self.ref[:, idx[on] // self.oracle_every], f"{tag} oracle t0 {t0}")
        return samples, wait, first, l1


def past_the_frontier(eng, t0, period, n, h):
    """a call whose last sample lies at h or later is MCS_E_INVALID, and the message names h"""
    for fn in (eng.trade_session_state_series, eng.trade_session_level1_series):
        assert str(h) in raises(L.MCS_E_INVALID, fn, t0, period, n)


def run_slices(ref, hs, period=1, submitted_below=None, **cfg):
    """Submit the jobs below hs[0] (or submitted_below), then per horizon append [h_prev, h), run(h) and
    compare every sample below h; finally append the rest, drain and compare every sample of the
    reference.  Returns what was non-zero."""
    arrays, streams = ref.arrays, ref.streams
    seen = dict(running=0, queued=0, undecided=0, total_wait_ms=0, level1=0)
    with session(arrays, **cfg) as eng:
        cut = hs[0] if submitted_below is None else submitted_below
        eng.submit_jobs(slice_streams(streams, 0, cut))
        prev = 0
        for h in hs:
            if h > cut:
                eng.append_jobs(slice_streams(streams, max(prev, cut), h))
            st = eng.run(h)
            assert st.online and st.t_horizon == h
            n = (h + period - 1) // period  # the samples 0, period, ... below h
            s, w, _, l1 = ref.check(eng, 0, period, n, f"h {h}")
            past_the_frontier(eng, 0, period, n + 1, h)  # one sample more lies at or past h
            node, start, _ = eng.placements()
            arr = eng.read_jobs().arrival
            seen["undecided"] += int(((node == L.MCS_NODE_UNPLACED) & (start == L.MCS_TIME_NONE) & (arr < h)).sum())
            seen["running"] += int(s["running"].sum())
            seen["queued"] += int(s["queued"].sum())
            seen["total_wait_ms"] += int(w["total_wait_ms"].sum())
            seen["level1"] += int(l1["len"].sum())
            prev = h
        eng.append_jobs(slice_streams(streams, max(prev, cut), EVER))
        eng.run()
        assert eng.trade_session_info()["drained"] == 1
        ref.check(eng, 0, period, ref.n, "drained")  # past t_final: the continued Go loop
        if period == 1:
            ref.check(eng, 3, 7, (ref.n - 3) // 7, "drained")
    return seen


# ---- 1. ("small", 4, 120) in slices --------------------------------------------------------------------
def workload_small():
    """("small", 4, 120) with cluster 3's jobs removed and every job of cluster 2 moved behind the first
    horizon (none of them is submitted: all are appended)."""
    arrays, s, _ = seeded_workload("small", 4, 120)
    hs = [53, 400, 3281]
    parts, off = [[], [], [], []], [0]
    for k in range(3):
        sl = s.of(k)
        parts[0].append(s.arrival[sl].astype(np.int64) + (hs[0] + 2 if k == 2 else 0))
        for i, f in enumerate(("dur", "cores", "mem")):
            parts[i + 1].append(getattr(s, f)[sl])
        off.append(off[-1] + sl.stop - sl.start)
    off.append(off[-1])
    return arrays, JobStreams(*[np.concatenate(p).astype(np.uint32) for p in parts], np.array(off, np.uint64)), hs


@pytest.fixture(scope="module")
def small():
    arrays, streams, hs = workload_small()
    ref = Batch(arrays, streams)
    o = ref.o
    assert o["n_foreign"] >= 10 and sum(len(v) for v in o["vnodes"]) >= 4
    f = o["foreign"]
    assert ((f["c"] >= 2 ** 32) | (f["m"] >= 2 ** 32)).any()  # a wrapped Go uint in the log
    # a trade, and Foreign jobs, at or past the last finite horizon: absent in the session below it
    assert (f["start"] >= hs[-1]).any() and (f["start"] == hs[-1] - 1).any()
    assert ((ref.state["cores_utilization"] < 0) | (ref.state["memory_utilization"] < 0)).any()
    return ref, hs


def test_slices_equal_the_batch_series_and_the_oracle(small):
    ref, hs = small
    streams = ref.streams
    assert streams.job_off[4] == streams.job_off[3] and int(streams.arrival[streams.of(2)].min()) >= hs[0]
    seen = run_slices(ref, hs)
    assert all(v > 0 for v in seen.values()), seen
    assert (ref.state[3]["queued"] == 0).all() and (ref.l1[3]["len"] == 0).all()


# ---- 2. ("big", 8, 800) at the reference cadence -------------------------------------------------------
def test_big_system_at_the_reference_cadence():
    """Foreign values past 2^32, hundreds of own jobs on virtual rows and Foreign jobs on a responder's
    virtual rows.  The horizons 121 and 12031 fall between a virtual node's trade (ticks 120 and 12030)
    and its first job (121 and 12031): the row exists in the session and holds nothing yet.  12371
    follows the Foreign jobs of tick 12370, one of them on a virtual row."""
    arrays, streams, _ = seeded_workload("big", 8, 800)
    ref = Batch(arrays, streams, period=5)
    o, nphys = ref.o, np.diff(arrays.node_off)
    f, won = o["foreign"], o["trades"][o["trades"]["winner"] >= 0]
    for t, r in ((120, 0), (12030, 4)):
        k = int(((won["requester"] == r) & (won["t"] < t)).sum())  # the virtual node of requester r's trade at t
        assert ((won["t"] == t) & (won["requester"] == r)).any()
        own = o["start"][streams.of(r)][o["node"][streams.of(r)] == nphys[r] + k]
        assert len(own) and int(own.min()) == t + 1
    assert ((f["node"] >= nphys[f["responder"]]) & (f["start"] < 12370) & (f["finish"] > 12350)).any()
    assert (f["start"] == 12370).any() and ((f["c"] >= 2 ** 32) | (f["m"] >= 2 ** 32)).sum() >= 2
    seen = run_slices(ref, [121, 12031, 12371], period=5, submitted_below=2001)
    assert all(v > 0 for v in seen.values()), seen


# ---- 3. the horizon on a tile's edges, and chunks ------------------------------------------------------
def test_frontier_on_tile_edges_and_chunks(small, monkeypatch):
    """NN <= 8 rows per cluster: dt_series_tile = 127 samples.  With h = 400 the last decided sample
    h - 1 is the last sample of a tile (n_samples 127 from h - 127) and the first of the next one
    (n_samples 128 from h - 128); one more sample is past the frontier.  A chunked call returns the
    same bytes."""
    ref, _ = small
    h = 400
    with session(ref.arrays) as eng:
        eng.submit_jobs(slice_streams(ref.streams, 0, h))
        eng.run(h)
        assert max(len(eng.virtual_node_caps(c)) for c in range(4)) + 5 <= 8
        for n in (127, 128):
            ref.check(eng, h - n, 1, n, f"n {n}")
            past_the_frontier(eng, h - n, 1, n + 1, h)
            past_the_frontier(eng, h - n + 1, 1, n, h)
        whole = ref.check(eng, 0, 1, h, "whole")
        monkeypatch.setenv("MCS_SERIES_CHUNK", "131")  # splits the samples, and not on a tile edge
        parts = ref.check(eng, 0, 1, h, "chunked")
        for a, b in zip(whole, parts):
            assert a.tobytes() == b.tobytes()
        monkeypatch.delenv("MCS_SERIES_CHUNK")
        past_the_frontier(eng, h, 1, 1, h)  # a sample at exactly h


# ---- 4. segments with slack ----------------------------------------------------------------------------
def workload_segments():
    """Three small clusters with 100, 700 and 300 jobs (prefixes of seeded streams)."""
    arrays, s, _ = seeded_workload("small", 3, 700)
    counts = [100, 700, 300]
    parts, off = [[], [], [], []], [0]
    for k, cnt in enumerate(counts):
        sl = slice(s.of(k).start, s.of(k).start + cnt)
        for i, f in enumerate(("arrival", "dur", "cores", "mem")):
            parts[i].append(getattr(s, f)[sl])
        off.append(off[-1] + cnt)
    return arrays, JobStreams(*[np.concatenate(p).astype(np.uint32) for p in parts], np.array(off, np.uint64))


def test_series_over_segments_with_slack():
    """A 700-job cluster behind a small one, fed by many small appends: its segment starts off a
    multiple of 256, holds several summary batches and moves at every relayout (both read from the
    engine: segment_offsets).  Each slice's series equals the batch run's and the oracle's record (period
    5), agrees with the previous slice's on their common samples, and a
    fresh session that receives the same jobs in one append returns the same bytes (nothing stale)."""
    arrays, streams = workload_segments()
    ref = Batch(arrays, streams, period=5)
    assert ref.o["n_foreign"] > 0 and sum(len(v) for v in ref.o["vnodes"]) > 0
    top = int(streams.arrival.max()) + 1
    hs = [5 * (x // 5) + 1 for x in range(11, top, max(5, top // 30))]
    relayouts = odd_starts = 0
    with session(arrays) as eng:
        eng.submit_jobs(slice_streams(streams, 0, hs[0]))
        eng.run(hs[0])
        seg = eng.segment_offsets()
        assert seg.tolist() == eng.job_offsets().tolist()  # submitted streams have no slack
        before = ref.check(eng, 0, 5, (hs[0] + 4) // 5, f"h {hs[0]}")[0]
        prev = hs[0]
        for h in hs[1:]:
            eng.append_jobs(slice_streams(streams, prev, h))
            now, counts = eng.segment_offsets(), np.diff(eng.job_offsets())
            assert (np.diff(now) >= counts).all()
            moved = now.tolist() != seg.tolist()
            if moved:  # the relayout alone changes no sample: the series before the next run
                mid = eng.trade_session_state_series(0, 5, before.shape[1])[0]
                assert mid.tobytes() == before.tobytes(), f"h {h}: the relayout changed samples"
            relayouts += moved
            seg = now
            eng.run(h)
            after = ref.check(eng, 0, 5, (h + 4) // 5, f"h {h}")[0]
            assert after[:, :before.shape[1]].tobytes() == before.tobytes(), f"h {h}: samples below {prev} changed"
            if counts[1] >= 600 and int(seg[1]) % 256 != 0:
                odd_starts += 1
            before, prev = after, h
        last = [x.tobytes() for x in ref.check(eng, 0, 5, (prev + 4) // 5, "last")]
        assert (np.diff(seg) > np.diff(eng.job_offsets())).any()  # slack: the segments are not dense
    assert relayouts >= 3 and odd_starts >= 1
    with session(arrays) as fresh:
        fresh.append_jobs(slice_streams(streams, 0, prev))
        fresh.run(prev)
        again = [x.tobytes() for x in ref.check(fresh, 0, 5, (prev + 4) // 5, "fresh")]
    assert again == last


# ---- 5. escalation inside a slice ----------------------------------------------------------------------
@pytest.mark.parametrize("case", ["slots", "vnodes"])
def test_series_after_an_escalation_replay(case):
    """The systems of tests/test_gpu_dtrade_session.py's escalation test: a slot-pool overflow (C5-DELAY,
    256 -> 384 slots) and a virtual-node overflow (81 virtual nodes, above the initial 64) inside a
    session of ten slices.  After each replay from t = 0 the series below the horizon is the batch
    run's, at period 50.  The virtual-node case compares every sample with dtrade_state_ref.py over the
    oracle's run.  The oracle's run of C5-DELAY (64 clusters x 55000 s) takes half a minute on the host, so
    there the reference reads the batch engine's own placements and logs (tests/test_gpu_dtrade_session.py
    compares those with the oracle) and is walked at every 4th sample; every sample is compared with the
    batch engine."""
    if case == "slots":
        arrays, streams, _ = seeded_workload("small", 64, 2000)
    else:
        arrays, streams = fuzz_workload("w16s", 2, n_clusters=8, J=1500, blocking=False)
    ref = Batch(arrays, streams, period=50, oracle_every=4 if case == "slots" else 1, oracle=case != "slots")
    hs = [50 * (int(x) // 50) + 1 for x in np.linspace(0, int(ref.o["t_final"]), 12)[1:-1]]
    esc = 0
    with session(arrays) as eng:
        prev = 0
        for h in hs:
            eng.append_jobs(slice_streams(streams, prev, h))
            e = eng.run(h).escalations
            esc += e
            if e or h in (hs[0], hs[-1]):
                ref.check(eng, 0, 50, (h + 49) // 50, f"{case} h {h} after {e} replays")
            prev = h
        eng.append_jobs(slice_streams(streams, prev, EVER))
        esc += eng.run().escalations
        ref.check(eng, 0, 50, ref.n, f"{case} drained")
        assert eng.trade_session_info()["restarts"] == esc >= 1


# ---- 6. restarts: rows an earlier pass wrote -----------------------------------------------------------
@pytest.mark.parametrize("how", ["rewind", "after_batch"])
def test_series_after_a_restart_with_new_jobs(how):
    """mcs_rewind, and a session begun after a batch trading run: both restart over rows an earlier pass
    decided, then receive jobs whose arrivals lie below the next horizon and change later decisions.  A
    stale row would read as decided: every sample below the horizon equals the batch run over all jobs."""
    arrays, streams = fuzz_workload("w16s", 2, n_clusters=4, J=900, blocking=False)
    keep = np.ones(len(streams.arrival), bool)
    keep[::7] = False  # every seventh job comes late: appended after the restart

    def part(m):
        off = np.concatenate([[0], np.cumsum([int(m[streams.of(k)].sum()) for k in range(arrays.n_clusters)])])
        return JobStreams(streams.arrival[m], streams.dur[m], streams.cores[m], streams.mem[m], off.astype(np.uint64))

    base, late = part(keep), part(~keep)
    lo = int(base.arrival.max()) + 1  # the late jobs, moved behind the base streams (appends continue a stream)
    late = JobStreams((late.arrival.astype(np.int64) // 4 + lo).astype(np.uint32), late.dur, late.cores, late.mem,
                      late.job_off)
    everything = concat_streams(base, late)
    ref = Batch(arrays, everything, period=5)
    h = 5 * ((lo + 1000) // 5) + 1
    with session(arrays) as eng:
        eng.submit_jobs(base)
        if how == "rewind":
            eng.run(4001)
            eng.run()
            eng.rewind()
            assert "mcs_rewind" in raises(L.MCS_E_STATE, eng.trade_session_state_series, 0, 5, 4)
            assert "mcs_rewind" in raises(L.MCS_E_STATE, eng.trade_session_level1_series, 0, 5, 4)
        else:
            st = eng.run()
            assert not st.online
        eng.append_jobs(late)
        eng.run(h)
        node, _, _ = eng.placements()
        assert (node == L.MCS_NODE_UNPLACED).any()
        ref.check(eng, 0, 5, (h + 4) // 5, how)
        eng.run()
        ref.check(eng, 0, 5, ref.n, how + " drained")


# ---- 7. a horizon past the end, then more jobs ---------------------------------------------------------
def test_horizon_past_the_end_then_append():
    """Drain, then mcs_run(t_final + 600): sample ticks and trader rounds the batch run over the jobs
    held never reaches (the statement's caveat).  Jobs appended then continue the system: every second
    below the new horizon, and after the drain, equals the batch run over all jobs."""
    arrays, streams, _ = seeded_workload("small", 8, 300)
    first = slice_streams(streams, 0, 600)
    with session(arrays) as eng:
        eng.append_jobs(first)
        eng.run()
        tf = eng.trade_stats()["t_final"]
        eng.run(tf + 600)
        assert eng.trade_session_info()["t_last"] > tf
        rest = slice_streams(streams, 600, EVER)
        shift = tf + 600 + 3 - int(rest.arrival.min())
        rest = JobStreams((rest.arrival.astype(np.int64) + shift).astype(np.uint32), rest.dur, rest.cores, rest.mem,
                          rest.job_off)
        everything = concat_streams(first, rest)
        ref = Batch(arrays, everything, period=5)
        ref.check(eng, 0, 5, (tf + 600 + 4) // 5, "past the end")  # before the new jobs: final all the same
        eng.append_jobs(rest)
        h = 5 * ((tf + 600 + 3 + 400) // 5) + 1
        eng.run(h)
        ref.check(eng, 0, 5, (h + 4) // 5, f"h {h}")
        eng.run()
        ref.check(eng, 0, 5, ref.n, "drained")


# ---- 8. the Foreign pre-pass changes no byte -----------------------------------------------------------
CHILD = r"""
import hashlib, sys
import numpy as np
from kat_util import seeded_workload
from mcs_amd import Engine
arrays, streams, _ = seeded_workload("big", 8, 800)
eng = Engine(0, policy="DELAY", trader=True)
eng.load_clusters(arrays)
eng.append_jobs(streams)
h = hashlib.sha256()
for hor in (12371, None):
    eng.run(hor) if hor else eng.run()
    for t0, period, n in ((0, 5, 2474), (12300, 1, 70), (0, 1, 300)) if hor else ((0, 5, 2600), (12000, 1, 1000)):
        for a in eng.trade_session_state_series(t0, period, n):
            h.update(a.tobytes())
assert len(eng.foreign()) > 50
print("SHA", h.hexdigest())
"""


def test_foreign_filter_switch_returns_the_same_bytes():
    """MCS_DT_FOREIGN_FILTER=0 (the log scanned as it is), =1 (dt_foreign_live_kernel's list in every
    call) and the default (the list where the call is long enough for it to pay: the 2474-sample calls
    here, 20 tiles) on ("big", 8, 800): a child process per setting, since the switch is read at
    mcs_create."""
    got = {}
    for v in ("0", "1", None):
        env = dict(os.environ, PYTHONPATH=os.pathsep.join(p for p in sys.path if p))
        env.pop("MCS_DT_FOREIGN_FILTER", None)
        if v is not None:
            env["MCS_DT_FOREIGN_FILTER"] = v
        r = subprocess.run([sys.executable, "-c", CHILD], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        got[v] = [ln for ln in r.stdout.splitlines() if ln.startswith("SHA")]
    assert len(got["0"]) == 1 and got["0"] == got["1"] == got[None]


# ---- 9. the batch call did not move; the old calls still refuse ----------------------------------------
def test_batch_call_and_old_refusals_are_what_they_were(small):
    ref, _ = small
    arrays, streams = ref.arrays, ref.streams
    # (Batch has compared mcs_dtrade_state_series after a batch run with dtrade_state_ref.py at every second)
    assert ref.oracle_every == 1 and ref.period == 1
    with session(arrays) as eng:
        eng.submit_jobs(slice_streams(streams, 0, 600))
        eng.run(101)
        for fn, args in ((eng.dtrade_state_series, (0, 5, 4)), (eng.level1_series, (0, 5, 4)),
                         (eng.level1_at, (0, 50)), (eng.online_state_series, (0, 5, 4)),
                         (eng.online_level1_series, (0, 5, 4)), (eng.stream_open, (0, 5)),
                         (eng.cluster_states, (50,)), (eng.cluster_state_series, (0, 5, 4)),
                         (eng.wait_time_series, (0, 5, 4))):
            msg = raises(L.MCS_E_STATE, fn, *args)
            assert "trading session" in msg and "mcs_trade_session_state_series" in msg, fn.__name__


# ---- 10. refusals --------------------------------------------------------------------------------------
def both(eng):
    return (eng.trade_session_state_series, eng.trade_session_level1_series)


def test_refusals(small, monkeypatch):
    ref, _ = small
    arrays, streams = ref.arrays, ref.streams
    # no trading session: before a run, after a batch trading run, in a plain session
    with session(arrays) as eng:
        eng.submit_jobs(streams)
        for fn in both(eng):
            assert "no trading session" in raises(L.MCS_E_STATE, fn, 0, 5, 4)
        eng.run()
        for fn in both(eng):
            assert "mcs_dtrade_state_series" in raises(L.MCS_E_STATE, fn, 0, 5, 4)
    with Engine(0, policy="DELAY") as eng:
        eng.load_clusters(arrays)
        eng.submit_jobs(streams)
        eng.run(101)
        for fn in both(eng):
            assert "mcs_online_state_series" in raises(L.MCS_E_STATE, fn, 0, 5, 4)
    with session(arrays, t_max_s=5000) as eng:
        eng.submit_jobs(slice_streams(streams, 0, 600))
        eng.rewind()  # a session at t = 0 that no run has followed
        for fn in both(eng):
            assert "run first" in raises(L.MCS_E_STATE, fn, 0, 5, 4)
        eng.run(101)
        for fn in both(eng):
            fn(0, 5, 21)  # the last sample at 100
            assert "101" in raises(L.MCS_E_INVALID, fn, 0, 5, 22)  # ... at 105
            assert "101" in raises(L.MCS_E_INVALID, fn, 101, 1, 1)  # a sample at exactly h
            fn(100, 1, 1)
            assert "positive" in raises(L.MCS_E_INVALID, fn, 0, 0, 4)
            assert "positive" in raises(L.MCS_E_INVALID, fn, 0, 5, 0)
        raises(L.MCS_E_INVALID, eng.run, 100)  # a refused run (a decreasing horizon) leaves the series readable
        eng.trade_session_state_series(0, 5, 21)
        s, w, f = eng.trade_session_state_series(0, 5, 21, with_wait=False)  # wait == NULL
        assert w is None
        eng.run()
        for fn in both(eng):
            assert "0xFFFFFFFE" in raises(L.MCS_E_INVALID, fn, 0xFFFFFFF0, 5, 10)
        assert eng.trade_session_state_series(0xFFFFFFFE, 1, 1)[0]["running"].max() == 0  # any second after a drain
        td = eng.trade_session_info()["t_last"]
        eng.append_jobs(one_job(arrays, td + 1))
        for fn in both(eng):  # jobs appended behind a drain that no run has seen
            assert "behind a drain" in raises(L.MCS_E_STATE, fn, 0, 5, 4)
        eng.run()
        eng.trade_session_state_series(0, 5, 4)
        eng.rewind()
        for fn in both(eng):
            assert "mcs_rewind" in raises(L.MCS_E_STATE, fn, 0, 5, 4)
    # first == NULL, and fewer clusters than the engine has, through the C interface
    with session(arrays) as eng:
        eng.submit_jobs(slice_streams(streams, 0, 600))
        eng.run(101)
        want = eng.trade_session_state_series(0, 5, 21)[0]
        out = np.zeros((2, 21), want.dtype)
        lib = L.lib()
        st = lib.mcs_trade_session_state_series(eng._h, 0, 5, 21, out.ctypes.data_as(L.C.POINTER(L.mcs_cluster_sample)),
                                                None, None, 2, None)
        assert st == L.MCS_OK and out.tobytes() == want[:2].tobytes()
        st = lib.mcs_trade_session_state_series(eng._h, 0, 5, 21, None, None, None, 2, None)
        assert st == L.MCS_E_INVALID
        st = lib.mcs_trade_session_state_series(eng._h, 0, 5, 21, out.ctypes.data_as(L.C.POINTER(L.mcs_cluster_sample)),
                                                None, None, 5, None)
        assert st == L.MCS_E_INVALID
    # the session failed: capacity exhausted with a fixed slot pool
    big, bs, _ = seeded_workload("small", 64, 2000)
    with session(big, slot_pool=4) as eng:
        eng.submit_jobs(bs)
        eng.rewind()
        raises(L.MCS_E_CAPACITY, eng.run)
        for fn in both(eng):
            assert "failed" in raises(L.MCS_E_STATE, fn, 0, 5, 4)
    # the Foreign log dropped records
    monkeypatch.setenv("MCS_DTRADE_FOREIGN_LOG_CAP", "8")
    assert ref.o["n_foreign"] > 8
    with session(arrays) as eng:
        eng.append_jobs(streams)
        eng.run()
        assert eng.trade_stats()["flags"] & 0x10  # MCS_FLAG_LOG_OVERFLOW
        for fn in both(eng):
            assert "MCS_FLAG_LOG_OVERFLOW" in raises(L.MCS_E_STATE, fn, 0, 5, 4)
