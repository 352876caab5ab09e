"""GPU tests of trading sessions: online mode of the lock-step DELAY trading system (mcs_run with a
finite horizon, mcs_append_jobs, mcs_rewind and mcs_trade_session_info with MCS_POLICY_DELAY and
cfg.trader; include/mcs_trade.h, DESIGN.md §14 "Trading sessions").

The guarantee under test: slicing never changes a decision.  After mcs_run(h) everything the readers
return equals, bit for bit, the state of a batch run over all the jobs the session ever receives, taken
after that run's last tick below h; after the final drain it equals the whole batch run, ticks and
t_final included.  With h = 1 (mod 5) a lock-step tick exists at h - 1 (every multiple of the sample
period is one), so the reference of a slice is a second engine with all jobs and t_max_s = h - 1, and the
CPU oracle with t_max = h - 1 (tests/test_dtrade_session_ref.py pins that on the oracle alone); only
the truncated batch run sets MCS_FLAG_T_MAX, which is masked out.  Run on a real MI355X."""
import json
import os

import numpy as np
import pytest

import oracle_ref as O
from kat_util import GOLDEN, fuzz_workload, seeded_workload
from mcs_amd import Engine, JobStreams, MCSError
from mcs_amd import _lib as L
from test_dtrade_oracle import check_kat, dt_system

pytestmark = pytest.mark.gpu
DT = json.load(open(os.path.join(GOLDEN, "kats_dtrade.json")))["dtrade"]
TRADE_F = ("t", "requester", "winner", "approvals", "policy", "cores", "mem", "time_s", "failed")
FOREIGN_F = ("requester", "responder", "node", "start", "finish", "c", "m")
STAT_F = ("total_wait_ms", "jobs_count", "moved_l1", "placed_l1")
NONE = L.MCS_TIME_NONE


def slice_streams(streams, lo, hi):
    """the jobs of every cluster with lo <= arrival < hi, as an appended batch (CSR)"""
    parts, off = [[], [], [], []], [0]
    for k in range(len(streams.job_off) - 1):
        sl = streams.of(k)
        a = streams.arrival[sl]
        m = (a >= lo) & (a < hi)
        for i, f in enumerate(("arrival", "dur", "cores", "mem")):
            parts[i].append(getattr(streams, f)[sl][m])
        off.append(off[-1] + int(m.sum()))
    return JobStreams(*[np.concatenate(p).astype(np.uint32) for p in parts], np.array(off, np.uint64))


def concat_streams(a, b):
    """per cluster: a's jobs, then b's"""
    parts, off = [[], [], [], []], [0]
    for k in range(len(a.job_off) - 1):
        for i, f in enumerate(("arrival", "dur", "cores", "mem")):
            parts[i].append(np.concatenate([getattr(a, f)[a.of(k)], getattr(b, f)[b.of(k)]]))
        off.append(off[-1] + len(parts[0][-1]))
    return JobStreams(*[np.concatenate(p).astype(np.uint32) for p in parts], np.array(off, np.uint64))


def snap(eng):
    """everything the readers of a trading run return"""
    node, start, fin = eng.placements()
    return dict(node=node, start=start, finish=fin, trades=eng.contracts(), foreign=eng.foreign(),
                vnodes=[eng.virtual_node_caps(c) for c in range(eng.num_clusters)], ds=eng.delay_stats(),
                ts=eng.trade_stats(), off=eng.job_offsets())


def session(arrays, **cfg):
    eng = Engine(0, policy="DELAY", trader=True, **cfg)
    eng.load_clusters(arrays)
    return eng


def batch(arrays, streams, **cfg):
    with session(arrays, **cfg) as eng:
        eng.submit_jobs(streams)
        eng.run()
        return snap(eng)


def held_rows(full_off, off):
    """rows of the full streams that a session holding the first jobs of every cluster has"""
    return np.concatenate([np.arange(int(full_off[k]), int(full_off[k]) + int(off[k + 1] - off[k]))
                           for k in range(len(off) - 1)]).astype(np.int64)


def rows_equal(g, want_node, want_start, want_fin, full_off, what):
    idx = held_rows(full_off, g["off"])
    rest = np.ones(len(want_node), bool)
    rest[idx] = False
    assert (want_node[rest] == -1).all(), what  # what the session does not hold yet is undecided in the reference
    np.testing.assert_array_equal(g["node"], want_node[idx], err_msg=f"{what} node")
    np.testing.assert_array_equal(g["start"], want_start[idx], err_msg=f"{what} start")
    np.testing.assert_array_equal(g["finish"], want_fin[idx], err_msg=f"{what} finish")


def equal_engine(g, b, full_off, what, mask=0):
    """check_equal of tests/test_gpu_dtrade.py between a session and a batch engine over the full streams"""
    rows_equal(g, b["node"], b["start"], b["finish"], full_off, what)
    assert g["trades"].tobytes() == b["trades"].tobytes(), what
    assert g["foreign"].tobytes() == b["foreign"].tobytes(), what
    assert g["vnodes"] == b["vnodes"], what
    for f in STAT_F:
        np.testing.assert_array_equal(g["ds"][f], b["ds"][f], err_msg=f"{what} {f}")
    for f in ("t_final", "ticks", "trades", "trades_won"):
        assert g["ts"][f] == b["ts"][f], (what, f, g["ts"][f], b["ts"][f])
    assert g["ts"]["flags"] & ~mask == b["ts"]["flags"] & ~mask, what


def equal_oracle(g, o, full_off, what):
    rows_equal(g, o["node"], o["start"], o["finish"], full_off, what)
    assert len(g["trades"]) == len(o["trades"]), what
    for f in TRADE_F:
        np.testing.assert_array_equal(g["trades"][f], o["trades"][f], err_msg=f"{what} {f}")
    assert len(g["foreign"]) == o["n_foreign"], what
    for f in FOREIGN_F:
        np.testing.assert_array_equal(g["foreign"][f], o["foreign"][f], err_msg=f"{what} {f}")
    assert g["vnodes"] == o["vnodes"], what
    for f in STAT_F:
        np.testing.assert_array_equal(g["ds"][f], o["stats"][f], err_msg=f"{what} {f}")
    assert g["ts"]["t_final"] == o["t_final"], what
    assert g["ts"]["trades"] == o["n_trades"], what


def system(name):
    if name == "fuzz":  # on the oracle: 31 trades, 51 Foreign jobs, t_final 18946
        return fuzz_workload("w16s", 2, n_clusters=4, J=900, blocking=False)
    arrays, streams, _ = seeded_workload("small", 8, 300)
    return arrays, streams


_REF = {}


def reference(name):
    """the batch run and the oracle over the whole system, computed once and never modified"""
    if name not in _REF:
        arrays, streams = system(name)
        _REF[name] = (arrays, streams, batch(arrays, streams), O.dtrade_run(arrays, streams))
    return _REF[name]


# ---- 1. the hand-derived scenarios as sessions ---------------------------------------------------------
@pytest.mark.parametrize("k", DT, ids=[k["name"] for k in DT])
def test_session_kats(k):
    """Every DELAY trading KAT, its jobs appended in three slices by arrival with horizons between them
    and a drain: the hand-derived answers pin the session without any batch run."""
    arrays, s = dt_system(k)
    arr = np.unique(s.arrival)
    h1, h2 = (min(int(arr[len(arr) * i // 3]), k["t_max"] + 1) for i in (1, 2))
    with session(arrays, t_max_s=k["t_max"]) as eng:
        eng.append_jobs(slice_streams(s, 0, h1))
        st = eng.run(h1)
        assert st.online and st.t_horizon == h1
        eng.append_jobs(slice_streams(s, h1, h2))
        eng.run(h2)
        eng.append_jobs(slice_streams(s, h2, 1 << 32))
        st = eng.run()
        assert st.online and st.t_horizon == NONE
        r = snap(eng)
        info = eng.trade_session_info()
    assert np.array_equal(r["off"], s.job_off)
    check_kat(k, r["node"], r["start"], r["finish"], r["trades"], r["foreign"], len(r["foreign"]), r["vnodes"],
              r["ts"]["t_final"])
    for key, v in k.get("stats0", {}).items():
        assert r["ds"][key][0] == v, key
    assert info["drained"] == 1 and info["restarts"] == 0 and info["ticks_total"] == r["ts"]["ticks"]


# ---- 2. slices equal the truncated batch run -----------------------------------------------------------
@pytest.mark.parametrize("name", ["fuzz", "small"])
def test_session_slices_equal_truncated_batch(name):
    """About eight horizons = 1 (mod 5) over the run, the jobs below each appended just before it: the
    state after every slice equals a second engine with all jobs and t_max_s = h - 1 and the oracle with
    t_max = h - 1; after the drain it equals the untruncated batch run and the oracle."""
    arrays, streams, b_full, o_full = reference(name)
    tf = int(o_full["t_final"])
    hs = sorted({5 * (int(x) // 5) + 1 for x in np.linspace(0, tf, 10)[1:-1]})
    assert len(hs) == 8 and hs[-1] < tf
    with session(arrays) as eng:
        prev = 0
        for h in hs:
            eng.append_jobs(slice_streams(streams, prev, h))
            st = eng.run(h)
            g = snap(eng)
            assert st.online and st.t_horizon == h and st.jobs == len(g["node"])
            assert st.placed == int((g["node"] >= 0).sum()) and st.pending == st.jobs - st.placed
            equal_engine(g, batch(arrays, streams, t_max_s=h - 1), streams.job_off, f"h={h}", mask=L.MCS_FLAG_T_MAX)
            equal_oracle(g, O.dtrade_run(arrays, streams, t_max=h - 1), streams.job_off, f"h={h}")
            info = eng.trade_session_info()
            assert info["t_horizon"] == h and info["t_last"] == h - 1 and info["t_next"] >= h and not info["drained"]
            prev = h
        eng.append_jobs(slice_streams(streams, prev, 1 << 32))
        eng.run()
        g = snap(eng)
        info = eng.trade_session_info()
    equal_engine(g, b_full, streams.job_off, "drain")
    equal_oracle(g, o_full, streams.job_off, "drain")
    assert info["drained"] == 1 and info["restarts"] == 0 and info["ticks_total"] == b_full["ts"]["ticks"]


# ---- 3. arbitrary horizons and tiny slices -------------------------------------------------------------
def test_session_200_arbitrary_slices_resume():
    """The fuzz system in 200 slices of random length 1 - 300 s (half of them at most 20 s: the sum has to
    stay below the batch run's final tick, past which a session executes ticks the batch run never
    reaches, case 5), no horizon = 1 (mod 5).  After every slice the rows with start < h equal the batch
    run's and the others are undecided; the contracts with t_s < h and the Foreign records with
    start_s < h equal the batch run's prefix.  After the drain everything is equal, and the ticks of the
    slices add up to the batch run's: no tick is executed twice, none is added (a replay from t = 0 per
    slice fails this)."""
    arrays, streams, b, o = reference("fuzz")
    rng = np.random.default_rng(11)
    lens = np.where(rng.random(200) < 0.5, rng.integers(1, 21, 200), rng.integers(1, 300, 200))
    hs = np.cumsum(lens)
    for i in range(len(hs)):  # (lengths stay within 1 - 300: at most one second is added to a slice)
        if hs[i] % 5 == 1:
            hs[i:] += 1
    assert len(hs) == 200 and (np.diff(np.concatenate([[0], hs])) >= 1).all() and (hs % 5 != 1).all()
    assert np.diff(np.concatenate([[0], hs])).max() <= 300 and hs[-1] < b["ts"]["t_final"]
    ticks = 0
    with session(arrays) as eng:
        prev = 0
        for h in (int(x) for x in hs):
            eng.append_jobs(slice_streams(streams, prev, h))
            eng.run(h)
            g = snap(eng)
            idx = held_rows(streams.job_off, g["off"])
            dec = (b["start"][idx] < h) & (b["node"][idx] >= 0)
            for f in ("node", "start", "finish"):
                np.testing.assert_array_equal(g[f][dec], b[f][idx][dec], err_msg=f"h={h} {f}")
            assert (g["node"][~dec] == L.MCS_NODE_UNPLACED).all() and (g["start"][~dec] == NONE).all(), h
            assert (g["finish"][~dec] == NONE).all(), h
            assert g["trades"].tobytes() == b["trades"][b["trades"]["t"] < h].tobytes(), h
            assert g["foreign"].tobytes() == b["foreign"][b["foreign"]["start"] < h].tobytes(), h
            info = eng.trade_session_info()
            ticks += info["ticks_last_run"]
            assert info["ticks_total"] == ticks and info["t_last"] < h <= info["t_next"], (h, info)
            prev = h
        eng.append_jobs(slice_streams(streams, prev, 1 << 32))
        eng.run()
        g = snap(eng)
        info = eng.trade_session_info()
    ticks += info["ticks_last_run"]
    equal_engine(g, b, streams.job_off, "drain")
    equal_oracle(g, o, streams.job_off, "drain")
    assert ticks == info["ticks_total"] == b["ts"]["ticks"] and info["restarts"] == 0


# ---- 4. idle ends --------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["below_parked", "above_parked", "at_horizon"])
def test_session_idle_end_then_append(where):
    """A horizon reached with every known job decided (the Go loops idle: samples every 5 s, trader rounds
    falling due), then jobs appended past it: the first new arrival below the parked tick, above it, or
    exactly at the horizon.  Equal to the batch run over all jobs."""
    arrays, streams, _, _ = reference("small")
    first = slice_streams(streams, 0, 600)
    o1 = O.dtrade_run(arrays, first)
    d = int(o1["t_final"])  # the tick that decides the last of them
    h = 5 * ((d + 60) // 5) + 1
    with session(arrays) as eng:
        eng.append_jobs(first)
        st = eng.run(h)
        assert st.pending == 0
        parked = eng.trade_session_info()["t_next"]
        assert h < parked <= h + 4  # (the next sample tick at the latest)
        a0 = {"below_parked": parked - 1, "above_parked": parked + 7, "at_horizon": h}[where]
        rest = slice_streams(streams, 600, 1 << 32)
        shift = a0 - int(rest.arrival.min())
        rest = JobStreams((rest.arrival.astype(np.int64) + shift).astype(np.uint32), rest.dur, rest.cores, rest.mem,
                          rest.job_off)
        everything = concat_streams(first, rest)
        # the idle stretch is not empty on the oracle: a sample tick or a trader round falls into it
        o = O.dtrade_run(arrays, everything)
        assert any(t % 5 == 0 for t in range(d + 1, h)) or ((o["trades"]["t"] > d) & (o["trades"]["t"] < h)).any()
        eng.append_jobs(rest)
        assert eng.trade_session_info()["t_next"] == min(parked, a0)
        eng.run()
        g = snap(eng)
        info = eng.trade_session_info()
    b = batch(arrays, everything)
    equal_engine(g, b, everything.job_off, where)
    equal_oracle(g, o, everything.job_off, where)
    assert info["ticks_total"] == b["ts"]["ticks"] and info["restarts"] == 0


# ---- 5. a horizon past the end -------------------------------------------------------------------------
def test_session_horizon_past_the_end_then_append():
    """Drain, then mcs_run(t_final + 600): sample ticks and trader rounds the batch run never reaches.
    Placements are unchanged, the logs up to the batch run's t_final are equal and every further record
    lies after it.  Jobs appended then continue the system: equal to the batch run over all jobs."""
    arrays, streams, _, _ = reference("small")
    first = slice_streams(streams, 0, 600)
    b1 = batch(arrays, first)
    tf = b1["ts"]["t_final"]
    with session(arrays) as eng:
        eng.append_jobs(first)
        eng.run()
        equal_engine(snap(eng), b1, first.job_off, "drain")
        st = eng.run(tf + 600)
        g = snap(eng)
        info = eng.trade_session_info()
        assert st.pending == 0 and info["ticks_last_run"] >= 600 // 5 and info["t_last"] > tf
        for f in ("node", "start", "finish"):
            np.testing.assert_array_equal(g[f], b1[f], err_msg=f)
        nt, nf = len(b1["trades"]), len(b1["foreign"])
        assert g["trades"][:nt].tobytes() == b1["trades"].tobytes() and (g["trades"]["t"][nt:] > tf).all()
        assert g["foreign"][:nf].tobytes() == b1["foreign"].tobytes() and (g["foreign"]["start"][nf:] > tf).all()
        rest = slice_streams(streams, 600, 1 << 32)
        shift = tf + 600 + 3 - int(rest.arrival.min())
        rest = JobStreams((rest.arrival.astype(np.int64) + shift).astype(np.uint32), rest.dur, rest.cores, rest.mem,
                          rest.job_off)
        everything = concat_streams(first, rest)
        eng.append_jobs(rest)
        eng.run()
        g = snap(eng)
    b = batch(arrays, everything)
    equal_engine(g, b, everything.job_off, "all jobs")
    equal_oracle(g, O.dtrade_run(arrays, everything), everything.job_off, "all jobs")


# ---- 6. escalation inside a session --------------------------------------------------------------------
@pytest.mark.parametrize("case", ["slots", "vnodes"])
def test_session_escalation_replays(case):
    """A slot-pool overflow (C5-DELAY's system: 256 -> 384 slots) and a virtual-node overflow (one cluster
    receives 81 virtual nodes, above the initial 64) inside a session of ten slices: the session is
    replayed from t = 0 with the grown capacity; the final state equals the batch run and the oracle."""
    if case == "slots":
        arrays, streams, _ = seeded_workload("small", 64, 2000)
    else:
        arrays, streams = fuzz_workload("w16s", 2, n_clusters=8, J=1500, blocking=False)
    o = O.dtrade_run(arrays, streams)
    if case == "vnodes":
        assert max(len(v) for v in o["vnodes"]) == 81
    b = batch(arrays, streams)
    hs = [int(x) for x in np.linspace(0, int(o["t_final"]), 12)[1:-1]]
    esc = 0
    with session(arrays) as eng:
        prev = 0
        for h in hs:
            eng.append_jobs(slice_streams(streams, prev, h))
            esc += eng.run(h).escalations
            prev = h
        eng.append_jobs(slice_streams(streams, prev, 1 << 32))
        st = eng.run()
        esc += st.escalations
        g = snap(eng)
        info = eng.trade_session_info()
    assert info["restarts"] >= 1 and info["restarts"] == esc
    if case == "slots":
        assert st.slot_pool == 6
    equal_engine(g, b, streams.job_off, case)
    equal_oracle(g, o, streams.job_off, case)
    assert info["ticks_total"] == b["ts"]["ticks"]


# ---- 7. rewind, and a session started after a batch run ------------------------------------------------
@pytest.mark.parametrize("how", ["rewind", "after_batch"])
def test_session_restart_with_new_jobs(how):
    """mcs_rewind restarts at t = 0 with every job so far; mcs_append_jobs after a batch run starts a
    session at t = 0 over the submitted jobs.  New jobs appended below the next horizon change later
    decisions: equal to a fresh batch engine over all jobs."""
    arrays, streams, _, _ = reference("fuzz")
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
    with session(arrays) as eng:
        eng.submit_jobs(base)
        if how == "rewind":
            eng.run(4001)
            eng.run()
            eng.rewind()
            assert eng.trade_session_info()["ticks_total"] == 0
        else:
            st = eng.run()
            assert not st.online and eng.trade_stats()["loop_form"] == 5
        eng.append_jobs(late)
        h = 5 * ((lo + 1000) // 5) + 1
        eng.run(h)
        g = snap(eng)
        equal_engine(g, batch(arrays, everything, t_max_s=h - 1), everything.job_off, how, mask=L.MCS_FLAG_T_MAX)
        eng.run()
        g = snap(eng)
    equal_engine(g, batch(arrays, everything), everything.job_off, how)
    equal_oracle(g, O.dtrade_run(arrays, everything), everything.job_off, how)


# ---- 8. refusals ---------------------------------------------------------------------------------------
def raises(code, fn, *a, **kw):
    with pytest.raises(MCSError) as ei:
        fn(*a, **kw)
    assert ei.value.code == code, ei.value
    return str(ei.value)


def one_job(arrays, arrival):
    return JobStreams(*[np.array([v], np.uint32) for v in (arrival, 5, 1, 1)],
                      np.array([0] + [1] * arrays.n_clusters, np.uint64))


def test_session_refusals():
    arrays, streams, _, _ = reference("small")
    # FIFO trading: sessions are not built for it
    for cfg in (dict(borrow=True), dict(trader=True), dict(borrow=True, trader=True)):
        with Engine(0, policy="FIFO", **cfg) as eng:
            eng.load_clusters(arrays)
            eng.submit_jobs(streams)
            assert "FIFO trading" in raises(L.MCS_E_INVALID, eng.run, 100)
            assert "FIFO trading" in raises(L.MCS_E_STATE, eng.append_jobs, one_job(arrays, 5000))
            raises(L.MCS_E_STATE, eng.trade_session_info)
    # a sharded engine, and one with a communicator
    with session(arrays) as eng:
        eng.set_shard(0, 2)
        eng.submit_jobs(streams)
        assert "one engine" in raises(L.MCS_E_STATE, eng.run, 100)
        assert "one engine" in raises(L.MCS_E_STATE, eng.append_jobs, one_job(arrays, 5000))
    with session(arrays) as eng:
        eng.set_shard(0, 1)
        eng.comm_init(Engine.comm_unique_id())
        eng.submit_jobs(streams)
        assert "one engine" in raises(L.MCS_E_STATE, eng.run, 100)
    with session(arrays, t_max_s=5000) as eng:
        eng.submit_jobs(slice_streams(streams, 0, 600))
        raises(L.MCS_E_STATE, eng.trade_session_info)  # no session yet
        raises(L.MCS_E_INVALID, eng.run, 5002)  # above t_max_s + 1
        eng.run(101)
        raises(L.MCS_E_INVALID, eng.run, 100)  # a decreasing horizon: nothing runs
        assert eng.trade_session_info()["t_horizon"] == 101
        raises(L.MCS_E_INVALID, eng.append_jobs, one_job(arrays, 100))  # below the last horizon
        raises(L.MCS_E_STATE, eng.trade_begin)
        # the telemetry calls are the follow-up
        for fn, args in ((eng.dtrade_state_series, (0, 5, 4)), (eng.level1_series, (0, 5, 4)),
                         (eng.level1_at, (0, 50)), (eng.online_state_series, (0, 5, 4)),
                         (eng.online_level1_series, (0, 5, 4)), (eng.stream_open, (0, 5)),
                         (eng.cluster_states, (50,)), (eng.cluster_state_series, (0, 5, 4)),
                         (eng.wait_time_series, (0, 5, 4))):
            assert "trading session" in raises(L.MCS_E_STATE, fn, *args), fn.__name__
        eng.run()
        td = eng.trade_session_info()["t_last"]
        raises(L.MCS_E_INVALID, eng.append_jobs, one_job(arrays, td))  # the drain floor is T_d + 1
        eng.append_jobs(one_job(arrays, td + 1))
        assert eng.trade_session_info()["t_next"] == td + 1
        assert eng.run().pending == 0 and eng.trade_session_info()["t_last"] >= td + 1
    # capacity exhausted with a fixed slot pool: MCS_E_CAPACITY, then MCS_E_STATE until mcs_rewind
    big, bs, _ = seeded_workload("small", 64, 2000)
    with session(big, slot_pool=4) as eng:
        eng.submit_jobs(bs)
        eng.rewind()  # (a session at t = 0: mcs_run(MCS_TIME_NONE) is then its drain, not a batch run)
        raises(L.MCS_E_CAPACITY, eng.run)  # (the system peaks at 331 running jobs in one cluster, above 256)
        assert eng.trade_session_info()["failed"] == 1
        assert "failed" in raises(L.MCS_E_STATE, eng.run, 4001)
        raises(L.MCS_E_STATE, eng.run)
        eng.rewind()
        assert eng.trade_session_info()["failed"] == 0
        eng.run(501)


# ---- 9. the batch run is what it was -------------------------------------------------------------------
@pytest.mark.parametrize("resident", ["1", "0"])
def test_batch_trading_run_unchanged(resident, monkeypatch):
    """A batch trading run on an engine that never had a session: the resident tick (loop form 5), or the
    replayed kernels with MCS_DT_RESIDENT=0 (0), equal to the oracle."""
    monkeypatch.setenv("MCS_DT_RESIDENT", resident)
    arrays, streams, _, o = reference("fuzz")
    with session(arrays) as eng:
        eng.submit_jobs(streams)
        st = eng.run()
        g = snap(eng)
        raises(L.MCS_E_STATE, eng.trade_session_info)
    assert not st.online and g["ts"]["loop_form"] == (5 if resident == "1" else 0)
    equal_oracle(g, o, streams.job_off, "batch")
