"""GPU tests of the external traders' calls on a trading session (mcs_trade_external,
mcs_trade_session_provide_vnodes, mcs_trade_session_receive_vnodes, mcs_trade_session_read_nodes;
include/mcs_trade.h, DESIGN.md §14 "External traders").

The reference is the oracle's own trading run replayed from outside (tests/test_dtrade_external_ref.py
pins the rule on the CPU): an external-mode session runs to every tick at which the oracle's built-in
traders reached a responder, issues that tick's ProvideVirtualNode calls and ReceiveVirtualNode calls
itself, and must end, bit for bit, where the oracle's run with built-in traders ended.  The walk's edges
are checked against AllocateVirtualNodeResources on the rows the engine reports (walk(), pinned to
O.allocate_virtual_node on the CPU).  Run on a real MI355X: ``pytest -m gpu``."""
import numpy as np
import pytest

import oracle_ref as O
from mcs_amd import Cluster, Engine, JobStreams, MCSError, Node, pack_clusters
from mcs_amd import _lib as L
from test_dtrade_external_ref import SYSTEMS, oracle, replay_plan, system, walk
from test_gpu_dtrade_session import STAT_F, raises
from test_gpu_online_series import assert_state_equal
from test_gpu_wait_series import assert_bits_equal

pytestmark = pytest.mark.gpu
FOREIGN_F = ("requester", "responder", "node", "start", "finish", "c", "m")


def ext_session(arrays, streams, t_max=0xFFFFFFFE, external=True, **cfg):
    if t_max != 0xFFFFFFFE:
        cfg["t_max_s"] = t_max
    eng = Engine(0, policy="DELAY", trader=True, **cfg)
    eng.load_clusters(arrays)
    eng.submit_jobs(streams)
    if external:
        eng.trade_external(True)
    return eng


def state(eng):
    node, start, fin = eng.placements()
    return dict(node=node, start=start, finish=fin, foreign=eng.foreign(), ds=eng.delay_stats(),
                vnodes=[eng.virtual_node_caps(c) for c in range(eng.num_clusters)])


def states_equal(a, b, what, stats=True):
    for f in ("node", "start", "finish"):
        np.testing.assert_array_equal(a[f], b[f], err_msg=f"{what} {f}")
    assert a["foreign"].tobytes() == b["foreign"].tobytes(), what
    assert a["vnodes"] == b["vnodes"], what
    if stats:
        for f in STAT_F:
            np.testing.assert_array_equal(a["ds"][f], b["ds"][f], err_msg=f"{what} {f}")


def equals_oracle(g, o, what):
    for f in ("node", "start", "finish"):
        np.testing.assert_array_equal(g[f], o[f], err_msg=f"{what} {f}")
    assert len(g["foreign"]) == o["n_foreign"], what
    for f in FOREIGN_F:
        np.testing.assert_array_equal(g["foreign"][f], o["foreign"][f], err_msg=f"{what} foreign {f}")
    assert g["vnodes"] == o["vnodes"], what
    for f in STAT_F:
        np.testing.assert_array_equal(g["ds"][f], o["stats"][f], err_msg=f"{what} {f}")


def replay(eng, plan, between=None):
    """The oracle's run as an outside trader's calls on an external-mode session: for every tick with a
    reached responder run(T + 1), one provide call with the tick's requests in (requester, pop) order,
    checked against the log and against the walk over the rows the engine reports, then the winners'
    nodes; then a drain.  between(eng, t_prev, t): extra work before the run to t + 1."""
    prev = 0
    for t, rounds, nodes in plan:
        if between:
            between(eng, prev, t)
        eng.run(t + 1)
        assert eng.trade_session_info()["t_last"] == t
        reqs = [r for _, _, _, rq in rounds for r in rq]
        if reqs:
            rows = {}
            want = []
            for r in reqs:
                c = r["responder"]
                if c not in rows:
                    rows[c] = [list(x) for x in eng.trade_session_nodes(c)]
                ok, visited, lc, lm, jobs, fc, fm = walk(rows[c][0], rows[c][1], r["cores"], r["memory"])
                if r["time_s"]:
                    rows[c] = [fc, fm]
                assert (ok, visited) == (r["ok"], r["visited"]), (t, r, ok, visited)
                want.append((ok, visited, lc, lm))
            res, st = eng.provide_virtual_nodes([(r["responder"], r["requester"], r["cores"], r["memory"], r["time_s"])
                                                 for r in reqs])
            got = [tuple(int(x) for x in row) for row in res]
            assert got == want, (t, got, want)
            assert st["n"] == len(reqs) and st["n_ok"] == sum(w[0] for w in want)
            assert st["foreign_added"] == sum(w[1] for w in want)
            for c, (fc, fm) in rows.items():
                gc, gm = eng.trade_session_nodes(c)
                assert [int(x) for x in gc] == [int(x) for x in fc] and [int(x) for x in gm] == [int(x) for x in fm], (t, c)
        if nodes:
            st = eng.receive_virtual_nodes(nodes)
            assert st["n"] == st["n_ok"] == len(nodes)
        prev = t
    eng.run()


# ---- 1. the replay equals the oracle -------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in SYSTEMS if n != "small8"])
def test_replay_equals_the_oracle(name):
    arrays, streams, t_max = system(name)
    o = oracle(name)
    with ext_session(arrays, streams, t_max) as eng:
        replay(eng, replay_plan(o))
        g = state(eng)
        assert len(eng.contracts()) == 0  # no round: nothing goes to the contract log
        assert eng.trade_session_info()["restarts"] == 0
        if name == "big8":
            n = int(o["t_final"]) // 5 + 1
            gs, gw, _ = eng.trade_session_state_series(0, 5, n)
    equals_oracle(g, o, name)
    if name == "big8":  # the Start stream over the whole run equals the run with built-in traders
        with ext_session(arrays, streams, t_max, external=False) as b:
            b.run()
            bs, bw, _ = b.dtrade_state_series(0, 5, n)
        assert_state_equal(gs, bs, "big8 state")
        assert_bits_equal(gw, bw, "big8 wait")


# ---- 2. no grants: the oracle without traders ------------------------------------------------------------
def test_no_grants_is_the_system_without_traders():
    arrays, streams, _ = system("small8")
    o = O.dtrade_run(arrays, streams, trader=False)
    assert o["n_trades"] == 0 and o["n_foreign"] == 0
    with ext_session(arrays, streams) as eng:  # a batch run: the replayed kernels, not the resident tick
        st = eng.run()
        assert not st.online
        g = state(eng)
        assert eng.trade_stats()["loop_form"] == 0 and len(eng.contracts()) == 0
    equals_oracle(g, o, "batch")
    with ext_session(arrays, streams) as eng:
        eng.run(1)
        eng.run()
        g = state(eng)
        assert eng.trade_stats()["loop_form"] == 0 and len(eng.contracts()) == 0
    equals_oracle(g, o, "session")


# ---- 3. the walk at its edges ------------------------------------------------------------------------------
SIZES = (1, 5, 64, 65, 129, 63)  # physical rows of the responders; the last one receives 2 virtual rows
T0 = 11                            # the tick the grants act at (no sample tick: it is forced)
REQ = len(SIZES)                   # the requester: a cluster of its own


def edge_system(last_big):
    """Responders whose rows are all free {32, 24000}, with last_big the last row {100, 60000} (a walk that
    carries {32, 24000} leaves a job {0, 0} on every row and is exhausted by the last one); a job per
    responder that arrives at 20 and fits no row left with {10, 1000}."""
    cls = []
    for k, n in enumerate(SIZES):
        nodes = [Node(Id=i, Cores=32, Memory=24000, CoresAvailable=32, MemoryAvailable=24000) for i in range(n)]
        if last_big and k != len(SIZES) - 1:
            nodes[-1] = Node(Id=n - 1, Cores=100, Memory=60000, CoresAvailable=100, MemoryAvailable=60000)
        cls.append(Cluster(Id=k + 1, Nodes=nodes))
    cls.append(Cluster(Id=len(SIZES) + 1, Nodes=[Node(Id=0, Cores=32, Memory=24000, CoresAvailable=32,
                                                      MemoryAvailable=24000)]))
    arrays = pack_clusters(cls)
    nj = len(SIZES)
    streams = JobStreams(np.full(nj, 20, np.uint32), np.full(nj, 5, np.uint32), np.full(nj, 11, np.uint32),
                         np.full(nj, 1001, np.uint32), np.array(list(range(nj + 1)) + [nj], np.uint64))
    return arrays, streams


def edge_session(last_big):
    arrays, streams = edge_system(last_big)
    eng = ext_session(arrays, streams)
    eng.run(T0 + 1)
    assert eng.trade_session_info()["t_last"] == T0
    eng.receive_virtual_nodes([(len(SIZES) - 1, 32, 24000), (len(SIZES) - 1, 100, 60000) if last_big
                               else (len(SIZES) - 1, 32, 24000)])
    return arrays, streams, eng


def rebuilt_rows(eng, arrays, streams, c, t):
    """a cluster's counters after tick t and the grants at it, from the loaded free values, the virtual
    nodes' capacities, the placements and the Foreign log"""
    sl = arrays.nodes_of(c)
    caps = eng.virtual_node_caps(c)
    fc = [int(x) for x in arrays.free_c[sl]] + [v[0] for v in caps]
    fm = [int(x) for x in arrays.free_m[sl]] + [v[1] for v in caps]
    node, start, fin = eng.placements()
    for j in range(int(streams.job_off[c]), int(streams.job_off[c + 1])):
        if node[j] >= 0 and start[j] <= t < fin[j]:
            fc[node[j]] -= int(streams.cores[j])
            fm[node[j]] -= int(streams.mem[j])
    for f in eng.foreign():
        if f["responder"] == c and f["start"] != f["finish"] and f["start"] <= t < f["finish"]:
            fc[f["node"]] -= int(f["c"])
            fm[f["node"]] -= int(f["m"])
    return [x % (1 << 64) for x in fc], [x % (1 << 64) for x in fm]


def provide_checked(eng, arrays, streams, reqs):
    """one provide call against the walk over the rows the engine reports; returns the expected results"""
    C = len(SIZES)
    rows = {c: [list(x) for x in eng.trade_session_nodes(c)] for c in range(C)}
    n_log = len(eng.foreign())
    want, recs = [], []
    for (c, q, rc, rm, ts) in reqs:
        ok, visited, lc, lm, jobs, fc, fm = walk(rows[c][0], rows[c][1], rc, rm)
        if ts:
            rows[c] = [fc, fm]
        want.append((ok, visited, lc, lm))
        recs += [(q, c, i, T0, T0 + ts, jc, jm) for i, (jc, jm) in enumerate(jobs)]
    res, st = eng.provide_virtual_nodes(reqs)
    assert [tuple(int(x) for x in r) for r in res] == want
    assert st["foreign_added"] == len(recs) and st["replayed"] == 0
    log = eng.foreign()[n_log:]  # array order, row order within a request
    assert [tuple(int(r[f]) for f in FOREIGN_F) for r in log] == recs
    for c in range(C):
        gc, gm = eng.trade_session_nodes(c)
        assert [int(x) for x in gc] == rows[c][0] and [int(x) for x in gm] == rows[c][1], c
        assert rebuilt_rows(eng, arrays, streams, c, T0) == (rows[c][0], rows[c][1]), c
    return want


def jobs_follow(eng, arrays, streams):
    """the job of every responder (arrival 20, {11, 1001}) goes to the first row that holds it while the
    Foreign jobs hold, or waits for their release"""
    rows = {c: eng.trade_session_nodes(c) for c in range(len(SIZES))}
    ends = {c: max([int(f["finish"]) for f in eng.foreign() if f["responder"] == c and f["start"] != f["finish"]] or [0])
            for c in range(len(SIZES))}
    eng.run(200)
    node, start, _ = eng.placements()
    for c in range(len(SIZES)):
        fit = [i for i in range(len(rows[c][0])) if int(rows[c][0][i]) >= 11 and int(rows[c][1][i]) >= 1001]
        if fit:
            assert (node[c], start[c]) == (fit[0], 20), (c, node[c], start[c], fit[0])
        else:
            assert node[c] >= 0 and start[c] >= ends[c] > 20, (c, node[c], start[c], ends[c])


EDGE = {
    # name: (last row big, the calls' requests as (cores, memory, time_s) per call, what every responder answers)
    "row0": (True, [[(10, 1000, 50)]], lambda nn: [(1, 1, 0, 0)]),
    "last_row": (True, [[(32, 24000, 50)]], lambda nn: [(1, nn, 0, 0)]),
    "never": (False, [[(32, 24000, 50)]], lambda nn: [(0, nn, 32, 24000)]),
    "cores_only": (True, [[(32, 0, 50)]], lambda nn: [(1, nn, 0, 0)]),
    "memory_only": (True, [[(0, 24000, 50)]], lambda nn: [(1, nn, 0, 0)]),
    "time0": (True, [[(32, 24000, 0)]], lambda nn: [(1, nn, 0, 0)]),
    # the second request wraps row 0's counters ({10, 1000} - {40, 4000}); the third meets the wrapped row
    "wrapped": (True, [[(10, 1000, 50)], [(50, 5000, 50)], [(5, 5, 50)]], None),
    # two requests to every responder in one array: the second sees the first
    "two_in_one": (True, [[(10, 1000, 50), (50, 5000, 50)]], None),
}


@pytest.mark.parametrize("name", list(EDGE))
def test_walk_edges(name):
    last_big, calls, answers = EDGE[name]
    arrays, streams, eng = edge_session(last_big)
    with eng:
        for k, call in enumerate(calls):
            # requests to all responders interleaved in one array: log order = array order
            reqs = [(c, REQ, rc, rm, ts) for (rc, rm, ts) in call for c in range(len(SIZES))]
            got = provide_checked(eng, arrays, streams, reqs)
            if answers:
                for c, n in enumerate(SIZES):
                    nn = n + (2 if c == len(SIZES) - 1 else 0)
                    assert [got[c]] == answers(nn), (name, c, got[c])
            if name == "wrapped" and k == 1:  # the second request wrapped row 0
                gc, gm = eng.trade_session_nodes(2)
                assert int(gc[0]) == (1 << 64) - 30 and int(gm[0]) == (1 << 64) - 3000
            if name == "wrapped" and k == 2:  # the third met it: exhausted at row 0 by the huge differences
                assert all(g == (1, 1, 0, 0) for g in got)
        if name == "time0":
            assert all(f["start"] == f["finish"] for f in eng.foreign())
        jobs_follow(eng, arrays, streams)


# ---- 4. the forced tick ---------------------------------------------------------------------------------
def test_forced_last_tick():
    h = 13  # the job finishes at h - 2; h - 1 = 12 is no sample tick
    arrays = pack_clusters([Cluster(Id=1, Nodes=[Node(Id=i, Cores=32, Memory=24000, CoresAvailable=32,
                                                      MemoryAvailable=24000) for i in range(5)])])
    streams = JobStreams(*[np.array([v], np.uint32) for v in (0, h - 2, 4, 100)], np.array([0, 1], np.uint64))
    out = []
    for hs in ((h,), (h - 3, h)):
        with ext_session(arrays, streams) as eng:
            for x in hs:
                eng.run(x)
                assert eng.trade_session_info()["t_last"] == x - 1
            fc, fm = eng.trade_session_nodes(0)
            assert [int(x) for x in fc] == [32] * 5 and [int(x) for x in fm] == [24000] * 5  # the job's node is free
            res, _ = eng.provide_virtual_nodes([(0, 0, 40, 30000, 7)])
            out.append((state(eng), res.tobytes(), [x.tobytes() for x in eng.trade_session_nodes(0)],
                        eng.trade_session_info()["ticks_total"]))
    states_equal(out[0][0], out[1][0], "forced tick")
    assert out[0][1] == out[1][1] and out[0][2] == out[1][2]
    assert (out[0][3], out[1][3]) == (4, 5)  # ticks 0, 5, 10, 12 and 0, 5, 9, 10, 12
    with ext_session(arrays, streams, external=False) as eng:  # with the built-in traders nothing is forced
        eng.run(h)
        assert eng.trade_session_info()["t_last"] == 10


# ---- 5. slicing invariance --------------------------------------------------------------------------------
def test_slicing_changes_no_grant_outcome():
    arrays, streams, t_max = system("small4")
    plan = replay_plan(oracle("small4"))
    rng = np.random.default_rng(11)

    def extra(eng, prev, t):
        if t - prev > 1:
            for h in sorted(int(x) for x in rng.integers(prev + 1, t + 1, 3)):
                eng.run(h)

    with ext_session(arrays, streams, t_max) as eng:
        replay(eng, plan)
        a, ticks_a = state(eng), eng.trade_session_info()["ticks_total"]
    with ext_session(arrays, streams, t_max) as eng:
        replay(eng, plan, between=extra)
        b, ticks_b = state(eng), eng.trade_session_info()["ticks_total"]
    states_equal(a, b, "sliced")
    assert ticks_b >= ticks_a


# ---- 6. capacity --------------------------------------------------------------------------------------------
def piled_system():
    """cluster 0: 8 rows, row 0 wide enough for 250 small long jobs; cluster 1: the requester"""
    nodes = [Node(Id=0, Cores=1000, Memory=100000, CoresAvailable=1000, MemoryAvailable=100000)] + \
            [Node(Id=i, Cores=32, Memory=24000, CoresAvailable=32, MemoryAvailable=24000) for i in range(1, 8)]
    arrays = pack_clusters([Cluster(Id=1, Nodes=nodes), Cluster(Id=2, Nodes=nodes[1:3])])
    nj = 250
    streams = JobStreams(np.zeros(nj, np.uint32), np.full(nj, 100000, np.uint32), np.ones(nj, np.uint32),
                         np.ones(nj, np.uint32), np.array([0, nj, nj], np.uint64))
    return arrays, streams


def piled_calls(eng):
    """an early grant and a node on cluster 1, then a walk over cluster 0's 8 rows with 6 running slots free"""
    eng.run(100)
    r1, s1 = eng.provide_virtual_nodes([(1, 0, 10, 1000, 5000)])
    eng.receive_virtual_nodes([(1, 7, 70)])
    eng.run(400)
    node, _, _ = eng.placements()
    assert (node == 0).all()  # 250 jobs run on row 0 {750, 99750}: 8 Foreign jobs need 258 slots of 256
    # {1000, 0}: |1000 - 750| = 250 leaves 750, |750 - 32| leaves 32, then every row leaves 32: 8 rows, never exhausted
    r2, s2 = eng.provide_virtual_nodes([(0, 1, 1000, 0, 5000)])
    return r1, s1, r2, s2


def test_provide_escalates_and_replays():
    arrays, streams = piled_system()
    with ext_session(arrays, streams) as eng:
        r1, s1, r2, s2 = piled_calls(eng)
        info = eng.trade_session_info()
        assert info["restarts"] == 1 and s2["replayed"] == 1 and s1["replayed"] == 0
        assert (int(r1["visited"][0]), int(r2["visited"][0]), int(r2["ok"][0])) == (1, 8, 0)
        got, rows = state(eng), [x.tobytes() for x in eng.trade_session_nodes(0)]
        f = eng.foreign()  # the earlier grants were re-applied: their record and their row are there
        assert len(f) == 9 and (int(f["start"][0]), int(f["responder"][0])) == (99, 1)
        assert (f["start"][1:] == 399).all() and list(f["node"][1:]) == list(range(8))
        assert eng.virtual_node_caps(1) == [(7, 70)]
    with ext_session(arrays, streams, slot_pool=6) as eng:  # a session started with the larger pool
        q1, _, q2, t2 = piled_calls(eng)
        assert eng.trade_session_info()["restarts"] == 0 and t2["replayed"] == 0
        assert q1.tobytes() == r1.tobytes() and q2.tobytes() == r2.tobytes()
        states_equal(got, state(eng), "escalated")
        assert rows == [x.tobytes() for x in eng.trade_session_nodes(0)]


def test_receive_escalates_and_keeps_the_rows():
    arrays, streams = piled_system()
    with ext_session(arrays, streams) as eng:
        eng.run(50)
        first = [(1, i, 10 * i) for i in range(60)]
        assert eng.receive_virtual_nodes(first)["replayed"] == 0
        eng.run(60)
        more = [(1, 100 + i, i) for i in range(10)]
        st = eng.receive_virtual_nodes(more)  # 70 rows: the pool of 64 grows
        assert st["replayed"] == 1 and eng.trade_session_info()["restarts"] == 1
        assert eng.virtual_node_caps(1) == [(c, m) for _, c, m in first + more]
        assert len(eng.trade_session_nodes(1)[0]) == 2 + 70
        assert eng.virtual_nodes()[1] == 70


def test_fixed_pool_and_the_257th_node():
    arrays, streams = piled_system()
    with ext_session(arrays, streams, slot_pool=4) as eng:  # 256 slots, fixed
        eng.run(100)
        eng.provide_virtual_nodes([(1, 0, 10, 1000, 5000)])
        eng.run(400)
        assert "capacity" in raises(L.MCS_E_CAPACITY, eng.provide_virtual_nodes, [(0, 1, 1000, 0, 5000)])
        assert eng.trade_session_info()["failed"] == 1
        assert "failed" in raises(L.MCS_E_STATE, eng.run, 500)
        assert "failed" in raises(L.MCS_E_STATE, eng.provide_virtual_nodes, [(0, 1, 1, 1, 1)])
        assert "failed" in raises(L.MCS_E_STATE, eng.receive_virtual_nodes, [(1, 1, 1)])
        eng.rewind()
        eng.run(100)
        res, st = eng.provide_virtual_nodes([(1, 0, 10, 1000, 5000)])
        assert len(eng.foreign()) == st["foreign_added"] == int(res["visited"][0])  # an empty grant log
        assert eng.trade_session_info()["restarts"] == 0
    with ext_session(arrays, streams) as eng:
        eng.run(10)
        st = eng.receive_virtual_nodes([(1, i, i) for i in range(256)])
        assert st["replayed"] == 1 and len(eng.virtual_node_caps(1)) == 256
        assert "capacity" in raises(L.MCS_E_CAPACITY, eng.receive_virtual_nodes, [(1, 1, 1)])
        assert eng.trade_session_info()["failed"] == 1


# ---- 7. the cursor ------------------------------------------------------------------------------------------
def test_cursor_across_grants():
    arrays, streams, t_max = system("small4")
    plan = replay_plan(oracle("small4"))[:40]
    P = 5
    with ext_session(arrays, streams, t_max) as eng:
        eng.run(0)  # the session begins; no tick yet
        eng.trade_stream_open(0, P, True, with_level1=True)
        cur = dict(t=0, seen=0, last=None, rebuilt=0, wrote=0)

        def take(tag):
            info = eng.trade_session_info()
            F = max(info["t_horizon"], info["t_last"] + 1 if info["ticks_total"] else 0)
            n = (F - cur["t"] + P - 1) // P if F > cur["t"] else 0
            s, w, l1, st = eng.trade_stream_next(max(n, 1))
            assert st["n_written"] == n, (tag, st)
            if n:
                ws, ww, _ = eng.trade_session_state_series(cur["t"], P, n)
                wl = eng.trade_session_level1_series(cur["t"], P, n)
                assert_state_equal(s, ws, tag)
                assert_bits_equal(w, ww, tag)
                assert l1.tobytes() == wl.tobytes(), tag
                nf = len(eng.foreign())
                if st["rebuilt"]:
                    cur["seen"] = 0
                assert st["foreign_scanned"] == nf - cur["seen"], (tag, st)  # the grants' records included
                cur.update(seen=nf, last=(cur["t"], n, s, w, l1), t=cur["t"] + n * P, wrote=cur["wrote"] + 1)
                cur["rebuilt"] += st["rebuilt"]
            return st

        def unchanged(tag):
            if cur["last"]:
                t, n, s, w, l1 = cur["last"]
                ws, ww, _ = eng.trade_session_state_series(t, P, n)
                assert_state_equal(s, ws, tag)
                assert_bits_equal(w, ww, tag)
                assert l1.tobytes() == eng.trade_session_level1_series(t, P, n).tobytes(), tag

        for t, rounds, nodes in plan:
            eng.run(t + 1)
            take(f"run {t + 1}")
            reqs = [r for _, _, _, rq in rounds for r in rq]
            if reqs:
                eng.provide_virtual_nodes([(r["responder"], r["requester"], r["cores"], r["memory"], r["time_s"])
                                           for r in reqs])
                unchanged(f"provide at {t}")
                take(f"provide at {t}")
            if nodes:
                eng.receive_virtual_nodes(nodes)
                unchanged(f"receive at {t}")
                take(f"receive at {t}")
        assert cur["rebuilt"] == 1 and cur["wrote"] > 10  # the first call that wrote samples, nothing since
        st = eng.receive_virtual_nodes([(0, 0, 0)] * 70)  # the pool of 64 virtual nodes grows: a replay
        assert st["replayed"] == 1
        unchanged("replay")
        eng.run(plan[-1][0] + 40)
        assert take("after the replay")["rebuilt"] == 1
        eng.run(plan[-1][0] + 80)
        assert take("later")["rebuilt"] == 0


# ---- 8. refusals ----------------------------------------------------------------------------------------------
def test_refusals():
    arrays, streams, _ = system("small4")
    one = [(0, 1, 1, 1, 1)]
    # external mode: what it needs
    # (cfg.borrow under MCS_POLICY_DELAY is refused by mcs_engine_create already)
    raises(L.MCS_E_INVALID, Engine, 0, policy="DELAY", trader=True, borrow=True)
    for cfg in (dict(policy="FIFO", trader=True), dict(policy="FIFO", borrow=True), dict(policy="DELAY")):
        with Engine(0, **cfg) as eng:
            eng.load_clusters(arrays)
            assert "MCS_POLICY_DELAY" in raises(L.MCS_E_STATE, eng.trade_external, True)
    with Engine(0, policy="DELAY", trader=True) as eng:
        eng.load_clusters(arrays)
        eng.set_shard(0, 2)
        assert "world 1" in raises(L.MCS_E_STATE, eng.trade_external, True)
    with Engine(0, policy="DELAY", trader=True) as eng:
        eng.load_clusters(arrays)
        eng.submit_jobs(streams)
        eng.trade_begin()
        assert "caller-driven" in raises(L.MCS_E_STATE, eng.trade_external, True)
    # an engine that never enabled external mode behaves as before; the grants need the switch
    with ext_session(arrays, streams, external=False) as eng:
        assert "no trading session" in raises(L.MCS_E_STATE, eng.provide_virtual_nodes, one)
        assert "no trading session" in raises(L.MCS_E_STATE, eng.trade_session_nodes, 0)
        eng.run(100)
        assert "external" in raises(L.MCS_E_STATE, eng.provide_virtual_nodes, one)
        assert "external" in raises(L.MCS_E_STATE, eng.receive_virtual_nodes, [(0, 1, 1)])
        assert len(eng.trade_session_nodes(0)[0]) == arrays.node_off[1] + len(eng.virtual_node_caps(0))  # either mode
        assert "tick" in raises(L.MCS_E_STATE, eng.trade_external, True)  # a tick has run
        eng.rewind()
        eng.trade_external(True)  # right after mcs_rewind
        eng.run(100)
        eng.provide_virtual_nodes(one)
        assert "tick" in raises(L.MCS_E_STATE, eng.trade_external, False)
    with ext_session(arrays, streams) as eng:
        eng.run(0)  # a session without a tick
        assert "no tick" in raises(L.MCS_E_STATE, eng.provide_virtual_nodes, one)
        assert "no tick" in raises(L.MCS_E_STATE, eng.receive_virtual_nodes, [(0, 1, 1)])
        assert "no tick" in raises(L.MCS_E_STATE, eng.trade_session_nodes, 0)
        eng.run(100)
        C = arrays.n_clusters
        res, st = eng.provide_virtual_nodes([])  # n == 0 is MCS_OK
        assert len(res) == 0 and st["n"] == 0 and eng.receive_virtual_nodes([])["n"] == 0
        assert "4096" in raises(L.MCS_E_INVALID, eng.provide_virtual_nodes, one * 4097)
        assert "4096" in raises(L.MCS_E_INVALID, eng.receive_virtual_nodes, [(0, 1, 1)] * 4097)
        assert "range" in raises(L.MCS_E_INVALID, eng.provide_virtual_nodes, [(C, 0, 1, 1, 1)])
        assert "range" in raises(L.MCS_E_INVALID, eng.provide_virtual_nodes, [(0, C, 1, 1, 1)])
        assert "range" in raises(L.MCS_E_INVALID, eng.receive_virtual_nodes, [(C, 1, 1)])
        assert "0xFFFFFFFE" in raises(L.MCS_E_INVALID, eng.provide_virtual_nodes, [(0, 1, 1, 1, 0xFFFFFFFE - 50)])
        assert "range" in raises(L.MCS_E_INVALID, eng.trade_session_nodes, C)
        rc = L.lib().mcs_trade_session_provide_vnodes(eng._h, None, 1, None, None)
        assert rc == L.MCS_E_INVALID
        assert L.lib().mcs_trade_session_receive_vnodes(eng._h, None, 1, None) == L.MCS_E_INVALID
        assert len(eng.foreign()) == 0  # nothing refused left a record
        # the setting survives mcs_rewind and mcs_submit_jobs; mcs_load_clusters resets it
        eng.rewind()
        eng.run(50)
        eng.provide_virtual_nodes(one)
        eng.submit_jobs(streams)
        eng.run(50)
        eng.provide_virtual_nodes(one)
        assert len(eng.foreign()) == 1  # the grant log started over with the jobs
        eng.load_clusters(arrays)
        eng.submit_jobs(streams)
        eng.run(50)
        assert "external" in raises(L.MCS_E_STATE, eng.provide_virtual_nodes, one)


def test_log_overflow_refuses_further_grants(monkeypatch):
    """Beyond foreign_cap the records are counted and MCS_FLAG_LOG_OVERFLOW is set, as the batch run does;
    the next grant is refused, as the series calls refuse such a run."""
    monkeypatch.setenv("MCS_DTRADE_FOREIGN_LOG_CAP", "3")
    arrays, streams, _ = system("small4")
    with ext_session(arrays, streams) as eng:
        eng.run(100)
        res, st = eng.provide_virtual_nodes([(0, 1, 32, 24000, 0), (1, 0, 32, 24000, 0), (2, 0, 1, 1, 0), (3, 0, 1, 1, 0)])
        assert st["foreign_added"] == int(res["visited"].sum()) > 3
        assert len(eng.foreign()) == st["foreign_added"]  # (the reader reports the count: the rest is counted)
        assert eng.trade_stats()["flags"] & L.MCS_FLAG_LOG_OVERFLOW
        assert "log" in raises(L.MCS_E_STATE, eng.provide_virtual_nodes, [(0, 1, 1, 1, 1)])
