"""The reference of the external traders' calls (mcs_trade_external, mcs_trade_session_provide_vnodes,
mcs_trade_session_receive_vnodes; include/mcs_trade.h, DESIGN.md §14 "External traders"), pinned on the
CPU oracle alone.

The reference is the oracle's own trading run, replayed from outside.  O.dtrade_run (built-in traders)
logs every round and every Foreign job; the responders a round's ProvideVirtualNode reached are the
distinct responders of the Foreign records with that start and requester, in log order; for a {0, 0}
contract no Foreign job exists and the winner alone is reached.  replay_plan() turns the logs into the
calls an outside trader makes, tick by tick, with what every call must answer; the GPU test
(tests/test_gpu_dtrade_external.py) issues them.  This file checks the rule on the oracle: the list of a
round has `failed` entries when nobody won and `failed + 1` entries ending in the winner otherwise, no
responder twice, no two rounds at one (t, requester); and that the systems contain every kind of grant,
so the GPU test cannot go vacuous.  It also pins the tick independence the forced last tick relies on,
and that libmcs.so exports the new symbols."""
import ctypes
import json
import os

import numpy as np
import pytest

import oracle_ref as O
from kat_util import GOLDEN, fuzz_workload, seeded_workload
from test_dtrade_oracle import dt_system

DT = json.load(open(os.path.join(GOLDEN, "kats_dtrade.json")))["dtrade"]
SYSTEMS = [k["name"] for k in DT] + ["fuzz", "small4", "small8", "big8"]
_SYS = {}


def system(name):
    """(arrays, streams, t_max) of a named system, built once"""
    if name not in _SYS:
        if name == "fuzz":  # the system of tests/test_gpu_dtrade_session.py
            _SYS[name] = (*fuzz_workload("w16s", 2, n_clusters=4, J=900, blocking=False), 0xFFFFFFFE)
        elif name in ("small4", "small8", "big8"):
            kind, c, j = {"small4": ("small", 4, 120), "small8": ("small", 8, 300), "big8": ("big", 8, 800)}[name]
            arrays, streams, _ = seeded_workload(kind, c, j)
            _SYS[name] = (arrays, streams, 0xFFFFFFFE)
        else:
            k = [x for x in DT if x["name"] == name][0]
            _SYS[name] = (*dt_system(k), k["t_max"])
    return _SYS[name]


_ORACLE = {}


def oracle(name):
    """the oracle's run with built-in traders, computed once and never modified"""
    if name not in _ORACLE:
        arrays, streams, t_max = system(name)
        _ORACLE[name] = O.dtrade_run(arrays, streams, t_max=t_max)
    return _ORACLE[name]


def replay_plan(o):
    """The oracle's trading run as an outside trader's calls: [(t, requests, nodes)] by ascending tick,
    rounds = [(requester, failed, winner, requests)] in requester order with requests = [dict(responder,
    requester, cores, memory, time_s, ok, visited)] in pop order, nodes = [(cluster, cores, memory)] of the
    winners in requester order.  (What remained of a failed request is not in the log, and the records do
    not determine it: a wrapped counter's difference rounds to 2^64 and is logged as uint 0, as an exact fit
    is.  walk() below computes it from the rows.)"""
    foreign = o["foreign"]
    plan = {}
    for tr in o["trades"]:
        t, q, win = int(tr["t"]), int(tr["requester"]), int(tr["winner"])
        kc, km, ks = int(tr["cores"]), int(tr["mem"]), int(tr["time_s"])
        recs = foreign[(foreign["start"] == t) & (foreign["requester"] == q)]
        reached = []
        for r in recs["responder"]:
            if int(r) not in reached:
                reached.append(int(r))
        if kc == 0 and km == 0 and win >= 0:
            assert len(recs) == 0
            reached = [win]
        reqs = []
        for r in reached:
            mine = recs[recs["responder"] == r]
            assert list(mine["node"]) == list(range(len(mine))), "the visited rows are a prefix"
            reqs.append(dict(responder=r, requester=q, cores=kc, memory=km, time_s=ks, ok=int(r == win),
                             visited=len(mine)))
        slot = plan.setdefault(t, ([], []))
        slot[0].append((q, int(tr["failed"]), win, reqs))
        if win >= 0:
            slot[1].append((q, kc, km))
    out = []
    for t in sorted(plan):
        rounds, nodes = plan[t]
        assert [r[0] for r in rounds] == sorted(r[0] for r in rounds), "rounds run in requester order"
        out.append((t, rounds, nodes))
    return out


def walk(free_c, free_m, rc, rm):
    """AllocateVirtualNodeResources over rows of Go uint64 counters (cluster.go:87-125) in Python's float64:
    (ok, visited, left_cores, left_memory, [(uint(core_diff), uint(mem_diff))], free_c', free_m')"""
    def go_u64(x):  # Go's float64 -> uint conversion on amd64 (oracle/mcs_oracle.c)
        if x < 2.0 ** 63:
            return int(x)
        y = x - 2.0 ** 63
        return 0 if y >= 2.0 ** 63 else int(y) ^ (1 << 63)

    fc, fm = [int(x) for x in free_c], [int(x) for x in free_m]
    jobs = []
    for i in range(len(fc)):
        if rc == 0 and rm == 0:
            break
        md = abs(float(rm) - float(fm[i])) if rm > 0 else 0.0
        cd = abs(float(rc) - float(fc[i])) if rc > 0 else 0.0
        rm = 0 if md > float(rm) else rm - int(md)
        rc = 0 if cd > float(rc) else rc - int(cd)
        jobs.append((go_u64(cd), go_u64(md)))
        fc[i] = (fc[i] - jobs[-1][0]) % (1 << 64)
        fm[i] = (fm[i] - jobs[-1][1]) % (1 << 64)
    return int(rc == 0 and rm == 0), len(jobs), rc, rm, jobs, fc, fm


def test_walk_equals_the_oracle():
    rng = np.random.default_rng(5)
    for _ in range(400):
        n = int(rng.integers(0, 9))
        fc = rng.integers(0, 70, n).astype(np.uint64)
        fm = rng.integers(0, 40000, n).astype(np.uint64)
        for i in range(n):  # some counters an earlier Foreign job wrapped
            if rng.random() < 0.2:
                fc[i] = np.uint64((1 << 64) - int(rng.integers(1, 50)))
            if rng.random() < 0.2:
                fm[i] = np.uint64((1 << 64) - int(rng.integers(1, 9000)))
        rc, rm = int(rng.integers(0, 200)), int(rng.integers(0, 50000))
        err, ofc, ofm, ojobs = O.allocate_virtual_node(fc, fm, rc, rm)
        ok, visited, lc, lm, jobs, wfc, wfm = walk(fc, fm, rc, rm)
        assert ok == (err == 0) and visited == len(ojobs)
        assert [(i, c, m) for i, (c, m) in enumerate(jobs)] == ojobs
        assert wfc == [int(x) for x in ofc] and wfm == [int(x) for x in ofm]
        assert ok == int(lc == 0 and lm == 0)


@pytest.mark.parametrize("name", SYSTEMS)
def test_replay_rule_on_the_oracle(name):
    o = oracle(name)
    assert o["n_foreign"] == len(o["foreign"]) and o["n_trades"] == len(o["trades"])
    seen = set()
    n_records = 0
    for t, rounds, nodes in replay_plan(o):
        for q, failed, win, reqs in rounds:
            assert (t, q) not in seen, "two rounds at one (t, requester)"
            seen.add((t, q))
            resp = [r["responder"] for r in reqs]
            assert len(set(resp)) == len(resp), "a responder twice in one round"
            if win < 0:
                assert len(resp) == failed
                assert not any(r["ok"] for r in reqs)
            else:
                assert len(resp) == failed + 1 and resp[-1] == win
                assert [r["ok"] for r in reqs] == [0] * failed + [1]
            n_records += sum(r["visited"] for r in reqs)
    assert n_records == o["n_foreign"], "every Foreign record belongs to one round's request"


def census(o, arrays):
    """what kinds of grants a system's replay holds"""
    plan = replay_plan(o)
    reqs = [r for _, rounds, _ in plan for _, _, _, rq in rounds for r in rq]
    n_phys = np.diff(arrays.node_off)
    return dict(won=sum(1 for _, rounds, _ in plan for r in rounds if r[2] >= 0),
                failed_allocs=sum(1 for r in reqs if not r["ok"] and r["visited"]),
                zero=sum(1 for r in reqs if r["cores"] == 0 and r["memory"] == 0),
                on_virtual=int((o["foreign"]["node"] >= n_phys[o["foreign"]["responder"]]).sum()),
                time0=int((o["foreign"]["finish"] == o["foreign"]["start"]).sum()))


def test_the_systems_hold_every_kind_of_grant():
    c = {name: census(oracle(name), system(name)[0]) for name in SYSTEMS}
    for name in ("KAT2", "KAT3", "KAT4", "KAT5", "KAT6a", "fuzz", "small4", "small8", "big8"):
        if name in c:
            assert c[name]["won"] > 0, name
    assert sum(v["won"] for v in c.values()) > 0
    for name in ("KAT1", "KAT3", "KAT6b"):
        if name in c:
            assert c[name]["failed_allocs"] > 0, name
    assert sum(v["failed_allocs"] for v in c.values()) > 0
    assert c["fuzz"]["zero"] > 0 and c["big8"]["zero"] > 0
    assert c["big8"]["on_virtual"] > 0
    assert c["big8"]["time0"] > 0


@pytest.mark.parametrize("name", SYSTEMS)
def test_ticks_decide_nothing_without_queued_jobs(name):
    """The forced last tick of external mode: a tick in a second in which nothing is queued does releases
    and samples only.  The system without traders returns the same placements and wait statistics with a
    tick every second (sample_period_s = 1) as with the sample period 5."""
    arrays, streams, t_max = system(name)
    a = O.dtrade_run(arrays, streams, t_max=t_max, trader=False)
    b = O.dtrade_run(arrays, streams, t_max=t_max, trader=False, sample_period_s=1)
    for f in ("node", "start", "finish"):
        np.testing.assert_array_equal(a[f], b[f], err_msg=f)
    for f in ("total_wait_ms", "jobs_count", "moved_l1", "placed_l1"):
        np.testing.assert_array_equal(a["stats"][f], b["stats"][f], err_msg=f)
    assert a["n_trades"] == 0 and a["n_foreign"] == 0


def test_the_library_exports_the_external_traders_calls():
    from mcs_amd import LIB_PATH

    lib = ctypes.CDLL(LIB_PATH)
    for sym in ("mcs_trade_external", "mcs_trade_session_provide_vnodes", "mcs_trade_session_receive_vnodes",
                "mcs_trade_session_read_nodes"):
        assert hasattr(lib, sym), sym
