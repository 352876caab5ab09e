"""CPU tests of tests/dtrade_state_ref.py, the host reference of the ClusterState record after a DELAY
trading run: pinned by the hand-traced records of tests/golden/kats_dtrade_state.json,
told from its four wrong readings on a seeded system, and checked for consistency against what the
oracle's traders did with the record (every contract follows from a sample that breaks its policy).
No GPU needed."""
import json
import os

import numpy as np
import pytest

import dtrade_state_ref as D
import oracle_ref as O
import wait_ref as W
from kat_util import GOLDEN, seeded_workload
from test_dtrade_oracle import DT, dt_system

STATE_KATS = json.load(open(os.path.join(GOLDEN, "kats_dtrade_state.json")))["kats"]


def test_float32_of_uint64_rounds_to_nearest_even():
    two64 = np.float32(2.0 ** 64)
    assert D.f32_of_u64(2 ** 64 - 33) == two64 and D.f32_of_u64(2 ** 64 - 1) == two64
    assert D.f32_of_u64(2 ** 64 - 2 ** 39) == two64  # a tie: the even neighbour is 2^64
    assert D.f32_of_u64(2 ** 64 - 2 ** 39 - 1) == np.float32(2.0 ** 64 - 2.0 ** 40)
    assert D.f32_of_u64((1 << 24) + 1) == np.float32(1 << 24) and D.f32_of_u64((1 << 24) + 3) == np.float32((1 << 24) + 4)
    assert D.f32_of_u64(18446744073709438976) == np.float32(18446744073709438976.0)
    for x in (0, 1, 24000, (1 << 24) - 1, 1 << 31, (1 << 32) - 17):
        assert D.f32_of_u64(x) == np.float32(x)


@pytest.mark.parametrize("g", STATE_KATS, ids=[g["name"] for g in STATE_KATS])
def test_reference_equals_the_hand_traced_records(g):
    k = [x for x in DT if x["name"] == g["name"]][0]
    arrays, s = dt_system(k)
    o = O.dtrade_run(arrays, s, t_max=k["t_max"])
    ref = D.series_ref(arrays, s, o, 0, 1, g["n"])
    want = D.golden_series(g, arrays.n_clusters, g["n"])
    bad = np.nonzero((D.bits(ref) != D.bits(want)).any(-1))
    assert len(bad[0]) == 0, [(int(c), int(t), ref[c, t], want[c, t]) for c, t in zip(*bad)][:3]
    # every fifth second, from another start: the same records
    assert D.bits(D.series_ref(arrays, s, o, 3, 5, 100)).tolist() == D.bits(want[:, 3:503:5]).tolist()


def test_the_fixtures_hold_the_cases_they_are_there_for():
    by = {g["name"]: g for g in STATE_KATS}
    assert {"DT-KAT2", "DT-KAT4", "DT-KAT5"} <= set(by)
    assert any(seg[2] < 0 for seg in by["DT-KAT5"]["segments"]["1"])  # a negative sample
    k4 = [x for x in DT if x["name"] == "DT-KAT4"][0]
    assert all(f[3] == f[4] for f in k4["foreign_first"]) and k4["n_foreign"] == 1  # a zero-duration Foreign job
    assert all(seg[4] == 0 for seg in by["DT-KAT4"]["segments"]["1"])  # ... which never runs


@pytest.fixture(scope="module")
def small4():
    arrays, streams, _ = seeded_workload("small", 4, 120)
    o = O.dtrade_run(arrays, streams)
    n = max(int(o["t_final"]), int(o["foreign"]["finish"].max())) + 6
    return arrays, streams, o, n, D.series_ref(arrays, streams, o, 0, 1, n)


@pytest.mark.parametrize("name,kw", [("non-strict Foreign start", dict(strict=False)),
                                     ("Foreign jobs left out", dict(with_foreign=False)),
                                     ("virtual rows left out", dict(with_vnodes=False)),
                                     ("counters truncated to uint32", dict(u32=True))])
def test_wrong_readings_differ(small4, name, kw):
    arrays, streams, o, n, ref = small4
    wrong = D.series_ref(arrays, streams, o, 0, 1, n, **kw)
    differ = int((D.bits(wrong) != D.bits(ref)).any(-1).sum())
    print(name, differ, "of", ref.size, "per-second samples differ")
    assert differ > 0


def test_the_seeded_system_wraps_counters(small4):
    arrays, streams, o, n, ref = small4
    assert ((ref["cores_utilization"] < 0) | (ref["memory_utilization"] < 0)).sum() > 100
    f = o["foreign"]
    assert ((f["c"] >= 2 ** 32) | (f["m"] >= 2 ** 32)).any()  # a Go uint past 32 bits
    assert (f["start"] == f["finish"]).any() and (f["finish"] > f["start"] + 1).any()
    nphys = np.repeat(np.diff(arrays.node_off), np.diff(streams.job_off).astype(np.int64))
    assert (o["node"] >= nphys).any()  # own jobs on virtual rows


def test_a_foreign_job_on_a_virtual_row():
    """A responder that received a virtual node earlier launches Foreign jobs on it too
    (AllocateVirtualNodeResources visits every node): ("big", 8, 800) has four such records, and the
    reference gives their row a term."""
    arrays, streams, _ = seeded_workload("big", 8, 800)
    o = O.dtrade_run(arrays, streams)
    f = o["foreign"]
    nphys = np.diff(arrays.node_off)
    virt = f["node"] >= nphys[f["responder"]]
    on_v = f[virt & (f["finish"] > f["start"] + 1) & ((f["c"] > 0) | (f["m"] > 0))]
    assert len(on_v) > 0
    r = on_v[0]
    t0, n = int(r["start"]), int(r["finish"]) - int(r["start"]) + 1
    a = D.series_ref(arrays, streams, o, t0, 1, n)[int(r["responder"])]
    b = D.series_ref(arrays, streams, dict(o, foreign=f[~virt]), t0, 1, n)[int(r["responder"])]
    differ = (D.bits(a) != D.bits(b)).any(-1)
    assert not differ[0] and differ[1:-1].all()  # not yet held at the sample of its start tick


@pytest.mark.parametrize("kind,C,J", [("small", 4, 120), ("small", 8, 300)])
def test_every_contract_follows_from_a_sample_that_breaks_its_policy(kind, C, J):
    """The traders act on the ClusterState they received: the monitor checks WaitTime on a fresh sample
    and Utilization on the stale one (a sleep of 120 s or 240 s earlier).  For every contract of the
    oracle's run the reference's record at the latest sample tick at or before t - d, for some d in
    {0, 120, 240}, breaks the contract's policy: utilization above 0.8 (policy 1) or the replayed
    average wait above 600000 ms (policy 0)."""
    arrays, streams, _ = seeded_workload(kind, C, J)
    o = O.dtrade_run(arrays, streams)
    T = int(o["t_final"])
    ref = D.series_ref(arrays, streams, o, 0, 5, T // 5 + 1)
    avg = []
    for c in range(C):
        js = streams.of(c)
        rep = W.replay(streams.arrival[js], o["start"][js], 10, T)
        avg.append(W.average(rep["total_ms"], rep["count"]))
        st = o["stats"][c]
        assert int(rep["total_ms"][T]) == int(st["total_wait_ms"]) and int(rep["count"][T]) == int(st["jobs_count"])
    tr = o["trades"]
    assert len(tr) > 50 and set(np.unique(tr["policy"])) == {0, 1}
    for r in tr:
        q, t = int(r["requester"]), int(r["t"])
        ticks = [(t - d) // 5 * 5 for d in (0, 120, 240) if t - d >= 0]
        if r["policy"] == 1:
            ok = any(ref["cores_utilization"][q, k // 5] > np.float32(0.8) or
                     ref["memory_utilization"][q, k // 5] > np.float32(0.8) for k in ticks)
        else:
            ok = any(avg[q][k] > 600000.0 for k in ticks)
        assert ok, (q, t, int(r["policy"]))
