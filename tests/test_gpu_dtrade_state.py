"""GPU parity of mcs_dtrade_state_series: the ClusterState record, its time series and the wait
statistics after a DELAY trading run (csrc/mcs_state.hip dt_state_kernel / dt_series_kernel, the
wait_*_kernels of csrc/mcs_wait.hip).

Every test first asserts that the engine's run equals the oracle's (placements, Foreign log, virtual
nodes), then compares the samples bit for bit (NaNs equal) with tests/dtrade_state_ref.py, the
brute-force reference over the run's public outputs, which tests/test_dtrade_state_ref.py pins with
hand-traced records.  The wait statistics are compared with tests/wait_ref.py's replay of the Go loop
over the run's start seconds."""
import json
import os

import numpy as np
import pytest

import dtrade_state_ref as D
import oracle_ref as O
import wait_ref as W
from kat_util import GOLDEN, REPO, fuzz_workload, seeded_workload
from mcs_amd import WAIT_SAMPLE_DTYPE, Engine, MCSError
from mcs_amd import _lib as L
from mcs_amd.shard import run_lockstep
from test_dtrade_oracle import DT, dt_system

pytestmark = pytest.mark.gpu

STATE_KATS = {g["name"]: g for g in json.load(open(os.path.join(GOLDEN, "kats_dtrade_state.json")))["kats"]}


def dt_engine(arrays, streams, **cfg):
    eng = Engine(0, policy="DELAY", trader=True, **cfg)
    eng.load_clusters(arrays)
    eng.submit_jobs(streams)
    return eng


def assert_run_is_the_oracles(eng, arrays, o):
    node, start, fin = eng.placements()
    for got, key in ((node, "node"), (start, "start"), (fin, "finish")):
        np.testing.assert_array_equal(got, o[key], err_msg=key)
    f = eng.foreign()
    assert len(f) == o["n_foreign"]
    for key in ("requester", "responder", "node", "start", "finish", "c", "m"):
        np.testing.assert_array_equal(f[key], o["foreign"][key], err_msg=key)
    assert [eng.virtual_node_caps(c) for c in range(arrays.n_clusters)] == o["vnodes"]
    assert eng.trade_stats()["t_final"] == o["t_final"]


def assert_samples_equal(got, want, tag=""):
    bad = np.nonzero((D.bits(got) != D.bits(want)).any(-1))
    assert len(bad[0]) == 0, f"{tag}: {len(bad[0])} samples differ, first (cluster, k) " \
                             f"{[(int(c), int(k), got[c, k], want[c, k]) for c, k in zip(*bad)][:3]}"


def wait_want(streams, o, t0, period, n, max_wait=10, clusters=None):
    """wait_ref's replay of every cluster (or of `clusters`, the other rows stay zero) over the run's
    start seconds, continued past the run's end."""
    T = t0 + (n - 1) * period
    out = np.zeros((len(streams.job_off) - 1, n), WAIT_SAMPLE_DTYPE)
    for c in range(out.shape[0]) if clusters is None else clusters:
        js = streams.of(c)
        rep = W.replay(streams.arrival[js], o["start"][js], max_wait, T)
        out["total_wait_ms"][c], out["jobs_count"][c] = W.samples(rep, t0, period, n)
    out["average_wait_time"] = W.average(out["total_wait_ms"], out["jobs_count"])
    return out


def assert_wait_equal(got, want):
    for f in ("total_wait_ms", "jobs_count"):
        np.testing.assert_array_equal(got[f], want[f], err_msg=f)
    np.testing.assert_array_equal(got["average_wait_time"].view(np.uint64), want["average_wait_time"].view(np.uint64))


# ---- 1. ("small", 4, 120): every second, the reference cadence, the cross-check, chunking -----------
@pytest.fixture(scope="module")
def run_s():
    arrays, streams, _ = seeded_workload("small", 4, 120)
    o = O.dtrade_run(arrays, streams)
    f = o["foreign"]
    assert ((f["c"] >= 2 ** 32) | (f["m"] >= 2 ** 32)).any()  # a wrapped Go uint in the log
    n = max(int(o["t_final"]), int(f["finish"].max())) + 6  # [0, last event + 5]
    ref = D.series_ref(arrays, streams, o, 0, 1, n)
    assert ((ref["cores_utilization"] < 0) | (ref["memory_utilization"] < 0)).sum() > 100
    with dt_engine(arrays, streams) as eng:
        eng.run()
        assert_run_is_the_oracles(eng, arrays, o)
        yield eng, arrays, streams, o, n, ref


def test_every_second(run_s):
    eng, arrays, streams, o, n, ref = run_s
    samples, wait, first = eng.dtrade_state_series(0, 1, n)
    assert_samples_equal(samples, ref, "every second")
    assert_wait_equal(wait, wait_want(streams, o, 0, 1, n))
    T = int(o["t_final"])
    ds = eng.delay_stats()
    np.testing.assert_array_equal(wait["total_wait_ms"][:, T], ds["total_wait_ms"])
    np.testing.assert_array_equal(wait["jobs_count"][:, T], ds["jobs_count"])
    assert (first["t_s"] == 0).all() and (first["total_cpu"] == 160).all() and (first["total_memory"] == 120000).all()


def test_reference_cadence(run_s):
    eng, arrays, streams, o, n, ref = run_s
    samples, wait, first = eng.dtrade_state_series(0, 5, (n + 4) // 5)
    assert_samples_equal(samples, ref[:, ::5], "period 5")
    assert_wait_equal(wait, wait_want(streams, o, 0, 5, (n + 4) // 5))
    samples, wait, first = eng.dtrade_state_series(3, 7, (n - 3) // 7, with_wait=False)
    assert wait is None
    assert_samples_equal(samples, ref[:, 3::7][:, :(n - 3) // 7], "t0 3, period 7")


def test_series_equals_the_plain_scan(run_s):
    """Sample k of the tile walk equals `first` (dt_state_kernel, a plain scan) of a call at t_k."""
    eng, arrays, streams, o, n, ref = run_s
    samples, _, _ = eng.dtrade_state_series(0, 1, n, with_wait=False)
    f = o["foreign"]
    ks = sorted(set(range(0, n, 397)) | {int(f["start"][0]), int(f["start"][0]) + 1, int(f["finish"].max()) - 1,
                                         int(f["finish"].max()), n - 1})
    for k in ks:
        one, _, first = eng.dtrade_state_series(k, 1, 1, with_wait=False)
        assert one[:, 0].tobytes() == samples[:, k].tobytes(), k
        assert first["cores_utilization"].tobytes() == samples["cores_utilization"][:, k].tobytes(), k
        assert first["memory_utilization"].tobytes() == samples["memory_utilization"][:, k].tobytes(), k
        assert (first["running"] == samples["running"][:, k]).all() and (first["t_s"] == k).all(), k


def test_chunks_give_the_same_bytes(run_s, monkeypatch):
    eng, arrays, streams, o, n, ref = run_s
    whole = eng.dtrade_state_series(0, 5, n // 5)
    monkeypatch.setenv("MCS_SERIES_CHUNK", "131")  # splits the samples, and not on a tile edge
    parts = eng.dtrade_state_series(0, 5, n // 5)
    for a, b in zip(whole, parts):
        assert a.tobytes() == b.tobytes()


# ---- 2. the hand-traced KATs ------------------------------------------------------------------------
@pytest.mark.parametrize("k", DT, ids=[k["name"] for k in DT])
def test_kats(k):
    """All seven DT-KATs against the reference; the four with hand-traced records (DT-KAT2, 4, 5, 6b)
    against those too.  DT-KAT6b is cut by t_max with two undecided jobs: they stay queued and their
    wait share grows past the end."""
    arrays, s = dt_system(k)
    o = O.dtrade_run(arrays, s, t_max=k["t_max"])
    g = STATE_KATS.get(k["name"])
    n = g["n"] if g else max(int(o["t_final"]), int(o["foreign"]["finish"].max()) if o["n_foreign"] else 0) + 6
    with dt_engine(arrays, s, t_max_s=k["t_max"]) as eng:
        eng.run()
        assert_run_is_the_oracles(eng, arrays, o)
        samples, wait, first = eng.dtrade_state_series(0, 1, n)
        ds = eng.delay_stats()
    assert_samples_equal(samples, D.series_ref(arrays, s, o, 0, 1, n), k["name"])
    if g:
        assert_samples_equal(samples, D.golden_series(g, arrays.n_clusters, n), k["name"] + " golden")
    assert_wait_equal(wait, wait_want(s, o, 0, 1, n))
    T = int(o["t_final"])
    np.testing.assert_array_equal(wait["total_wait_ms"][:, T], ds["total_wait_ms"])
    if k["name"] == "DT-KAT6b":
        assert (o["node"][:2] == -1).all() and T == 740
        assert (samples["queued"][0] == 2).all() and (samples["running"][0] == 0).all()
        assert wait["total_wait_ms"][0, n - 1] == wait["total_wait_ms"][0, T] + 2 * 1000 * (n - 1 - T)


# ---- 3. larger systems at the reference cadence -----------------------------------------------------
def series_at_5(arrays, streams, o, eng, wait_clusters=None):
    """wait_clusters: the clusters whose wait statistics are replayed (the replay of a long Level1 list
    is slow on the host); every cluster's are checked against the run's own sums at t_final."""
    last = max(int(o["t_final"]), int(o["foreign"]["finish"].max()) if o["n_foreign"] else 0)
    n = last // 5 + 3
    samples, wait, first = eng.dtrade_state_series(0, 5, n)
    assert_samples_equal(samples, D.series_ref(arrays, streams, o, 0, 5, n))
    rows = list(range(arrays.n_clusters)) if wait_clusters is None else list(wait_clusters)
    assert_wait_equal(wait[rows], wait_want(streams, o, 0, 5, n, clusters=rows)[rows])
    T, ds = int(o["t_final"]), eng.delay_stats()
    if T % 5 == 0:
        np.testing.assert_array_equal(wait["total_wait_ms"][:, T // 5], ds["total_wait_ms"])
    one, _, f2 = eng.dtrade_state_series(5 * (n // 2), 5, 1, with_wait=False)
    assert one[:, 0].tobytes() == samples[:, n // 2].tobytes()
    assert f2["cores_utilization"].tobytes() == samples["cores_utilization"][:, n // 2].tobytes()
    return samples


def test_big_system():
    """("big", 8, 800): Foreign values past 2^32, hundreds of jobs on virtual rows and Foreign jobs on a
    responder's virtual rows."""
    arrays, streams, _ = seeded_workload("big", 8, 800)
    o = O.dtrade_run(arrays, streams)
    f = o["foreign"]
    nphys = np.diff(arrays.node_off)
    assert ((f["c"] >= 2 ** 32) | (f["m"] >= 2 ** 32)).sum() >= 2
    assert (o["node"] >= np.repeat(nphys, 800)).sum() > 500 and (f["node"] >= nphys[f["responder"]]).any()
    with dt_engine(arrays, streams) as eng:
        eng.run()
        assert_run_is_the_oracles(eng, arrays, o)
        series_at_5(arrays, streams, o, eng, wait_clusters=(0, 5))


@pytest.mark.parametrize("resident,form", [("1", 5), ("0", 0)])
@pytest.mark.parametrize("shape,seed", [("w16s", 1), ("w32", 15)])
def test_fuzz_systems_on_both_tick_forms(shape, seed, resident, form, monkeypatch):
    """w16s/1: clusters of up to 64 nodes; w32/15: 256 nodes, sums past 2^24 (the float32 row sum
    rounds) and 166 won trades, so wide tiles of N + V rows.  The resident tick and the replayed
    kernels leave the same record."""
    monkeypatch.setenv("MCS_DT_RESIDENT", resident)
    arrays, streams = fuzz_workload(shape, seed, n_clusters=8, J=300, blocking=False)
    o = O.dtrade_run(arrays, streams)
    assert (o["trades"]["winner"] >= 0).sum() >= 5
    with dt_engine(arrays, streams) as eng:
        eng.run()
        assert eng.trade_stats()["loop_form"] == form
        assert_run_is_the_oracles(eng, arrays, o)
        samples = series_at_5(arrays, streams, o, eng)
    assert samples["running"].max() > 0


def test_caller_driven_equals_run():
    arrays, streams, _ = seeded_workload("small", 4, 120)
    got = []
    for driven in (False, True):
        with dt_engine(arrays, streams) as eng:
            if driven:
                run_lockstep(eng, lambda b: b)
            else:
                eng.run()
            got.append(eng.dtrade_state_series(0, 5, 1000))
    for a, b in zip(*got):
        assert a.tobytes() == b.tobytes()
    assert got[0][0]["running"].max() > 0


# ---- 4. refusals ------------------------------------------------------------------------------------
def refused(eng, word, code=L.MCS_E_STATE, args=(0, 5, 10)):
    with pytest.raises(MCSError) as ei:
        eng.dtrade_state_series(*args)
    assert ei.value.code == code and word in str(ei.value), str(ei.value)


def test_refusals(monkeypatch):
    arrays, streams, _ = seeded_workload("small", 4, 120)
    with dt_engine(arrays, streams) as eng:
        refused(eng, "mcs_run first")  # before a run
        eng.run()
        refused(eng, "positive", L.MCS_E_INVALID, (0, 0, 10))
        refused(eng, "positive", L.MCS_E_INVALID, (0, 5, 0))
        refused(eng, "0xFFFFFFFE", L.MCS_E_INVALID, (0xFFFFFFF0, 5, 10))
        assert eng.dtrade_state_series(0xFFFFFFFE, 1, 1)[0]["running"].max() == 0
    with Engine(0, policy="DELAY") as eng:  # plain DELAY
        eng.load_clusters(arrays)
        eng.submit_jobs(streams)
        eng.run()
        refused(eng, "mcs_cluster_state_series")
    with Engine(0, policy="DELAY") as eng:  # after append_jobs
        eng.load_clusters(arrays)
        eng.append_jobs(streams)
        eng.run()
        refused(eng, "mcs_append_jobs")
    with Engine(0, borrow=True, trader=True, t_max_s=20_000_000) as eng:  # FIFO trading
        eng.load_clusters(arrays)
        eng.submit_jobs(streams)
        eng.run()
        refused(eng, "mcs_cluster_state_series")
    monkeypatch.setenv("MCS_DTRADE_FOREIGN_LOG_CAP", "8")  # the Foreign log drops records
    assert O.dtrade_run(arrays, streams)["n_foreign"] > 8
    with dt_engine(arrays, streams) as eng:
        eng.run()
        assert eng.trade_stats()["flags"] & 0x10  # MCS_FLAG_LOG_OVERFLOW
        refused(eng, "MCS_FLAG_LOG_OVERFLOW")


def test_mcs_h_calls_still_refuse_a_delay_trading_run(run_s):
    eng = run_s[0]
    for call in (lambda: eng.cluster_states(10), lambda: eng.cluster_state_series(0, 5, 10),
                 lambda: eng.wait_time_series(0, 5, 10)):
        with pytest.raises(MCSError) as ei:
            call()
        assert ei.value.code == L.MCS_E_STATE and "mcs_dtrade_state_series" in str(ei.value)


# ---- 5. the plain and TRADE instantiations stay the code they are -----------------------------------
def test_plain_and_fifo_trading_state_calls_return_the_recorded_bytes():
    """The plain FIFO, plain DELAY (with the wait series) and FIFO-trading state calls of one workload
    return the bytes recorded when mcs_dtrade_state_series was added, where they were equal to the
    parent build's (profiles/dtrade_state/byte_identity.json, tools/dtrade_state_bench.py bytes)."""
    import sys

    sys.path.insert(0, os.path.join(REPO, "tools"))
    try:
        import dtrade_state_bench as B
    finally:
        sys.path.pop(0)
    want = json.load(open(os.path.join(REPO, "profiles", "dtrade_state", "byte_identity.json")))
    assert all(want["equal"].values())
    got = B.state_bytes(None)
    assert {k: got[k] for k in want["sha256"]} == want["sha256"]
