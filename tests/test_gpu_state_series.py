"""GPU parity of the ClusterState time series (csrc/mcs_state.hip series_kernel,
mcs_cluster_state_series): every sample of every cluster from one call equals, bit for bit,
(1) a host reference built per sample from the oracle's placements — the oracle's
GetResourceUtilization (cluster.go:46-63, float32 in node order) over the rebuilt counters, running
and queued from plain numpy masks — and (2) the unchanged single call mcs_cluster_states at t_k."""
import ctypes as C

import numpy as np
import pytest

import oracle_ref as O
from kat_util import fuzz_workload, seeded_workload
from mcs_amd import CLUSTER_SAMPLE_DTYPE, ClusterArrays, Engine, GenParams, JobStreams, MCSError, replicate, \
    uniform_cluster
from mcs_amd import _lib as L
from mcs_amd.engine import scaled_lambda

pytestmark = pytest.mark.gpu

FIELDS = ("cores_utilization", "memory_utilization", "running")


def tile(n_nodes):
    """Samples per tile of a cluster (series_tile, csrc/mcs_internal.h): 2 N + 34 LDS rows in 78 KiB,
    at most 127, odd."""
    return (min(78 * 1024 // (4 * (2 * n_nodes + 34)), 127) - 1) | 1


def concat(parts):
    arrays = ClusterArrays(*(np.concatenate([getattr(a, f) for a, _ in parts]) for f in
                             ("cap_c", "cap_m", "free_c", "free_m")),
                           np.concatenate([parts[0][0].node_off] + [
                               sum(int(p[0].node_off[-1]) for p in parts[:i]) + p[0].node_off[1:]
                               for i, p in enumerate(parts) if i > 0]).astype(np.uint32))
    offs, base = [np.zeros(1, np.uint64)], 0
    for _, s in parts:
        offs.append(base + s.job_off[1:])
        base += int(s.job_off[-1])
    streams = JobStreams(*(np.concatenate([getattr(s, f) for _, s in parts]) for f in ("arrival", "dur", "cores", "mem")),
                         np.concatenate(offs).astype(np.uint64))
    return arrays, streams


def series_ref(arrays, streams, node, start, fin, t0, period, n):
    """Brute force per sample: the counters after second t_k, the oracle's utilization over them,
    and the two counts."""
    out = np.zeros((arrays.n_clusters, n), CLUSTER_SAMPLE_DTYPE)
    for c in range(arrays.n_clusters):
        ns, js = arrays.nodes_of(c), streams.of(c)
        nn = ns.stop - ns.start
        nd, st, fi = node[js], start[js].astype(np.int64), fin[js].astype(np.int64)
        arr = streams.arrival[js].astype(np.int64)
        cores, mem = streams.cores[js].astype(np.float64), streams.mem[js].astype(np.float64)
        for k in range(n):
            t = t0 + k * period
            run = (nd >= 0) & (st <= t) & (fi > t)
            uc = np.bincount(nd[run], weights=cores[run], minlength=nn).astype(np.uint64)
            um = np.bincount(nd[run], weights=mem[run], minlength=nn).astype(np.uint64)
            cu, mu = O.resource_utilization(arrays.cap_c[ns], arrays.cap_m[ns], arrays.free_c[ns].astype(np.uint64) - uc,
                                            arrays.free_m[ns].astype(np.uint64) - um)
            queued = (arr <= t) & ((nd < 0) | (st > t))
            out[c, k] = (np.float32(cu), np.float32(mu), int(run.sum()), int(queued.sum()))
    return out


def assert_samples_equal(got, want, tag=""):
    for f in CLUSTER_SAMPLE_DTYPE.names:
        bad = np.argwhere(got[f].view(np.uint32) != want[f].view(np.uint32))
        assert bad.size == 0, f"{tag} {f}: {len(bad)} samples differ, first (cluster, k) {bad[:4].tolist()}: " \
                              f"got {got[f][tuple(bad[0])]} want {want[f][tuple(bad[0])]}"


def assert_matches_single_call(eng, samples, t0, period, ks):
    for k in ks:
        one = eng.cluster_states(t0 + k * period)
        for f in FIELDS:
            bad = np.nonzero(samples[f][:, k].view(np.uint32) != one[f].view(np.uint32))[0]
            assert bad.size == 0, f"{f} at k={k} (t={t0 + k * period}), clusters {bad[:4].tolist()}"


def workload_a(policy):
    n256 = "n256_delay" if policy == "DELAY" else "n256"
    big = "n600_delay" if policy == "DELAY" else "n600"  # one tile is 15 samples: below a wave
    return concat([seeded_workload("small", 5, 700)[:2], seeded_workload("big", 3, 700)[:2],
                   seeded_workload(n256, 4, 1500)[:2], seeded_workload(big, 1, 1500)[:2]])


def oracle_run(policy, arrays, streams):
    run = O.fifo_run_batch if policy == "FIFO" else O.delay_run_batch
    return run(arrays, streams, n_threads=8)[:3]


@pytest.fixture(scope="module", params=["FIFO", "DELAY"])
def run_a(request):
    """Workload A run once per policy: (engine, arrays, streams, the oracle's node/start/finish)."""
    policy = request.param
    arrays, streams = workload_a(policy)
    node, start, fin = oracle_run(policy, arrays, streams)
    with Engine(0, policy=policy) as eng:
        eng.load_clusters(arrays)
        eng.submit_jobs(streams)
        eng.run()
        gn, gs, gf = eng.placements()
        np.testing.assert_array_equal(gn, node)
        np.testing.assert_array_equal(gs, start)
        np.testing.assert_array_equal(gf, fin)
        yield eng, arrays, streams, node, start, fin


def test_series_matches_host_reference(run_a):
    eng, arrays, streams, node, start, fin = run_a
    n = 200
    period = int(fin[node >= 0].max()) // (n - 5) + 1  # the series ends a few samples past the last finish
    assert (n - 1) * period > int(fin[node >= 0].max()) + 2 * period
    samples, first = eng.cluster_state_series(0, period, n)
    assert samples.shape == (arrays.n_clusters, n) and samples.dtype == CLUSTER_SAMPLE_DTYPE
    assert_samples_equal(samples, series_ref(arrays, streams, node, start, fin, 0, period, n))
    assert (samples["running"][:, -1] == 0).all() and (samples["queued"][:, -1] == 0).all()
    assert samples["running"].max() > 64 and samples["queued"].max() > 0


def test_series_matches_single_call_every_second(run_a):
    eng, arrays, streams, node, start, fin = run_a
    ts = max(tile(int(x)) for x in np.diff(arrays.node_off))
    n, t0 = 3 * ts + 7, int(np.median(start[node >= 0]))
    samples, first = eng.cluster_state_series(t0, 1, n)
    assert_matches_single_call(eng, samples, t0, 1, range(n))
    one = eng.cluster_states(t0)
    assert first.tobytes() == one.tobytes()
    # every arrival, start and finish second of the window is a sample: the counts move with them
    assert (np.diff(samples["running"].astype(np.int64), axis=1) != 0).any()


def test_series_matches_single_call_at_the_reference_cadence(run_a):
    eng, arrays, streams, node, start, fin = run_a
    period = 5
    n = int(fin[node >= 0].max()) // period + 8
    assert n > 400
    samples, first = eng.cluster_state_series(0, period, n)
    ks = set(range(0, n, 29))
    for ts in {tile(int(x)) for x in np.diff(arrays.node_off)}:  # each tile's first and last sample
        ks |= set(range(0, n, ts)) | set(range(ts - 1, n, ts))
    ks.add(n - 1)
    assert_matches_single_call(eng, samples, 0, period, sorted(ks))
    assert first.tobytes() == eng.cluster_states(0).tobytes()


def test_series_in_chunks_is_the_same_series(run_a, monkeypatch):
    """The engine may split the samples over several launches (MCS_SERIES_CHUNK samples each)."""
    eng = run_a[0]
    whole, _ = eng.cluster_state_series(3, 7, 150)
    monkeypatch.setenv("MCS_SERIES_CHUNK", "41")
    parts, _ = eng.cluster_state_series(3, 7, 150)
    assert parts.tobytes() == whole.tobytes()


def test_series_edges(run_a):
    eng, arrays, streams, node, start, fin = run_a
    t_mid = int(np.median(start[node >= 0]))
    # one sample: the single call
    samples, first = eng.cluster_state_series(t_mid, 3, 1)
    assert samples.shape[1] == 1
    assert_matches_single_call(eng, samples, t_mid, 3, [0])
    # past every finish: idle, nothing running, nothing queued (every job of workload A is placed)
    assert (node >= 0).all()
    t_end = int(fin.max())
    samples, first = eng.cluster_state_series(t_end, 11, 4)
    assert (samples["running"] == 0).all() and (samples["queued"] == 0).all()
    for c in range(arrays.n_clusters):
        ns = arrays.nodes_of(c)
        cu, mu = O.resource_utilization(arrays.cap_c[ns], arrays.cap_m[ns], arrays.free_c[ns], arrays.free_m[ns])
        assert (samples["cores_utilization"][c].view(np.uint32) == np.float32(cu).view(np.uint32)).all()
        assert (samples["memory_utilization"][c].view(np.uint32) == np.float32(mu).view(np.uint32)).all()
    # sample times at the top of the uint32 range, and a period of 2^31: no index arithmetic wraps
    for t0, period, n in ((0xFFFFFFF0, 7, 3), (5, 0x80000000, 2)):
        samples, first = eng.cluster_state_series(t0, period, n)
        assert_samples_equal(samples, series_ref(arrays, streams, node, start, fin, t0, period, n), f"t0 {t0:#x}")
        assert int(first["t_s"][0]) == t0


def test_series_with_an_empty_job_range():
    a1, s1, _ = seeded_workload("small", 1, 300)
    a2, s2, _ = seeded_workload("small", 2, 300, seed=77)
    nothing = JobStreams(*(np.zeros(0, np.uint32) for _ in range(4)), np.zeros(2, np.uint64))
    arrays, streams = concat([(a1, s1), (replicate(uniform_cluster(7), 1), nothing), (a2, s2)])
    assert streams.job_off.tolist() == [0, 300, 300, 600, 900]  # cluster 1 has no jobs
    with Engine(0, policy="FIFO") as eng:
        eng.load_clusters(arrays)
        eng.submit_jobs(streams)
        eng.run()
        node, start, fin = eng.placements()
        period = int(fin[node >= 0].max()) // 115 + 1
        samples, first = eng.cluster_state_series(0, period, 120)
        assert_samples_equal(samples, series_ref(arrays, streams, node, start, fin, 0, period, 120))
        assert (samples["running"][1] == 0).all() and (samples["queued"][1] == 0).all()
        assert samples["running"][[0, 2, 3]].max(axis=1).min() > 0


def test_series_keeps_unplaced_jobs_queued():
    """Workload B under FIFO: deadlocked clusters leave jobs unplaced; they stay queued for good."""
    arrays, streams = fuzz_workload("w16r", 3, n_clusters=24, J=600, blocking=True)
    assert (streams.dur == 0).any()
    node, start, fin = oracle_run("FIFO", arrays, streams)
    unplaced = np.array([(node[streams.of(c)] < 0).sum() for c in range(24)])
    assert (unplaced > 0).any()
    with Engine(0, policy="FIFO") as eng:
        eng.load_clusters(arrays)
        eng.submit_jobs(streams)
        eng.run()
        gn, gs, gf = eng.placements()
        np.testing.assert_array_equal(gn, node)
        np.testing.assert_array_equal(gs, start)
        np.testing.assert_array_equal(gf, fin)
        n = 160
        period = int(max(fin[node >= 0].max(), streams.arrival.max())) // (n - 4) + 1
        samples, first = eng.cluster_state_series(0, period, n)
        assert_samples_equal(samples, series_ref(arrays, streams, node, start, fin, 0, period, n))
        assert_matches_single_call(eng, samples, 0, period, range(0, n, 7))
        t = np.arange(n, dtype=np.int64) * period
        for c in np.nonzero(unplaced)[0]:
            js = streams.of(c)
            arrived = t >= streams.arrival[js][node[js] < 0].max()
            assert arrived.any() and (samples["queued"][c][arrived] >= unplaced[c]).all()
            assert samples["queued"][c][-1] == unplaced[c] and samples["running"][c][-1] == 0
        # past every finish: queued is the unplaced count, utilization the idle value
        late, _ = eng.cluster_state_series(int(t[-1]) + 1000, 1, 2)
        assert (late["queued"][:, 1] == unplaced).all() and (late["running"] == 0).all()
        assert late["cores_utilization"].tobytes() == np.repeat(samples["cores_utilization"][:, -1:], 2, 1).tobytes()


def test_series_of_a_fused_run_equals_the_materialised_stream():
    arrays = replicate(uniform_cluster(256), 4)
    got = []
    for fused in (True, False):
        gp = GenParams(seed=0x5EED, arrival_mode=1, lam=scaled_lambda(256, load=0.9), fused=fused)
        with Engine(0, policy="FIFO") as eng:
            eng.load_clusters(arrays)
            eng.generate_jobs(gp, 800)
            eng.run()
            got.append(eng.cluster_state_series(0, 5, 260))
            if not fused:
                streams = eng.read_jobs()
                node, start, fin = eng.placements()
    assert got[0][0].tobytes() == got[1][0].tobytes() and got[0][1].tobytes() == got[1][1].tobytes()
    assert got[0][0]["running"].max() > 0
    assert_samples_equal(got[0][0][:, ::13], series_ref(arrays, streams, node, start, fin, 0, 65, 20))


def test_series_refusals(run_a):
    eng, arrays = run_a[0], run_a[1]
    n = arrays.n_clusters
    out = np.zeros((n + 1, 4), CLUSTER_SAMPLE_DTYPE)
    po = out.ctypes.data_as(C.POINTER(L.mcs_cluster_sample))
    f = L.lib().mcs_cluster_state_series
    assert f(eng._h, 0, 5, 4, po, None, n, None) == L.MCS_OK
    assert f(eng._h, 0, 0, 4, po, None, n, None) == L.MCS_E_INVALID           # period_s == 0
    assert f(eng._h, 0, 5, 0, po, None, n, None) == L.MCS_E_INVALID           # n_samples == 0
    assert f(eng._h, 0, 5, 4, None, None, n, None) == L.MCS_E_INVALID         # out == NULL
    assert f(eng._h, 0, 5, 4, po, None, n + 1, None) == L.MCS_E_INVALID       # more clusters than the engine has
    assert f(eng._h, 0xFFFFFFFC, 1, 4, po, None, n, None) == L.MCS_E_INVALID  # last sample 0xFFFFFFFF
    assert f(eng._h, 0xFFFFFFFB, 1, 4, po, None, n, None) == L.MCS_OK         # last sample 0xFFFFFFFE
    assert f(eng._h, 3, 0x80000000, 3, po, None, n, None) == L.MCS_E_INVALID  # 3 + 2 * 2^31 wraps in 32 bits
    with pytest.raises(MCSError) as ei:
        eng.cluster_state_series(0, 0, 4)
    assert ei.value.code == L.MCS_E_INVALID


def test_series_refused_without_a_batch_run():
    arrays, streams, _ = seeded_workload("small", 3, 200)
    with Engine(0, policy="DELAY") as eng:  # before run()
        eng.load_clusters(arrays)
        eng.submit_jobs(streams)
        with pytest.raises(MCSError) as ei:
            eng.cluster_state_series(0, 5, 10)
        assert ei.value.code == L.MCS_E_STATE
    with Engine(0, policy="DELAY", trader=True) as eng:  # after a trader run
        eng.load_clusters(arrays)
        eng.submit_jobs(streams)
        eng.run()
        with pytest.raises(MCSError) as ei:
            eng.cluster_state_series(0, 5, 10)
        assert ei.value.code == L.MCS_E_STATE
    with Engine(0, policy="FIFO") as eng:  # after append_jobs
        eng.load_clusters(arrays)
        eng.append_jobs(streams)
        eng.run()
        with pytest.raises(MCSError) as ei:
            eng.cluster_state_series(0, 5, 10)
        assert ei.value.code == L.MCS_E_STATE
