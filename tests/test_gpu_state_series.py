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


# ---- long streams: the batch cursor of series_kernel beyond one round of 256 summaries ----------
#
# Workload L, FIFO on cluster_small (5 nodes, tiles of 127 samples): arrivals about a second apart,
# durations of at most 30 s, so a batch of 256 jobs ends soon after its last arrival.  Cluster LONG has
# 3 * 65536 + 300 jobs, 769 batches: three full rounds and a fourth.  The streams before it have 300,
# and those between it and the next multi-batch cluster 255 and 257 jobs, so the multi-batch
# clusters start at job offsets that are no multiple of 256.  HOLD_0 and HOLD_300 repeat LONG's stream
# with one small job of duration 2^30 in batch 0 and in batch 300: that batch never ends, so the
# leading run of ended batches stops there in every tile.
L_JOBS = (300, 3 * 65536 + 300, 255, 257, 70000)
LONG, HOLD_0, HOLD_300 = 1, 5, 6
HOLD_BATCH = 300
BATCH, ROUND, GROUP = 256, 256, 8  # kSeriesBatch, kStateThreads, kGroup (csrc/mcs_state.hip)


def workload_l():
    rng = np.random.default_rng(0x4C4F4E47)
    parts = []
    for J in L_JOBS:
        parts.append([np.cumsum(rng.integers(0, 3, J)), rng.integers(0, 31, J), rng.integers(0, 9, J),
                      rng.integers(0, 6001, J)])
    for b in (0, HOLD_BATCH):
        p = [x.copy() for x in parts[LONG]]
        i = b * BATCH + 17
        p[1][i], p[2][i], p[3][i] = 1 << 30, 1, 1
        parts.append(p)
    arrays = seeded_workload("small", len(parts), 1)[0]
    off = np.concatenate([[0], np.cumsum([len(p[0]) for p in parts])]).astype(np.uint64)
    assert [int(o) % BATCH != 0 for o in off[[LONG, 4, HOLD_0, HOLD_300]]] == [True] * 4
    return arrays, JobStreams(*(np.concatenate([p[f] for p in parts]).astype(np.uint32) for f in range(4)), off)


def summaries(streams, node, fin, c):
    """{arrival_min, end_max} per 256 jobs of cluster c, as series_summary_kernel defines them (an
    unplaced job never ends)."""
    js = streams.of(c)
    arr = streams.arrival[js].astype(np.int64)
    end = np.where(node[js] >= 0, fin[js].astype(np.int64), 0xFFFFFFFF)
    cuts = np.arange(0, len(arr), BATCH)
    return np.minimum.reduceat(arr, cuts), np.maximum.reduceat(end, cuts)


def cursor_walk(amin, emax, t0, period, n, ts):
    """What the cursor of one cluster has to do, tile by tile, stated from the summaries alone: the
    rounds of 256 summaries from the first batch that may still be alive up to the round with the
    first batch that arrives after the tile.  Per tile: b_lo on entry and on exit, and per round its
    base, the length of the run of ended batches at its head, its hit batches and whether it holds a
    batch past the tile."""
    nb, b_lo, tiles = len(amin), 0, []
    for k0 in range(0, n, ts):
        tsa = min(ts, n - k0)
        t_first = t0 + k0 * period
        t_last = t_first + (tsa - 1) * period
        dead, past = emax <= t_first, amin > t_last
        alive = np.nonzero(~dead)[0]
        b_next = int(alive[0]) if alive.size else nb  # every batch below has ended before the tile
        rounds = []
        for base in range(b_lo, nb, ROUND):
            sl = slice(base, min(base + ROUND, nb))
            live = np.nonzero(~dead[sl])[0]
            rounds.append(dict(base=base, lead=int(live[0]) if live.size else sl.stop - sl.start,
                               hits=base + np.nonzero(~dead[sl] & ~past[sl])[0], past=bool(past[sl].any())))
            if rounds[-1]["past"]:
                break
        tiles.append(dict(b_in=b_lo, b_out=max(b_lo, b_next), rounds=rounds, t_first=t_first, t_last=t_last))
        b_lo = max(b_lo, b_next)
    return tiles


def window_jobs(arrays, streams, node, start, fin, t0, t_last):
    """The jobs that can touch a sample in [t0, t_last] (the others change no sample), as streams of
    their own with their placements: the brute-force reference then reads far fewer jobs."""
    keep = (streams.arrival.astype(np.int64) <= t_last) & ((node < 0) | (fin.astype(np.int64) > t0))
    off = np.concatenate([[0], np.cumsum([int(keep[streams.of(c)].sum()) for c in range(arrays.n_clusters)])])
    sub = JobStreams(*(getattr(streams, f)[keep] for f in ("arrival", "dur", "cores", "mem")), off.astype(np.uint64))
    return sub, node[keep], start[keep], fin[keep]


def assert_window(run, t0, period, n):
    eng, arrays, streams, node, start, fin = run
    samples, first = eng.cluster_state_series(t0, period, n)
    sub, sn, ss, sf = window_jobs(arrays, streams, node, start, fin, t0, t0 + (n - 1) * period)
    assert_samples_equal(samples, series_ref(arrays, sub, sn, ss, sf, t0, period, n), f"t0 {t0} period {period}")
    assert first.tobytes() == eng.cluster_states(t0).tobytes()
    return samples


@pytest.fixture(scope="module")
def run_l():
    arrays, streams = workload_l()
    node, start, fin = oracle_run("FIFO", arrays, streams)
    assert (node >= 0).all()  # the held jobs are small enough: every stream drains
    with Engine(0, policy="FIFO") as eng:
        eng.load_clusters(arrays)
        eng.submit_jobs(streams)
        eng.run()
        gn, gs, gf = eng.placements()
        np.testing.assert_array_equal(gn, node)
        np.testing.assert_array_equal(gs, start)
        np.testing.assert_array_equal(gf, fin)
        yield eng, arrays, streams, node, start, fin


def walks(run, t0, period, n):
    eng, arrays, streams, node, start, fin = run
    assert tile(5) == 127 and (np.diff(arrays.node_off) == 5).all()
    return {c: cursor_walk(*summaries(streams, node, fin, c), t0, period, n, 127) for c in (LONG, HOLD_0, HOLD_300)}


def assert_held_clusters(w, k):
    """Tile k lies late in the streams.  HOLD_0: batch 0 never ends, so the cursor stays at 0, every
    round up to the tile's own is read, and batch 0 is the only hit below the tile's batches.
    HOLD_300: the run of ended batches stops at batch 300, 44 batches into the second round."""
    t0, t300, tl = w[HOLD_0][k], w[HOLD_300][k], w[LONG][k]
    assert tl["b_out"] > 2 * ROUND  # late: LONG's own cursor is past two rounds
    assert t0["b_in"] == 0 and t0["b_out"] == 0
    assert [r["base"] for r in t0["rounds"]] == list(range(0, ROUND * len(t0["rounds"]), ROUND))
    assert len(t0["rounds"]) >= 3
    hits = np.concatenate([r["hits"] for r in t0["rounds"]])
    assert hits[0] == 0 and hits.size > 1 and hits[1] > 2 * ROUND
    assert t300["b_out"] == HOLD_BATCH and t300["b_in"] in (0, HOLD_BATCH)
    hits = np.concatenate([r["hits"] for r in t300["rounds"]])
    assert hits[0] == HOLD_BATCH and hits.size > 1 and hits[1] > 2 * ROUND
    if t300["b_in"] == 0:  # the run ends in the middle of the second round
        assert [r["lead"] for r in t300["rounds"][:2]] == [ROUND, HOLD_BATCH - ROUND]


def run_length(run):
    streams, fin = run[2], run[5]
    return int(fin[: int(streams.job_off[HOLD_0])].max())  # without the two jobs of 2^30 seconds


def test_long_stream_cursor_carries_over_full_rounds(run_l):
    period = run_length(run_l) // 140 + 1
    n = 150
    w = walks(run_l, 0, period, n)
    second = w[LONG][1]
    assert second["b_in"] == 0  # nothing has ended at t = 0, so the whole dead run is found in this tile
    assert [r["lead"] for r in second["rounds"][:2]] == [ROUND, ROUND] and second["b_out"] >= 2 * ROUND
    assert_held_clusters(w, 1)
    samples = assert_window(run_l, 0, period, n)
    assert samples["running"][[LONG, HOLD_0, HOLD_300]].max(axis=1).min() > 1
    assert samples["running"][:, -1].tolist() == [0, 0, 0, 0, 0, 1, 1]  # the two held jobs


def test_long_stream_cursor_stops_inside_the_second_round(run_l):
    streams = run_l[2]
    t0 = int(streams.arrival[streams.of(LONG)][70000])
    w = walks(run_l, t0, 1, 300)
    head = w[LONG][0]
    assert head["b_in"] == 0 and len(head["rounds"]) == 2
    assert head["rounds"][0]["lead"] == ROUND and not head["rounds"][0]["past"]
    assert 0 < head["rounds"][1]["lead"] < ROUND and head["rounds"][1]["past"]
    assert ROUND < head["b_out"] < 2 * ROUND
    assert w[HOLD_0][0]["b_out"] == 0 and len(w[HOLD_0][0]["rounds"]) == 2
    assert w[HOLD_300][0]["b_out"] == head["b_out"]  # batch 300 has not arrived yet
    assert_window(run_l, t0, 1, 300)


def test_long_stream_cursor_breaks_in_the_first_round(run_l):
    w = walks(run_l, 0, 1, 40)
    for c in (LONG, HOLD_0, HOLD_300):
        (only,) = w[c]
        assert len(only["rounds"]) == 1 and only["rounds"][0]["past"] and only["b_out"] == 0
    streams = run_l[2]
    assert (int(streams.job_off[LONG + 1] - streams.job_off[LONG]) + BATCH - 1) // BATCH - ROUND > ROUND
    assert_window(run_l, 0, 1, 40)


def test_long_stream_round_with_more_hits_than_a_group(run_l):
    streams = run_l[2]
    t0 = int(streams.arrival[streams.of(LONG)][150000])
    period, n = 20, 2 * 127 + 30
    w = walks(run_l, t0, period, n)
    for c in (LONG, HOLD_0, HOLD_300):
        assert max(len(r["hits"]) for t in w[c] for r in t["rounds"]) > GROUP
    assert_held_clusters(w, 0)
    assert_held_clusters(w, 1)
    assert_window(run_l, t0, period, n)


def test_long_stream_in_chunks_is_the_same_series(run_l, monkeypatch):
    eng = run_l[0]
    period = run_length(run_l) // 140 + 1
    whole, first = eng.cluster_state_series(0, period, 150)
    monkeypatch.setenv("MCS_SERIES_CHUNK", "41")
    parts, first2 = eng.cluster_state_series(0, period, 150)
    assert parts.tobytes() == whole.tobytes() and first2.tobytes() == first.tobytes()


def test_series_of_the_first_clusters_only(run_l):
    """n_clusters below the engine's count: those rows, and nothing written behind them."""
    eng, arrays = run_l[0], run_l[1]
    assert arrays.n_clusters == 7
    period, n = run_length(run_l) // 140 + 1, 150
    whole, first = eng.cluster_state_series(0, period, n)
    out = np.zeros((7, n), CLUSTER_SAMPLE_DTYPE)
    out.view(np.uint8)[...] = 0xA5
    one = np.zeros(7, first.dtype)
    one.view(np.uint8)[...] = 0xA5
    rc = L.lib().mcs_cluster_state_series(eng._h, 0, period, n, out.ctypes.data_as(C.POINTER(L.mcs_cluster_sample)),
                                          one.ctypes.data_as(C.POINTER(L.mcs_cluster_state)), 3, None)
    assert rc == L.MCS_OK
    assert out[:3].tobytes() == whole[:3].tobytes() and one[:3].tobytes() == first[:3].tobytes()
    assert (out[3:].view(np.uint8) == 0xA5).all() and (one[3:].view(np.uint8) == 0xA5).all()


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
