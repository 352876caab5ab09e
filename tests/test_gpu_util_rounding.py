"""GPU parity of GetResourceUtilization where its float32 arithmetic rounds (csrc/mcs_state.hip
state_kernel and series_kernel, csrc/mcs_kernels.hip utilization_kernel).

Workload R has node memories of 2^24 .. 2^30 (some of them 2^24 + odd, which float32 cannot hold),
requests that move the low bits of the per-node terms, and node counts on both sides of every
wave, workgroup and tile boundary up to the ABI's 1024.  Each conversion, each subtraction and each
addition of the Go loop (cluster.go:46-63) then rounds, so a sum in another order, in a tree, in
float64 or in integers gives other bits; the tests assert on the CPU that this is so for their own
inputs (util_ref.wrong_utilizations) before the GPU runs.  Three clusters are degenerate: a uint32
memory total that wraps to 5 (SetTotalResources sums in uint32), one that wraps to 0 (utilization
+Inf in use, NaN idle) and a cluster without nodes (NaN).  Two NaNs compare equal whatever their
sign and payload; everything else compares bit for bit (util_ref.same).
"""
import numpy as np
import pytest

import oracle_ref as O
import util_ref as U
from mcs_amd import CLUSTER_SAMPLE_DTYPE, ClusterArrays, Engine, JobStreams
from mcs_amd import _lib as L
from test_gpu_state import expected_states
from test_gpu_state_series import oracle_run, series_ref, tile

pytestmark = pytest.mark.gpu

NODE_COUNTS = (1, 3, 64, 65, 200, 256, 257, 600, 1024)
C_WRAP_SMALL, C_WRAP_ZERO, C_EMPTY = len(NODE_COUNTS), len(NODE_COUNTS) + 1, len(NODE_COUNTS) + 2
C_256 = NODE_COUNTS.index(256)
WRAPPED_SMALL = 5
JOBS = 600
SEED = 2  # chosen so that the reference meets the conditions asserted in run_r and in the sentinel test


def workload_r(seed=SEED):
    """(arrays, streams).  Node 0 of every cluster is fully available, and every request fits some
    node's initial availability, so every job of a cluster with nodes is placed in the end.  Cores
    go up to 4000 a node, and up to 60000 in the 600- and 1024-node clusters: there the cores sums
    pass 2^24 as well."""
    rng = np.random.default_rng(seed)
    cols, parts, off = [], [], [0]
    for nn in NODE_COUNTS + ("wrap_small", "wrap_zero", 0):
        if nn == "wrap_small":  # 4 * 2^30 + 5 = 5 mod 2^32
            cap_m = np.array([1 << 30, 1 << 30, 1 << 30, (1 << 30) - (1 << 24), (1 << 24) + WRAPPED_SMALL], np.int64)
        elif nn == "wrap_zero":
            cap_m = np.full(4, 1 << 30, np.int64)
        else:
            cap_m = rng.integers(1 << 24, (1 << 30) + 1, nn)
            odd = rng.random(nn) < 0.3  # 2^24 + odd: not a float32
            cap_m[odd] = (1 << 24) + 2 * rng.integers(0, 1 << 10, int(odd.sum())) + 1
        n = len(cap_m)
        cap_c = rng.integers(1, 60001 if n >= 600 else 4001, n)
        free_c = np.where(rng.random(n) < 0.5, cap_c, rng.integers(0, cap_c + 1))
        free_m = np.where(rng.random(n) < 0.5, cap_m, rng.integers(0, cap_m + 1))
        if n:
            free_c[0], free_m[0] = cap_c[0], cap_m[0]
        if nn == "wrap_zero":  # idle before the first arrival and after the last finish: 0 / 0
            free_c, free_m = cap_c.copy(), cap_m.copy()
        cols.append((cap_c, cap_m, free_c, free_m))
        off.append(off[-1] + n)
        # arrivals a little over a second apart (DELAY decides one Level0 job a second)
        arr = np.cumsum(1 + rng.poisson(0.4, JOBS))
        dur = rng.integers(0, 300, JOBS)
        if n:  # up to the initial availability of a random node; some memory requests at 2^24 +- 1
            k = rng.integers(0, n, JOBS)
            cores, mem = rng.integers(0, free_c[k] + 1), rng.integers(0, free_m[k] + 1)
            near = (rng.random(JOBS) < 0.1) & (free_m[k] > (1 << 24))
            mem[near] = (1 << 24) + rng.integers(-1, 2, int(near.sum()))
        else:
            cores, mem = np.ones(JOBS, np.int64), np.ones(JOBS, np.int64)
        parts.append((arr, dur, cores, mem))
    arrays = ClusterArrays(*(np.concatenate([c[f] for c in cols]).astype(np.uint32) for f in range(4)),
                           np.array(off, np.uint32))
    streams = JobStreams(*(np.concatenate([p[f] for p in parts]).astype(np.uint32) for f in range(4)),
                         np.arange(len(parts) + 1, dtype=np.uint64) * JOBS)
    return arrays, streams


def free_at(arrays, streams, node, start, fin, c, t):
    """(cap_c, cap_m, free_c, free_m) of cluster c after second t, from the placements."""
    ns, js = arrays.nodes_of(c), streams.of(c)
    n = ns.stop - ns.start
    run = (node[js] >= 0) & (start[js] <= t) & (fin[js] > t)
    k = node[js][run]
    uc = np.bincount(k, weights=streams.cores[js][run].astype(np.float64), minlength=n).astype(np.uint64)
    um = np.bincount(k, weights=streams.mem[js][run].astype(np.float64), minlength=n).astype(np.uint64)
    return (arrays.cap_c[ns].astype(np.uint64), arrays.cap_m[ns].astype(np.uint64),
            arrays.free_c[ns].astype(np.uint64) - uc, arrays.free_m[ns].astype(np.uint64) - um)


def discriminating(arrays, streams, node, start, fin, t, clusters):
    """Per wrong method, the clusters whose serial utilization at t differs from it (either column)."""
    out = {}
    for c in clusters:
        cap_c, cap_m, free_c, free_m = free_at(arrays, streams, node, start, fin, c, t)
        dc, dm = U.discriminates(cap_c, free_c), U.discriminates(cap_m, free_m)
        for name in dm:
            out.setdefault(name, []).append(dc[name] or dm[name])
    return {k: int(np.sum(v)) for k, v in out.items()}


def assert_samples_same(got, want, tag=""):
    for f in CLUSTER_SAMPLE_DTYPE.names:
        ok = U.same(got[f], want[f]) if got[f].dtype.kind == "f" else got[f] == want[f]
        bad = np.argwhere(~ok)
        assert bad.size == 0, f"{tag} {f}: {len(bad)} samples differ, first (cluster, k) {bad[:4].tolist()}: " \
                              f"got {got[f][tuple(bad[0])]!r} want {want[f][tuple(bad[0])]!r}"


@pytest.fixture(scope="module")
def workload():
    return workload_r()


@pytest.fixture(scope="module", params=["FIFO", "DELAY"])
def run_r(request, workload):
    """Workload R run once per policy: the conditions on the reference's placements are asserted
    before the engine is opened, the placements' equality before anything is sampled."""
    policy = request.param
    arrays, streams = workload
    node, start, fin = oracle_run(policy, arrays, streams)
    with_nodes = [c for c in range(arrays.n_clusters) if c != C_EMPTY]
    for c in with_nodes:
        assert (node[streams.of(c)] >= 0).all(), c
    assert (node[streams.of(C_EMPTY)] < 0).all()
    t_mid = int(np.median(start[node >= 0]))
    regular = [c for c in range(arrays.n_clusters) if c not in (C_WRAP_ZERO, C_EMPTY)]
    found = discriminating(arrays, streams, node, start, fin, t_mid, regular)
    assert len(found) == 4 and min(found.values()) * 2 >= len(regular), found
    with Engine(0, policy=policy) as eng:
        eng.load_clusters(arrays)
        eng.submit_jobs(streams)
        eng.run()
        gn, gs, gf = eng.placements()
        np.testing.assert_array_equal(gn, node)
        np.testing.assert_array_equal(gs, start)
        np.testing.assert_array_equal(gf, fin)
        yield eng, arrays, streams, node, start, fin, t_mid


def sample_times(node, start, fin, t_mid):
    placed = node >= 0
    return 0, t_mid, int(start[placed].max()), int(fin[placed].max()) + 5


def test_cluster_states_where_sums_round(run_r):
    eng, arrays, streams, node, start, fin, t_mid = run_r
    seen = set()
    for t in sample_times(node, start, fin, t_mid):
        got = eng.cluster_states(t)
        want = expected_states(arrays, streams, node, start, fin, t)
        for c, (cu, mu, tc, tm, nrun) in enumerate(want):
            g = got[c]
            assert (g["total_cpu"], g["total_memory"], g["running"], g["t_s"]) == (tc, tm, nrun, t), (c, t)
            assert U.same(g["cores_utilization"], cu), (c, t, g["cores_utilization"], cu)
            assert U.same(g["memory_utilization"], mu), (c, t, g["memory_utilization"], mu)
        assert got[C_WRAP_SMALL]["total_memory"] == WRAPPED_SMALL and got[C_WRAP_ZERO]["total_memory"] == 0
        assert np.isnan(got[C_EMPTY]["memory_utilization"]) and np.isnan(got[C_EMPTY]["cores_utilization"])
        mz = got[C_WRAP_ZERO]["memory_utilization"]
        assert np.isnan(mz) or mz == np.inf
        seen.add("nan" if np.isnan(mz) else "inf")
    assert seen == {"nan", "inf"}  # the wrapped divisor met both an idle cluster and one in use


def assert_series_same_as_single_call(eng, samples, t0, period, ks):
    for k in ks:
        one = eng.cluster_states(t0 + k * period)
        for f in ("cores_utilization", "memory_utilization", "running"):
            ok = U.same(samples[f][:, k], one[f]) if one[f].dtype.kind == "f" else samples[f][:, k] == one[f]
            assert ok.all(), f"{f} at k={k} (t={t0 + k * period}), clusters {np.nonzero(~ok)[0][:4].tolist()}"


def tile_edges(arrays, n):
    ks = {0, n - 1}
    for ts in {tile(int(x)) for x in np.diff(arrays.node_off)}:  # each tile's first and last sample
        ks |= set(range(0, n, ts)) | set(range(ts - 1, n, ts))
    return sorted(ks)


def test_series_every_second_where_sums_round(run_r):
    eng, arrays, streams, node, start, fin, t_mid = run_r
    sizes = {tile(int(x)) for x in np.diff(arrays.node_off)}
    assert 9 in sizes and 127 in sizes  # the 1024-node cluster's tile, and the largest
    n = 3 * min(sizes) + 7
    samples, first = eng.cluster_state_series(t_mid, 1, n)
    assert_samples_same(samples, series_ref(arrays, streams, node, start, fin, t_mid, 1, n))
    assert_series_same_as_single_call(eng, samples, t_mid, 1, tile_edges(arrays, n))
    one = eng.cluster_states(t_mid)
    for f in one.dtype.names:
        assert (U.same(first[f], one[f]) if one[f].dtype.kind == "f" else first[f] == one[f]).all(), f


def test_series_over_the_run_where_sums_round(run_r):
    eng, arrays, streams, node, start, fin, t_mid = run_r
    n = 150
    period = (int(fin[node >= 0].max()) + 5) // (n - 3) + 1
    assert (n - 1) * period > int(fin[node >= 0].max())
    samples, first = eng.cluster_state_series(0, period, n)
    assert_samples_same(samples, series_ref(arrays, streams, node, start, fin, 0, period, n))
    assert_series_same_as_single_call(eng, samples, 0, period, tile_edges(arrays, n))
    one = eng.cluster_states(0)
    for f in one.dtype.names:
        assert (U.same(first[f], one[f]) if one[f].dtype.kind == "f" else first[f] == one[f]).all(), f
    assert (samples["running"][:, -1] == 0).all()
    assert np.isinf(samples["memory_utilization"][C_WRAP_ZERO]).any()
    assert np.isnan(samples["memory_utilization"][C_WRAP_ZERO][-1])
    assert np.isnan(samples["memory_utilization"][C_EMPTY]).all()


def test_expected_bits_differ_from_every_wrong_sum(run_r):
    """The sentinel: what the tests above expect of the 256-node cluster at the sampled second is
    none of the four wrong sums, so a kernel that computes one of them fails them."""
    eng, arrays, streams, node, start, fin, t_mid = run_r
    cap_c, cap_m, free_c, free_m = free_at(arrays, streams, node, start, fin, C_256, t_mid)
    want = expected_states(arrays, streams, node, start, fin, t_mid)[C_256][1]
    assert U.same(want, U.utilization(cap_m, free_m))
    wrong = U.wrong_utilizations(cap_m, free_m)
    assert len(wrong) == 4
    for name, v in wrong.items():
        assert not U.same(want, v), name


def mirror_plan(arrays):
    """Per cluster, five requests that each fit a node (first fit places them there or earlier),
    the node the oracle's ScheduleJob gives each, and the counters after they are committed."""
    rng = np.random.default_rng(SEED + 1)
    plan = []
    for c in range(arrays.n_clusters):
        ns = arrays.nodes_of(c)
        fc, fm = arrays.free_c[ns].astype(np.uint64), arrays.free_m[ns].astype(np.uint64)
        held = []
        for _ in range(5 if len(fc) else 0):
            k = int(rng.integers(0, len(fc)))
            cores, mem = int(rng.integers(0, fc[k] + 1)), int(rng.integers(0, fm[k] + 1))
            want = O.schedule_job(fc, fm, cores, mem)
            assert 0 <= want <= k
            fc[want] -= cores
            fm[want] -= mem
            held.append((want, cores, mem))
        plan.append((held, fc, fm))
    return plan


def test_live_mirror_utilization_where_sums_round(engine, workload):
    """mcs_resource_utilization over the live counters: after load, after a few commits of
    mcs_schedule_one, and after mcs_release_one has given them back."""
    arrays, streams = workload
    plan = mirror_plan(arrays)
    found = {}
    for c, (held, fc, fm) in enumerate(plan):
        ns = arrays.nodes_of(c)
        for free in (arrays.free_m[ns], fm):
            for name, d in U.discriminates(arrays.cap_m[ns], free).items():
                found.setdefault(name, set()).update({c} if d else ())
    # each wrong sum shows in some state of at least half of the 7 clusters of 64 nodes and more
    assert len(found) == 4 and min(len(v) for v in found.values()) >= 4, found

    engine.load_clusters(arrays)

    def check(c, fc, fm, tag):
        ns = arrays.nodes_of(c)
        lc, lm = engine.live_state(c)
        np.testing.assert_array_equal(lc, fc.astype(np.uint32))
        np.testing.assert_array_equal(lm, fm.astype(np.uint32))
        gc, gm = (np.float32(x) for x in engine.resource_utilization(c))
        oc, om = (np.float32(x) for x in O.resource_utilization(arrays.cap_c[ns], arrays.cap_m[ns], fc, fm))
        wc, wm = U.resource_utilization(arrays.cap_c[ns], arrays.cap_m[ns], fc, fm)
        assert U.same(oc, wc) and U.same(om, wm), (c, tag)
        assert U.same(gc, wc) and U.same(gm, wm), (c, tag, gc, wc, gm, wm)

    for c, (held, fc, fm) in enumerate(plan):
        ns = arrays.nodes_of(c)
        check(c, arrays.free_c[ns], arrays.free_m[ns], "loaded")
        if c == C_EMPTY:
            assert engine.schedule_one(c, 0, 0) == L.MCS_NODE_UNPLACED
            continue
        for want, cores, mem in held:
            assert engine.schedule_one(c, cores, mem) == want
        check(c, fc, fm, "committed")
        for k, cores, mem in held:
            engine.release_one(c, k, cores, mem)
        check(c, arrays.free_c[ns], arrays.free_m[ns], "released")
