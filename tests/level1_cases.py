"""Workloads and expectations shared by the CPU and the GPU tests of the Level1 series — TEST
INFRASTRUCTURE ONLY.  The CPU tests (tests/test_level1_ref.py) check, without a GPU, that the seeds
the GPU tests (tests/test_gpu_level1_series.py) use meet their coverage conditions."""
from __future__ import annotations

import numpy as np

import level1_ref as R
from kat_util import fuzz_workload
from mcs_amd import Cluster, ClusterArrays, JobStreams, Node, pack_clusters, replicate, uniform_cluster

T_MAX = 0xFFFFFFFE
HOT_SEED = 0x4C314854


def hot_clusters(sizes, seed, nodes=None, gaps=(0, 0, 1, 1, 1, 2)):
    """Small hot clusters: 2-6 nodes (or `nodes`) of 8 cores / 32 memory, gaps drawn from `gaps`,
    durations 0-40, requests up to a node (every job fits an empty node: no deadlock)."""
    rng = np.random.default_rng(seed)
    clusters, parts = [], []
    for k, J in enumerate(sizes):
        nn = int(rng.integers(2, 7)) if nodes is None else nodes[k]
        clusters.append(Cluster(Id=k + 1, Nodes=[Node(Id=i + 1, Cores=8, Memory=32, CoresAvailable=8,
                                                      MemoryAvailable=32) for i in range(nn)]))
        parts.append((np.cumsum(rng.choice(gaps, J)), rng.integers(0, 41, J), rng.integers(0, 9, J),
                      rng.integers(0, 33, J)))
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    return pack_clusters(clusters), JobStreams(*(np.concatenate([p[f] for p in parts]).astype(np.uint32)
                                                 for f in range(4)), off)


def hot_five_nodes():
    """The hot 5-node clusters of the every-second tests."""
    return hot_clusters([300] * 8, HOT_SEED, nodes=[5] * 8)


def rounds_system():
    """Streams of 255, 256, 257 and 513 jobs on 2-3 nodes: Level1 windows across the 256-job batches."""
    return hot_clusters([255, 256, 257, 513], 0x4C315244, nodes=[2, 3, 2, 3])


def concat(parts):
    """Single-cluster (arrays, streams) pairs as one system."""
    assert all(a.n_clusters == 1 for a, _ in parts)
    arrays = ClusterArrays(*(np.concatenate([getattr(a, f) for a, _ in parts]) for f in
                             ("cap_c", "cap_m", "free_c", "free_m")),
                           np.concatenate([[0], np.cumsum([int(a.node_off[-1]) for a, _ in parts])]).astype(np.uint32))
    off = np.concatenate([[0], np.cumsum([s.n_jobs for _, s in parts])]).astype(np.uint64)
    return arrays, JobStreams(*(np.concatenate([getattr(s, f) for _, s in parts]) for f in
                                ("arrival", "dur", "cores", "mem")), off)


DEAD, EMPTY, CALM = 0, 1, 2


def deadlock_system():
    """Cluster DEAD: one node of 4 cores / 2^31 - 1 memory and 40 jobs, every third one asking 5 cores
    (it fits no node, moves to Level1 and stays) and 2^30 memory: the 14 leftovers' memories sum to
    14 * 2^30 = 3.5 * 2^32, which wraps.  Cluster EMPTY has no jobs.  Cluster CALM places every job at
    its arrival: nothing ever moves to Level1."""
    J = 40
    big = np.arange(J) % 3 == 0
    dead = (pack_clusters([Cluster(Id=1, Nodes=[Node(Id=1, Cores=4, Memory=0x7FFFFFFF, CoresAvailable=4,
                                                     MemoryAvailable=0x7FFFFFFF)])]),
            JobStreams(np.arange(J, dtype=np.uint32) * 2, np.where(big, 7 + np.arange(J) % 5, 1).astype(np.uint32),
                       np.where(big, 5, 1).astype(np.uint32), np.where(big, 1 << 30, 3).astype(np.uint32),
                       np.array([0, J], np.uint64)))
    nothing = JobStreams(*(np.zeros(0, np.uint32) for _ in range(4)), np.zeros(2, np.uint64))
    calm = JobStreams(np.arange(30, dtype=np.uint32) * 50, np.full(30, 5, np.uint32), np.full(30, 1, np.uint32),
                      np.full(30, 1, np.uint32), np.array([0, 30], np.uint64))
    return concat([dead, (replicate(uniform_cluster(7), 1), nothing), (replicate(uniform_cluster(7), 1), calm)])


def level1_pressure(n_clusters=2, J=1500, blocked=660):
    """256 nodes of 2 cores / 4000 memory, every fourth one available, more than two arrivals per
    second: small jobs wait MaxWaitTime and are placed from Level1, and `blocked` requests of 3 cores
    fit no node, so Level1 outgrows the 640 entries the hand-scheduled loop keeps in LDS and the
    cluster is handed to delay_kernel (the shape of tests/test_gpu_wait_series.py, restated)."""
    rng = np.random.default_rng(0x4C31)
    cl = Cluster(Id=1, Nodes=[Node(Id=i + 1, Cores=2, Memory=4000, CoresAvailable=0 if i % 4 else 2,
                                   MemoryAvailable=0 if i % 4 else 4000) for i in range(256)])
    parts = []
    for _ in range(n_clusters):
        cores = rng.integers(0, 3, J)
        cores[rng.choice(J, blocked, replace=False)] = 3
        parts.append((np.cumsum(rng.poisson(0.4, J)), rng.integers(0, 400, J), cores, rng.integers(0, 4001, J)))
    off = np.arange(n_clusters + 1, dtype=np.uint64) * J
    return replicate(cl, n_clusters), JobStreams(*(np.concatenate([p[f] for p in parts]).astype(np.uint32)
                                                   for f in range(4)), off)


class Ref:
    """The replay of every cluster of a DELAY run with known starts (an unplaced job's start is
    MCS_TIME_NONE), and the samples a series call must return."""

    def __init__(self, streams, start, W):
        self.streams, self.start, self.W = streams, np.asarray(start), int(W)
        self.C = len(streams.job_off) - 1
        self._rep = {}

    def of(self, c):
        js = self.streams.of(c)
        return self.streams.arrival[js], self.start[js]

    def replay(self, c, T):
        if (c, T) not in self._rep:
            self._rep[c, T] = R.replay(*self.of(c), self.W, T)
        return self._rep[c, T]

    def members(self, c, t, T):
        return self.replay(c, T)["lists"][t]

    def want(self, t0, period, n, T=None):
        """The samples from the replay up to second T (default: the last sample); later seconds read
        the loop's fixed point, which the replay must have reached by T."""
        last = t0 + (n - 1) * period
        T = last if T is None else T
        out = np.zeros((self.C, n), R.LEVEL1)
        for c in range(self.C):
            js = self.streams.of(c)
            rep = self.replay(c, T)
            if last > T:
                assert R.steady_after(rep, *self.of(c))
            out[c] = R.series(rep, self.streams.dur[js], self.streams.cores[js], self.streams.mem[js], t0, period, n,
                              steady=last > T)
        return out


def assert_coverage(want):
    """The sampled seconds hold the lengths and the small-node times at which the kernels take
    another path (asserted on the reference before anything is compared with it)."""
    lens = set(np.unique(want["len"]).tolist())
    assert {0, 1, 19, 20, 21} <= lens and max(lens) >= 40, sorted(lens)[:30]
    mult = (want["len"] > 0) & (want["len"] % 20 == 0)
    assert (mult & (want["small_time_s"] != 0)).any(), "no positive multiple of 20 with a small-node time"
    assert (mult & (want["small_time_s"] == 0)).any(), "no positive multiple of 20 with an odd trailing run"
    assert (want["small_time_s"][~mult] == 0).all()


def assert_samples_equal(got, want, tag=""):
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype)
    for f in want.dtype.names:
        bad = np.argwhere(got[f] != want[f])
        assert bad.size == 0, f"{tag} {f}: {len(bad)} samples differ, first (cluster, k) {bad[:4].tolist()}: " \
                              f"got {got[f][tuple(bad[0])]!r} want {want[f][tuple(bad[0])]!r}"
