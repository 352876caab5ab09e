"""The streamed W16R loop's fit test and commit ("Fit and commit"): the fit test sign-replicates
the guard bits of two chunks with one v_perm (their cores guards into the low half, their memory guards into the
high half) and ANDs the halves, and the commit writes the fitting lane's chunk with a v_cndmask under a scalar
lane mask, `exec` staying the full wave from the fit test to the record read.  What can go wrong there is a
pairing (chunk i's cores guard ANDed with chunk j's memory guard), a lane mask that misses its lane (lanes 31 and
32 are the two dwords' edges), a chunk register other than the picked one, and a path that relied on the `exec`
the commit used to restore.  Every case is a bit-exact parity run against the oracle (node, start, finish, t_end,
placed, waited, peak_running, flags) on the production and the counting build, with the kernel asserted; what a
case relies on is asserted from the oracle's results on the CPU first.  The cases pin behaviour that does not
change: they pass on the loop with four SDWA ANDs and a one-lane `exec` as well.  Run on a real MI355X:
``pytest -m gpu``.

Node 4 * lane + chunk is chunk `chunk` of lane `lane`; the first fit is the lowest lane with a fitting chunk, and
its lowest fitting chunk."""
import numpy as np
import pytest

from mcs_amd import MCS_FLAG_DEADLOCK, pack_clusters, uniform_cluster
from mcs_amd.cluster import Cluster, Node
from test_gpu_calendar_rows import diag, run_and_compare, streams_of  # noqa: F401
from test_gpu_deferred_insert import finishes_of, nodes_of
from test_gpu_wait_section import crowded, oracle_of, starts_of

pytestmark = pytest.mark.gpu

EDGE_LANES = (0, 31, 32, 63)  # the first and the last bit of either dword of a lane mask
CORES, MEM = 32, 24000
REQ = (8, 1000)


def cluster_of(n, free):
    """n nodes of 32 cores and 24000 MB with nothing available but `free`: {node: (cores, memory)}.  A node with
    nothing available fits no request that asks for anything."""
    return Cluster(Id=1, Nodes=[Node(Id=i + 1, Cores=CORES, Memory=MEM, CoresAvailable=free.get(i, (0, 0))[0],
                                     MemoryAvailable=free.get(i, (0, 0))[1]) for i in range(n)])


def size_for(lane, k):
    """256 nodes, or 129 (lanes 0 ... 31 whole, chunk 0 of lane 32, the rest padding) in turn where the lane has
    all its nodes in it."""
    return 129 if lane < 32 and k % 2 else 256


# ---- the pairing -----------------------------------------------------------------------------------------------
def case_pairing(lane, i):
    """One cluster per j != i.  Chunk i of the lane has the cores and not the memory, chunk j the memory and not
    the cores, chunk k (the higher of the other two) exactly the request, and nothing else is available.  Two
    jobs ask for the same at second 0: the first takes chunk k, the second fits nowhere (not c_i with m_j) and
    waits for it; a third comes later."""
    per, want, clusters = [], [], []
    for n, j in enumerate(c for c in range(4) if c != i):
        k = max(c for c in range(4) if c not in (i, j))
        free = {4 * lane + i: (CORES, REQ[1] - 1), 4 * lane + j: (REQ[0] - 1, MEM), 4 * lane + k: REQ}
        clusters.append(cluster_of(size_for(lane, n) if lane < 32 else 256, free))
        per.append([(0, 50, *REQ), (0, 50, *REQ), (200, 5, *REQ)])
        want.append(4 * lane + k)
    arrays, s = pack_clusters(clusters), streams_of(per)
    oracle = oracle_of(arrays, s)
    assert not oracle[3]["flags"].any() and oracle[3]["waited"].tolist() == [1] * 3
    for c in range(3):
        assert nodes_of(oracle, s, c) == [want[c]] * 3 and starts_of(oracle, s, c) == [0, 50, 200]
    return arrays, s, oracle


@pytest.mark.parametrize("i", range(4))
@pytest.mark.parametrize("lane", EDGE_LANES)
def test_cores_of_one_chunk_and_memory_of_another_do_not_fit(engine, diag, lane, i):
    run_and_compare(engine, *case_pairing(lane, i), diag)


def case_pairing_nothing_fits(lane):
    """The same without chunk k, for the four (i, j) a cluster each: the job fits nowhere with nothing running."""
    pairs = [(0, 1), (1, 0), (2, 3), (3, 2)] if lane % 2 else [(0, 2), (2, 0), (1, 3), (3, 1)]
    clusters = [cluster_of(256, {4 * lane + i: (CORES, REQ[1] - 1), 4 * lane + j: (REQ[0] - 1, MEM)}) for i, j in pairs]
    per = [[(0, 0, 0, 1), (0, 50, *REQ), (1, 5, *REQ)] for _ in pairs]  # (a zero-duration job fits chunk j first)
    arrays, s = pack_clusters(clusters), streams_of(per)
    oracle = oracle_of(arrays, s)
    assert ((oracle[3]["flags"] & MCS_FLAG_DEADLOCK) != 0).all() and oracle[3]["placed"].tolist() == [1] * 4
    assert [nodes_of(oracle, s, c)[0] for c in range(4)] == [4 * lane + min(p) for p in pairs]
    return arrays, s, oracle


@pytest.mark.parametrize("lane", EDGE_LANES)
def test_pairing_with_no_fitting_chunk_deadlocks(engine, diag, lane):
    run_and_compare(engine, *case_pairing_nothing_fits(lane), diag)


# ---- each chunk alone, the lowest chunk, the lowest lane -------------------------------------------------------
def case_single_chunks(lane):
    """Clusters 0-3: chunk c of the lane alone holds the request.  4, 5: two chunks of the lane do (0 and 3, 1
    and 2): the lower one is taken first, then the other.  6: chunk 3 of the lane and chunk 0 of the next lane
    (the lane before for lane 63): the lower lane first.  7: this lane and the lane 32 away."""
    other = lane + 1 if lane < 63 else lane - 1
    frees = [[4 * lane + c] for c in range(4)] + [[4 * lane, 4 * lane + 3], [4 * lane + 1, 4 * lane + 2]]
    frees += [sorted([4 * lane + 3, 4 * other]), sorted([4 * lane + 2, 4 * (lane ^ 32) + 1])]
    clusters, per = [], []
    for n, f in enumerate(frees):
        small = max(f) < 129 and n % 2
        clusters.append(cluster_of(129 if small else 256, {x: REQ for x in f}))
        per.append([(0, 30, *REQ)] * len(f) + [(0, 9, *REQ), (100, 3, *REQ)])
    arrays, s = pack_clusters(clusters), streams_of(per)
    oracle = oracle_of(arrays, s)
    assert not oracle[3]["flags"].any() and oracle[3]["waited"].tolist() == [1] * len(frees)
    for c, f in enumerate(frees):
        assert nodes_of(oracle, s, c) == f + [f[0], f[0]], (c, f)
        assert starts_of(oracle, s, c) == [0] * len(f) + [30, 100]
    return arrays, s, oracle


@pytest.mark.parametrize("lane", EDGE_LANES)
def test_each_chunk_alone_lowest_chunk_lowest_lane(engine, diag, lane):
    run_and_compare(engine, *case_single_chunks(lane), diag)


# ---- boundaries ------------------------------------------------------------------------------------------------
def case_boundaries():
    """Node 130 (lane 32, chunk 2) holds (8, 1000).  Requests equal to it in cores, in memory and in both fit,
    one after the other; one above it in cores (cluster 0) or memory (cluster 1) fits nowhere, and requests of
    0x8000, 0xffff, 0x10000 and 0x18000 cores or MB (clusters 2-9: clamped to 0x7fff, and the last two with
    low halves that read 0 and 0x8000) fit no node of a cluster with everything free."""
    eq = [(0, 5, REQ[0], REQ[1] - 1), (10, 5, REQ[0] - 1, REQ[1]), (20, 5, *REQ)]
    per = [eq + [(30, 5, REQ[0] + 1, REQ[1])], eq + [(30, 5, REQ[0], REQ[1] + 1)]]
    clusters = [cluster_of(256, {130: REQ}), cluster_of(256, {130: REQ})]
    for big in (0x8000, 0xFFFF, 0x10000, 0x18000):
        per += [[(0, 5, 1, 1), (1, 5, big, 1)], [(0, 5, 1, 1), (1, 5, 1, big)]]
        clusters += [uniform_cluster(256), uniform_cluster(129)]
    arrays, s = pack_clusters(clusters), streams_of(per)
    oracle = oracle_of(arrays, s)
    assert ((oracle[3]["flags"] & MCS_FLAG_DEADLOCK) != 0).all()
    assert oracle[3]["placed"].tolist() == [3, 3] + [1] * 8
    for c in range(2):
        assert nodes_of(oracle, s, c)[:3] == [130] * 3 and starts_of(oracle, s, c)[:3] == [0, 10, 20]
    return arrays, s, oracle


def test_requests_at_and_above_what_is_free(engine, diag):
    run_and_compare(engine, *case_boundaries(), diag)


def case_padding_never_fits():
    """A 129-node cluster takes 129 whole-node jobs on nodes 0 ... 128; the next one fits no padding node (129 ...
    255: the chunks 1-3 of lane 32 and the lanes behind it) and waits for node 0.  Cluster 1: only node 128 is
    available."""
    whole = (CORES, MEM)
    per = [[(0, 40 + i % 5, *whole) for i in range(129)] + [(1, 7, *whole), (2, 7, 1, 1)],
           [(0, 40, *REQ), (0, 7, *REQ), (90, 7, *REQ)]]
    arrays = pack_clusters([uniform_cluster(129), cluster_of(129, {128: REQ})])
    s = streams_of(per)
    oracle = oracle_of(arrays, s)
    assert not oracle[3]["flags"].any() and oracle[3]["waited"].tolist() == [1, 1]
    assert nodes_of(oracle, s, 0)[:130] == list(range(129)) + [0] and starts_of(oracle, s, 0)[129] == 40
    assert nodes_of(oracle, s, 1) == [128] * 3 and starts_of(oracle, s, 1) == [0, 40, 90]
    return arrays, s, oracle


def test_padding_nodes_never_fit(engine, diag):
    run_and_compare(engine, *case_padding_never_fits(), diag)


# ---- the commit under the lane mask ----------------------------------------------------------------------------
HALF = 17  # cores: a node of 32 holds one such job


def neighbours(lane):
    return sorted({lane - 1, lane + 1, lane ^ 32, 0, 63} & set(range(64)) - {lane})


def case_commit(lane):
    """The lane's four nodes are whole; the nodes of the lanes beside it, of the lane 32 away and of lanes 0 and
    63 have 16 cores and all their memory.  Four jobs of 17 cores and four amounts of memory take chunks 0-3 of
    the lane in the pass; four more fail, and each is placed as a waiting head on the chunk that comes back
    (chunks 0-3 in turn, three seconds apart).  When all have finished, four whole-node requests arrive, which
    fit the lane's nodes only if each got back exactly what was taken, and then one request of (16 cores, all the
    memory) per neighbouring node, which fits it only if nothing was written there: a commit into another lane
    or chunk shows in where and when those run."""
    others = [4 * l + c for l in neighbours(lane) for c in range(4)]
    free = {4 * lane + c: (CORES, MEM) for c in range(4)}
    free.update({x: (16, MEM) for x in others})
    rows = [(0, 20 + 3 * c, HALF, 700 + 11 * c) for c in range(4)]
    rows += [(1, 40 + c, HALF, 900 + 13 * c) for c in range(4)]
    rows += [(300, 10, CORES, MEM)] * 4 + [(300, 10, 16, MEM)] * len(others) + [(400, 1, CORES, MEM)]
    arrays, s = pack_clusters([cluster_of(256, free)] * 2), streams_of([rows, rows])
    oracle = oracle_of(arrays, s)
    assert not oracle[3]["flags"].any() and oracle[3]["waited"].tolist() == [4, 4]
    nd, st = nodes_of(oracle, s, 0), starts_of(oracle, s, 0)
    mine = [4 * lane + c for c in range(4)]
    assert nd[:12] == mine * 3 and nd[12:-1] == others and nd[-1] == mine[0]
    assert st[:8] == [0] * 4 + [20, 23, 26, 29] and st[8:-1] == [300] * (4 + len(others))
    return arrays, s, oracle


@pytest.mark.parametrize("lane", EDGE_LANES)
def test_commit_writes_one_lane_and_chunk(engine, diag, lane):
    run_and_compare(engine, *case_commit(lane), diag)


def case_64_at_one_instant():
    """64 placements at one second, each in another fit lane (cluster 0: one available node per lane, chunk
    lane & 3) or four to a lane (cluster 1: a uniform cluster, whole-node jobs), then whole-node requests once
    they have finished."""
    free = [4 * l + (l & 3) for l in range(64)]
    per = [[(0, 30 + l % 7, CORES, MEM - l) for l in range(64)] + [(100, 5, CORES, MEM)] * 64,
           [(0, 30 + l % 7, CORES, 1 + l) for l in range(64)] + [(100, 5, CORES, MEM)] * 64]
    arrays = pack_clusters([cluster_of(256, {x: (CORES, MEM) for x in free}), uniform_cluster(256)])
    s = streams_of(per)
    oracle = oracle_of(arrays, s)
    assert not oracle[3]["flags"].any() and not oracle[3]["waited"].any()
    assert nodes_of(oracle, s, 0) == free * 2 and nodes_of(oracle, s, 1) == list(range(64)) * 2
    assert starts_of(oracle, s, 0) == [0] * 64 + [100] * 64
    return arrays, s, oracle


def test_64_placements_at_one_instant(engine, diag):
    run_and_compare(engine, *case_64_at_one_instant(), diag)


def case_release_behind_a_placement():
    """One node is available, chunk lane & 3 of an edge lane (a cluster each).  A (17 cores) runs one second on
    it, B (15 cores) is placed beside it at the same second, and the next job arrives a second on: the release
    that follows B's placement refreshes the node copy under the `exec` the commit left and hands A's request
    back.  C asks for exactly what the node then holds (17 cores, all the memory but B's), D for the whole node
    once B and C have finished."""
    clusters, per, marks = [], [], []
    for lane in EDGE_LANES:
        a = 4 * lane + (lane & 3)
        clusters.append(cluster_of(256, {a: (CORES, MEM)}))
        per.append([(0, 1, HALF, 777), (0, 60, CORES - HALF, 100), (1, 9, HALF, MEM - 100), (70, 2, CORES, MEM)])
        marks.append(a)
    arrays, s = pack_clusters(clusters), streams_of(per)
    oracle = oracle_of(arrays, s)
    assert not oracle[3]["flags"].any() and not oracle[3]["waited"].any()
    for c, a in enumerate(marks):
        assert nodes_of(oracle, s, c) == [a] * 4 and starts_of(oracle, s, c) == [0, 0, 1, 70]
        assert finishes_of(oracle, s, c)[0] == 1
    return arrays, s, oracle


def test_release_right_behind_a_placement(engine, diag):
    run_and_compare(engine, *case_release_behind_a_placement(), diag)


# ---- fuzz --------------------------------------------------------------------------------------------------------
def case_fuzz_crowded(seed):
    arrays, s = crowded(seed)
    oracle = oracle_of(arrays, s)
    assert not oracle[3]["flags"].any() and 5 * int(oracle[3]["waited"].sum()) >= int(s.job_off[-1])  # (a fifth wait)
    return arrays, s, oracle


@pytest.mark.parametrize("seed", [103, 110])
def test_fuzz_crowded_streams(engine, diag, seed):
    run_and_compare(engine, *case_fuzz_crowded(seed), diag)
