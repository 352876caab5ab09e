"""The streamed W16R loop's calendar slot rows ("Calendar rows"): a running slot lives in
row finish & 7 of the 8 x 64 pool, a clock advance compares one row, a slot whose row is full is
misplaced into the next row with a free lane and found through the earliest misplaced finish (XMIN),
and a failed fit sleeps second by second, after eight seconds to the exact earliest finish.  None of
this shows in a placement unless it goes wrong, so every case is a bit-exact parity run against the
oracle (node, start, finish, t_end, placed, waited, peak_running, flags) on a stream built to drive one
of those places; what a case relies on is asserted from the oracle's results on the CPU before the GPU
runs.  A release that is missed or done twice shows in peak_running: every stream ends with a burst
that takes the running count to a new peak.  Every stream runs on the production and the counting
build and asserts the kernel it ran on; the counting build's iterations and release_scans are checked
against a replay of the loop's clock from the oracle's start and finish seconds.  The cases pin
behaviour that does not change: they pass on the loop as it was before as well.  Run on a real MI355X:
``pytest -m gpu``.

Clusters are uniform_cluster(n) (32 cores, 24000 MB a node), where a TINY request (1 MB) always fits,
and one_big_node(n): node 0 holds 24000 MB and every other node 100 MB, so a BIG request (20000 MB)
runs on node 0 alone, one at a time, beside any number of TINY ones."""
import heapq

import numpy as np
import pytest

import oracle_ref as O
from kat_util import fuzz_workload
from mcs_amd import MCS_FLAG_DEADLOCK, MCS_FLAG_OVERFLOW, Engine, JobStreams, pack_clusters, uniform_cluster
from mcs_amd.cluster import Cluster, Node

pytestmark = pytest.mark.gpu

W16R = "mcs::fifo_asm_kernel<16, true, 4, 8>"
NODES = (256, 129, 200, 255)  # the W16R shape: no padding, padding lanes and chunks
BIG = (1, 20000)
MID = (1, 50)
TINY = (0, 1)
NEVER = (1, 30000)  # no node holds it
POOL, LANES = 512, 64


@pytest.fixture(params=["0", "1"], ids=["prod", "diag"])
def diag(request, monkeypatch):
    monkeypatch.setenv("MCS_FIFO_DIAG", request.param)
    return request.param


def streams_of(per_cluster):
    """JobStreams from one list of (arrival, duration, cores, memory) rows per cluster."""
    cols = [np.array([r[f] for rows in per_cluster for r in rows], np.uint32) for f in range(4)]
    off = np.cumsum([0] + [len(rows) for rows in per_cluster]).astype(np.uint64)
    return JobStreams(*cols, off)


def one_big_node(n):
    return Cluster(Id=1, Nodes=[Node(Id=i + 1, Cores=32, Memory=24000 if i == 0 else 100, CoresAvailable=32,
                                     MemoryAvailable=24000 if i == 0 else 100) for i in range(n)])


def big_node_clusters(per):
    return pack_clusters([one_big_node(NODES[i % len(NODES)]) for i in range(len(per))])


def uniform_for(per):
    return pack_clusters([uniform_cluster(NODES[i % len(NODES)]) for i in range(len(per))])


def tiny(t, durs):
    return [(t, int(d), *TINY) for d in durs]


def ticks(t0, t1, dur=1):
    """One TINY job a second: the clock visits every second of [t0, t1) (dur 0: without a slot)."""
    return [(t, dur, *TINY) for t in range(t0, t1)]


def replay(arr, dur, start, finish):
    """The loop's clock from a cluster's placements (tools/scan_rows_model.py): the passes without a
    decision (arrival advances and failed fits) and the clock advances that release something."""
    heap, t, slow, scans = [], 0, 0, 0

    def advance():
        nonlocal scans
        if heap and heap[0] <= t:
            scans += 1
            while heap and heap[0] <= t:
                heapq.heappop(heap)

    for k in range(len(arr)):
        if arr[k] > t:
            t, slow = int(arr[k]), slow + 1
            advance()
        waited = False
        while int(start[k]) != t:  # a failed fit: the head sleeps to the next completion
            assert int(start[k]) > t and heap
            waited, slow = True, slow + 1
            t = max(t + 1, heap[0])
            advance()
        if dur[k]:
            heapq.heappush(heap, int(finish[k]))
        if waited:  # a placed WaitQueue head sleeps one second
            t += 1
            advance()
    return slow, scans


def run_and_compare(engine, arrays, streams, oracle, diag, escalations=0):
    on, os_, of, osd = oracle
    engine.load_clusters(arrays)
    engine.submit_jobs(streams)
    st = engine.run()
    node, start, fin = engine.placements()
    cs = engine.cluster_stats()
    assert engine.last_kernel == W16R
    bad = np.nonzero((node != on) | (start != os_) | (fin != of))[0]
    assert bad.size == 0, f"{bad.size} mismatches, first at job {bad[:5]}: gpu {node[bad[:5]]},{start[bad[:5]]} " \
                          f"oracle {on[bad[:5]]},{os_[bad[:5]]}"
    for key in ("t_end", "placed", "waited", "peak_running", "flags"):
        np.testing.assert_array_equal(cs[key], osd[key], err_msg=key)
    assert st.escalations == escalations
    if diag == "1" and not escalations:  # the counting build: passes and release scans
        for c in range(arrays.n_clusters):
            if osd["flags"][c]:
                continue
            j0, j1 = int(streams.job_off[c]), int(streams.job_off[c + 1])
            slow, scans = replay(streams.arrival[j0:j1], streams.dur[j0:j1], os_[j0:j1], of[j0:j1])
            assert (int(cs["iterations"][c]), int(cs["release_scans"][c])) == (j1 - j0 + slow, scans), c
    return cs


def running_at(oracle, j0, j1, t):
    """(running jobs, the largest number of them in one calendar row) at second t, arrivals at t placed."""
    live = (oracle[1][j0:j1] <= t) & (oracle[2][j0:j1] > t)
    return int(live.sum()), int(np.bincount(oracle[2][j0:j1][live] & 7, minlength=8).max())


# ---- a full row: misplaced slots -------------------------------------------------------------------
FAR = 800


def spill_streams():
    """70 TINY jobs at t = 0 whose finishes share one calendar row: the last 6 find it full.
    0: the misplaced slots are due at 16 ... 56, seconds at which their calendar row has no expiry (its
       regular slots finish at 800), one after the other: XMIN is rebuilt with 5 ... 1 of them alive;
    1: the misplaced slot due at 24 shares its second with regular slots of the row;
    2: residue 3, the row's regular slots expire at 11 and 19, the misplaced ones at 27 and 35 beside
       regular slots placed later into the lanes those freed."""
    a = tiny(0, [FAR] * 64 + [16, 24, 32, 40, 48, 56]) + ticks(1, 60) + tiny(60, [5] * 80)
    b = tiny(0, [FAR] * 60 + [24] * 4 + [24, 40, 40, 48, 56, 64]) + ticks(1, 70) + tiny(70, [5] * 80)
    c = tiny(0, [FAR + 3] * 50 + [11] * 7 + [19] * 7 + [27, 27, 35, 35, 43, 51]) + ticks(1, 11, 3) \
        + tiny(11, [16, 24]) + ticks(12, 60, 2) + tiny(60, [5] * 80)
    return [a, b, c]


def test_row_full(engine, diag):
    per = spill_streams()
    arrays, s = uniform_for(per), streams_of(per)
    oracle = O.fifo_run_batch(arrays, s, n_threads=4)
    stats = oracle[3]  # (on the CPU, first)
    assert not stats["flags"].any() and not stats["waited"].any()
    for c in range(3):
        assert running_at(oracle, int(s.job_off[c]), int(s.job_off[c + 1]), 0) == (70, 70)
    assert stats["peak_running"].tolist() == [64 + 80, 60 + 80, 50 + 80 + 1]
    run_and_compare(engine, arrays, s, oracle, diag)


def test_misplaced_slot_due_in_a_failed_fits_sleep(engine, diag):
    """A head fails at 30 with misplaced slots due 5 s on (found by the XMIN test of a step; the retry
    fails again), 13 s on (after the eight steps: the exact minimum is a misplaced slot's finish) and
    then the BIG job's own finish, 8 steps after that."""
    rows = tiny(0, [FAR + 3] * 64 + [35, 43, 43, 67, 75, 83]) + [(0, 51, *BIG)] + ticks(1, 30) \
        + [(30, 4, *BIG)] + tiny(30, [2] * 5) + tiny(90, [5] * 90)
    per = [rows, rows]
    arrays, s = big_node_clusters(per), streams_of(per)
    oracle = O.fifo_run_batch(arrays, s, n_threads=4)
    stats = oracle[3]  # (on the CPU, first)
    head = 70 + 1 + 29
    assert not stats["flags"].any() and stats["waited"].tolist() == [1, 1]
    assert oracle[1][head] == 51 and oracle[1][head + 1] == 52
    run_and_compare(engine, arrays, s, oracle, diag)


# ---- the pool's bounds with one residue only ---------------------------------------------------------
def test_pool_exactly_full_of_one_row(engine, diag):
    """512 running, all due in one calendar row (64 regular and 448 misplaced slots): no escalation;
    and exactly full, one release, one insert, full again."""
    per = [
        tiny(0, [80] * POOL) + ticks(1, 90, 0) + tiny(90, [3] * 70),
        tiny(0, [80] * (POOL - 1) + [8]) + ticks(1, 8, 0) + tiny(8, [72]) + ticks(9, 90, 0) + tiny(90, [3] * 70),
    ]
    arrays, s = uniform_for(per), streams_of(per)
    oracle = O.fifo_run_batch(arrays, s, n_threads=4)
    assert oracle[3]["peak_running"].tolist() == [POOL, POOL]  # (on the CPU, first)
    assert running_at(oracle, int(s.job_off[1]), int(s.job_off[2]), 8) == (POOL, POOL)
    assert not oracle[3]["waited"].any() and not oracle[3]["flags"].any()
    cs = run_and_compare(engine, arrays, s, oracle, diag)
    assert not (cs["flags"] & MCS_FLAG_OVERFLOW).any()


def test_pool_of_513_in_one_row_escalates_once(diag):
    """513 running: the last insert finds no row with a free lane and is skipped, the count stays above
    the pool, and the cluster is run again with a larger pool (an engine of its own: the larger pool
    stays with the engine)."""
    per = [tiny(0, [80] * (POOL + 1)) + ticks(1, 90, 0) + tiny(90, [3] * 70)]
    arrays, s = uniform_for(per), streams_of(per)
    oracle = O.fifo_run_batch(arrays, s, n_threads=4)
    assert oracle[3]["peak_running"].tolist() == [POOL + 1]  # (on the CPU, first)
    with Engine(0) as eng:
        cs = run_and_compare(eng, arrays, s, oracle, diag, escalations=1)
    assert (cs["peak_running"] > POOL).all()


# ---- arrival gaps --------------------------------------------------------------------------------------
GAPS = (1, 2, 7, 8, 9, 1000)


def gap_stream(first):
    """Arrival gaps of 1 ... 1000 s from every residue of the clock (the k-th round starts at a second
    = first + k mod 8), each after a burst whose jobs finish 1 ... 12 s on: completions inside the gap
    at every residue, and gaps that reach none of them (the durations > gap stay for the next gaps)."""
    rows, t = [], first
    for k in range(8):
        for g in GAPS:
            rows += tiny(t, range(1, 13))
            t += g
        t += (first + k + 1 - t) % 8 + 1008  # (everything has finished; the next residue)
    return rows + tiny(t, [5] * 20)


def quiet_gap_stream():
    """The same gaps with nothing due in any of them."""
    rows, t = [], 3
    for g in GAPS * 2:
        rows += tiny(t, [50000] * 3)
        t += g
    return rows + tiny(t, [5] * 20)


def test_arrival_gaps(engine, diag):
    per = [gap_stream(0), gap_stream(5), quiet_gap_stream()]
    arrays, s = uniform_for(per), streams_of(per)
    oracle = O.fifo_run_batch(arrays, s, n_threads=4)
    stats = oracle[3]  # (on the CPU, first)
    assert not stats["flags"].any() and not stats["waited"].any()
    assert stats["peak_running"].tolist()[2] == 3 * 12 + 20
    for c in (0, 1):  # every residue of the clock sees a completion
        j0, j1 = int(s.job_off[c]), int(s.job_off[c + 1])
        assert set((oracle[2][j0:j1] & 7).tolist()) == set(range(8))
    run_and_compare(engine, arrays, s, oracle, diag)


# ---- failed fits -----------------------------------------------------------------------------------------
AHEAD = (1, 2, 8, 9, 600)


def ahead_stream(k):
    """The head fails at 10; the next completion, which lets it in, is k seconds on."""
    return [(0, 10 + k, *BIG), (10, 5, *BIG), (10, 2, *TINY), (10 + k + 1, 1, *TINY)] + tiny(10 + k + 700, [5] * 9)


def test_failed_fit_sleeps(engine, diag):
    """The next completion 1, 2, 8 (the last step), 9 (the first the exact minimum finds) and 600 s
    ahead; each stream also on a clock that starts at another residue (offset 3)."""
    per = [ahead_stream(k) for k in AHEAD]
    per = [per[0] + [(r[0] + 2003, *r[1:]) for r in per[1]], per[2], per[3] + [(r[0] + 2003, *r[1:]) for r in per[2]],
           per[4]]
    arrays, s = big_node_clusters(per), streams_of(per)
    oracle = O.fifo_run_batch(arrays, s, n_threads=4)
    stats = oracle[3]  # (on the CPU, first)
    assert not stats["flags"].any() and stats["placed"].tolist() == [len(rows) for rows in per]
    assert stats["waited"].tolist() == [2, 1, 2, 1]
    assert [int(oracle[1][int(s.job_off[c]) + 1]) for c in range(4)] == [11, 18, 19, 610]
    run_and_compare(engine, arrays, s, oracle, diag)


def test_failed_fit_at_three_completions_and_deadlocks(engine, diag):
    """A head that fails at its arrival and at three completions (4, 12 and 21 s apart: a step, the
    exact minimum, and a step again); a deadlock with nothing running, and one after earlier jobs ran
    (the head sleeps to their completion, fails again, and nothing runs any more)."""
    per = [
        [(0, 47, *BIG), (0, 4, *MID), (0, 16, *MID), (0, 37, *MID), (0, 5, *BIG), (0, 2, *TINY), (48, 1, *TINY)]
        + tiny(100, [5] * 9),
        [(0, 1, *NEVER), (1, 1, *TINY)],
        [(0, 10, *BIG), (0, 3, *TINY), (5, 1, *NEVER), (6, 1, *TINY)],
        [(3, 2, *NEVER)],
    ]
    arrays, s = big_node_clusters(per), streams_of(per)
    oracle = O.fifo_run_batch(arrays, s, n_threads=4)
    stats = oracle[3]  # (on the CPU, first)
    assert ((stats["flags"] & MCS_FLAG_DEADLOCK) != 0).tolist() == [False, True, True, True]
    assert stats["placed"].tolist() == [len(per[0]), 0, 2, 0] and stats["waited"].tolist() == [1, 1, 1, 1]
    assert oracle[1][4] == 47 and oracle[1][5] == 48
    run_and_compare(engine, arrays, s, oracle, diag)


# ---- stream lengths and batch boundaries ---------------------------------------------------------------
LENGTHS = (1, 63, 64, 65, 129)


def boundary_stream(J):
    """Three jobs a second, durations 1 ... 13, and zero-duration jobs at the batch boundaries."""
    return [(i // 3, 0 if i in (0, 63, 64, 127, 128) else (i % 5) * 3 + 1, *TINY) for i in range(J)]


def test_stream_lengths_and_batch_boundaries(engine, diag):
    per = [boundary_stream(J) for J in LENGTHS[:4]]
    for group in (per, [boundary_stream(LENGTHS[4]), [(7, 0, *TINY)]]):
        arrays, s = uniform_for(group), streams_of(group)
        oracle = O.fifo_run_batch(arrays, s, n_threads=4)
        assert not oracle[3]["flags"].any() and oracle[3]["placed"].tolist() == [len(r) for r in group]
        run_and_compare(engine, arrays, s, oracle, diag)


# ---- fuzz --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [41, 42])
def test_fuzz_streams(engine, diag, seed):
    arrays, s = fuzz_workload("w16r", seed, n_clusters=4, J=400)
    oracle = O.fifo_run_batch(arrays, s, n_threads=4)
    assert oracle[3]["waited"].any()  # (failed fits happen)
    run_and_compare(engine, arrays, s, oracle, diag)


def residue_workload(seed, n_clusters=3, J=1200):
    """Bursts of 70-140 simultaneous arrivals with durations drawn from the multiples of 8, so a burst's
    finishes share one calendar row; 16-32 cores a job, so a cluster of 256 nodes runs at most 512."""
    rng = np.random.default_rng(seed)
    per = []
    for _ in range(n_clusters):
        rows, t = [], 0
        while len(rows) < J:
            t += int(rng.integers(1, 12))
            for _ in range(min(int(rng.integers(70, 141)), J - len(rows))):
                rows.append((t, 8 * int(rng.integers(1, 9)), int(rng.integers(16, 33)), int(rng.integers(0, 12000))))
        per.append(rows)
    return per


@pytest.mark.parametrize("seed", [51, 52])
def test_fuzz_one_residue_bursts(engine, diag, seed):
    per = residue_workload(seed)
    arrays, s = uniform_for(per), streams_of(per)
    oracle = O.fifo_run_batch(arrays, s, n_threads=4)
    stats = oracle[3]  # (on the CPU, first)
    assert not stats["flags"].any() and stats["waited"].all() and (stats["peak_running"] <= POOL).all()
    for c in range(len(per)):  # rows overflow: more than 64 running jobs are due in one calendar row
        j0, j1 = int(s.job_off[c]), int(s.job_off[c + 1])
        assert max(running_at(oracle, j0, j1, int(t))[1] for t in np.unique(oracle[1][j0:j1])) > LANES
    run_and_compare(engine, arrays, s, oracle, diag)
