"""The streamed W16R loop's deferred slot insert ("Running jobs stay in their batch lane"): a
placed job takes no calendar slot while its batch is the current one.  Its finish sits in the batch's LIVE
column, every clock advance compares that column beside the calendar row, a job that finishes inside its
batch is released from its lane, and at the batch end the live lanes go into their calendar rows together
(a row with more candidates than free lanes spills the rest one at a time).  None of this shows in a
placement unless it goes wrong, so every case is a bit-exact parity run against the oracle (node, start,
finish, t_end, placed, waited, peak_running, flags) on a stream built to drive one of those places, on the
production and the counting build, with the kernel asserted and the counting build's iterations and
release_scans checked against a replay of the clock (the helpers of test_gpu_calendar_rows.py).  What a case
relies on (the job really finishes before its batch ends, the rows really hold that many) is asserted from
the oracle's results on the CPU before the GPU runs.  The cases pin behaviour that does not change: they
pass on the loop with the per-job insert as well.  Run on a real MI355X: ``pytest -m gpu``.

A batch is 64 consecutive jobs of a stream (job i runs in lane i & 63 of batch i >> 6), and its end is
reached when job 64 * (b + 1) is read, or never for the stream's last batch.  pad() fills a stream with
zero-duration jobs (they take neither a lane of LIVE nor a slot) up to a given lane.  A job in lane 63 is
the last of its batch.  Placed by the pass, it is followed by the batch end at once (the record read finds
no next job), so it cannot finish inside its batch: its case is the release from the calendar row right
after the move.  Placed as a waiting head, it sleeps its one second before anything tests for the batch
end, so a head of one second in lane 63 does finish inside its batch, with the batch end right behind the
release (test_waiting_head_in_lane_63_finishes_inside_its_batch)."""
import numpy as np
import pytest

from kat_util import fuzz_workload
from mcs_amd import Engine, JobStreams, pack_clusters, uniform_cluster
from mcs_amd.cluster import Cluster, Node
from test_gpu_calendar_rows import (BIG, FAR, LANES, MID, POOL, TINY, big_node_clusters, diag,  # noqa: F401
                                    residue_workload, run_and_compare, running_at, streams_of, ticks, tiny,
                                    uniform_for)
from test_gpu_wait_section import completions_in, crowded, oracle_of, span, starts_of

pytestmark = pytest.mark.gpu

NODE = (32, 1)  # a request that takes a whole node of uniform_cluster: job after job on the next node


def pad(rows, lane, t):
    """Zero-duration TINY jobs arriving at t until the next job's lane is `lane`."""
    return rows + [(t, 0, *TINY)] * ((lane - len(rows)) % LANES)


def batch_of(i):
    return i >> 6


def nodes_of(oracle, s, c):
    j0, j1 = span(s, c)
    return oracle[0][j0:j1].tolist()


def finishes_of(oracle, s, c):
    j0, j1 = span(s, c)
    return oracle[2][j0:j1].tolist()


# ---- a job that finishes inside its own batch ------------------------------------------------------------
VARIANTS = ("empty_row", "row_expires", "two_same_node", "two_other_node")


def inside_stream(lane, variant):
    """One round per residue k of the finish second F (F & 7 = k), 2048 s apart.  A round is two batches.
    The first holds job X alone (the rest zero-duration), which the batch end moves into its calendar row;
    X finishes at F (row_expires) or 20 s after it.  In the second the jobs before `lane` run 40 s (they
    are live beside the job, in other rows), job S in `lane` arrives at F - 1 and runs one second, and the
    job behind it arrives at F: a one-second advance inside the batch.  two_*: a second one-second job S2
    next to S, on node 0 as S (TINY) or on the next node (NODE requests)."""
    rows, marks = [], []
    two = variant.startswith("two")
    req = NODE if variant == "two_other_node" else TINY
    for k in range(8):
        F = 2048 * (k + 1) + k
        rows = pad(rows, 0, F - 200)
        rows += [(F - 100, 100 if variant == "row_expires" else 120, *TINY)]
        rows = pad(rows, 0, F - 100)
        first = lane - 1 if two and lane else lane  # (S2 sits before S, or behind it in lane 0)
        rows += tiny(F - 3, [40] * first)
        s_at = len(rows) + (1 if two and lane else 0)
        rows += [(F - 1, 1, *req)] * (2 if two else 1)
        marks.append((F, s_at, len(rows)))
        rows += tiny(F, [40] * (LANES - len(rows) % LANES)) if len(rows) % LANES else []
    return pad(rows, 0, 2048 * 10) + tiny(2048 * 10, [5] * 70), marks


@pytest.mark.parametrize("variant", VARIANTS)
def test_job_finishes_inside_its_batch(engine, diag, variant):
    lanes = (0, 31, 62) if not variant.startswith("two") else (0, 31, 61)
    built = [inside_stream(lane, variant) for lane in lanes]
    per = [b[0] for b in built]
    arrays, s = uniform_for(per), streams_of(per)
    oracle = oracle_of(arrays, s)
    stats = oracle[3]  # (on the CPU, first)
    assert not stats["flags"].any() and not stats["waited"].any()
    for c, (lane, (_, marks)) in enumerate(zip(lanes, built)):
        st, fin, nd = starts_of(oracle, s, c), finishes_of(oracle, s, c), nodes_of(oracle, s, c)
        for k, (F, s_at, behind) in enumerate(marks):
            assert F & 7 == k and s_at & 63 == lane and batch_of(s_at) == batch_of(behind)  # same batch
            assert (st[s_at], fin[s_at], st[behind]) == (F - 1, F, F)
            other = [f for i, f in enumerate(fin) if f == F and batch_of(i) < batch_of(s_at)]
            assert len(other) == (variant == "row_expires")  # the calendar row of that second
            if variant.startswith("two"):
                s2 = s_at - 1 if lane else s_at + 1
                assert fin[s2] == F and (nd[s2] == nd[s_at]) == (variant == "two_same_node")
    run_and_compare(engine, arrays, s, oracle, diag)


def test_last_lane_is_released_from_its_calendar_row(engine, diag):
    """Job 63 of a batch runs one second and job 0 of the next batch arrives a second (cluster 0) or two
    (cluster 1: every row is scanned) later, for every residue of that second: job 63 is placed by the pass
    (it does not wait), so the batch end lies between the placement and the release."""
    per = []
    for gap in (1, 2):
        rows = []
        for k in range(8):
            F = 2048 * (k + 1) + k
            rows = pad(rows, 0, F - 9) + tiny(F - 5, [30] * 63) + [(F - 1, 1, *TINY), (F - 1 + gap, 3, *TINY)]
        per.append(rows + tiny(2048 * 10, [5] * 70))
    arrays, s = uniform_for(per), streams_of(per)
    oracle = oracle_of(arrays, s)
    assert not oracle[3]["flags"].any() and not oracle[3]["waited"].any()  # (on the CPU, first)
    for c, gap in enumerate((1, 2)):
        st, fin = starts_of(oracle, s, c), finishes_of(oracle, s, c)
        last = [i for i in range(len(st)) if i & 63 == 63 and fin[i] == st[i] + 1]
        assert len(last) >= 8 and all(st[i + 1] == fin[i] - 1 + gap for i in last[:8])
    run_and_compare(engine, arrays, s, oracle, diag)


# ---- every way the clock reaches a batch-lane expiry -----------------------------------------------------
GAPS = (1, 2, 7, 8, 600)


def test_expiry_reached_by_an_arrival_gap(engine, diag):
    """Job S in lane 10 runs d seconds and the job behind it arrives g seconds after S: d = g (the expiry
    at the arrival's second) and d = 1 (inside the gap; for g = 1 the same), with other jobs of the batch
    live beside it, from two residues of the clock."""
    per = []
    for first in (0, 5):
        rows, t = [], 1000 + first
        for g in GAPS:
            for d in sorted({g, 1}):
                rows = pad(rows, 7, t - 1) + tiny(t - 1, [900] * 3) + [(t, d, *TINY), (t + g, 2, *TINY)]
                t += 2048 + 1
        per.append(rows + tiny(t + 2048, [5] * 70))
    arrays, s = uniform_for(per), streams_of(per)
    oracle = oracle_of(arrays, s)
    assert not oracle[3]["flags"].any() and not oracle[3]["waited"].any()  # (on the CPU, first)
    for c in range(2):
        st, fin = starts_of(oracle, s, c), finishes_of(oracle, s, c)
        at = [i for i in range(len(st) - 70) if i & 63 == 10]
        assert len(at) == 2 * len(GAPS) - 1
        assert sorted({st[i + 1] - st[i] for i in at}) == sorted(GAPS) and all(fin[i] <= st[i + 1] for i in at)
    run_and_compare(engine, arrays, s, oracle, diag)


def head_stream(kind):
    """A BIG head H that waits for a BIG job B of its own batch (one_big_node: one BIG job at a time), so
    the release that lets it in comes from B's batch lane.  -> rows, H's index, H's start, the start of the
    job behind H"""
    T = 1003
    rows = pad([], 5, T - 1)
    if kind in ("step1", "step8", "exact"):  # B finishes 1, 8 or 20 s after the failed fit (nothing else runs)
        k = {"step1": 1, "step8": 8, "exact": 20}[kind]
        rows += [(T, k, *BIG), (T, 5, *BIG), (T, 2, *TINY)]
        return rows, len(rows) - 2, T + k, T + k + 1
    if kind == "refail":  # a MID job's lane release at T + 6 fails it again
        rows += [(T, 12, *BIG), (T, 6, *MID), (T + 4, 5, *BIG), (T + 4, 2, *TINY)]
        return rows, len(rows) - 2, T + 12, T + 13
    if kind == "zero_head":
        rows += [(T, 9, *BIG), (T + 2, 0, *BIG), (T + 2, 1, *TINY)]
        return rows, len(rows) - 2, T + 9, T + 10
    assert kind == "placed_step"  # a TINY job of the batch finishes in the placed head's one-second sleep
    rows += [(T, 5, *BIG), (T, 6, *TINY), (T, 5, *BIG), (T, 1, *TINY)]
    return rows, len(rows) - 2, T + 5, T + 6


HEADS = ("step1", "step8", "exact", "refail", "zero_head", "placed_step")


def test_waiting_head_and_batch_lane_releases(engine, diag):
    built = [head_stream(kind) for kind in HEADS]
    per = [b[0] + tiny(4000, [5] * 70) for b in built]
    arrays, s = big_node_clusters(per), streams_of(per)
    oracle = oracle_of(arrays, s)
    stats = oracle[3]  # (on the CPU, first)
    assert not stats["flags"].any() and stats["waited"].tolist() == [1] * len(HEADS)
    for c, (kind, (_, head, placed, follow)) in enumerate(zip(HEADS, built)):
        st = starts_of(oracle, s, c)
        assert batch_of(head + 1) == 0 and st[head:head + 2] == [placed, follow]
        assert completions_in(oracle, s, c, 1003, placed) == ([1009] if kind == "refail" else [])
        if kind == "placed_step":
            assert finishes_of(oracle, s, c)[head - 1] == follow
    run_and_compare(engine, arrays, s, oracle, diag)


def last_lane_head_stream(k, gap):
    """One round per residue r of the second F at which the head finishes (F & 7 = r), 2048 s apart: the BIG
    job B in lane 62 runs k seconds from T, the BIG head H in lane 63 arrives with it, runs one second and
    waits for it, and job 64 of the round, the next batch's first, has arrived as well (gap 1) or arrives
    gap seconds after H's placement.  H is let in by B's batch-lane release at T + k, takes lane 63, which
    sets the cursor to the batch end, and sleeps its second to F = T + k + 1 before anything tests for the
    batch end: the expiry of lane 63 is found in the row block of F (the full scan's ninth row for a gap of
    two and more), and the batch ends right behind the release.  -> rows, [(H's index, F)]"""
    rows, marks = [], []
    for r in range(8):
        F = 2048 * (r + 1) + r
        T = F - k - 1
        rows = pad(rows, 62, T - 1) + [(T, k, *BIG), (T, 1, *BIG)]
        marks.append((len(rows) - 1, F))
        rows += [(T if gap == 1 else F - 1 + gap, 2, *TINY)]
    return rows + tiny(2048 * 10, [5] * 70), marks


def misplaced_last_lane_head_stream():
    """The head's one-second step finds a misplaced slot due and goes to the full scan: 64 TINY jobs fill
    calendar row 3, job 64 (due at 35) is misplaced at its batch end, and in the third batch B (lane 62)
    runs from 33 to 34 and H (lane 63) from 34 to 35.  -> rows, [(H's index, 35)]"""
    rows = tiny(0, [FAR + 3] * 64) + pad([(0, 35, *TINY)], 0, 0) + pad([], 62, 0) + [(33, 1, *BIG), (33, 1, *BIG)]
    return rows + [(33, 2, *TINY)] + tiny(300, [5] * 70), [(len(rows) - 1, 35)]


def test_waiting_head_in_lane_63_finishes_inside_its_batch(engine, diag):
    built = [last_lane_head_stream(1, 1), last_lane_head_stream(3, 1), last_lane_head_stream(1, 2),
             misplaced_last_lane_head_stream()]
    per = [b[0] for b in built]
    arrays, s = big_node_clusters(per), streams_of(per)
    oracle = oracle_of(arrays, s)
    stats = oracle[3]  # (on the CPU, first)
    assert not stats["flags"].any() and stats["waited"].tolist() == [8, 8, 8, 1]
    for c, (_, marks) in enumerate(built):
        st, fin = starts_of(oracle, s, c), finishes_of(oracle, s, c)
        assert sorted(F & 7 for _, F in marks) == (list(range(8)) if c < 3 else [3])
        for head, F in marks:
            assert head & 63 == 63 and st[head] > st[head - 1]  # lane 63, and it waited
            assert fin[head - 1] == st[head] == F - 1 and fin[head] == F  # let in by B's release, one second
            assert st[head + 1] >= F  # H finishes before job 64 of the round starts: inside its batch
            assert st[head + 1] == (F + 1 if c == 2 else F)
    assert [i for i, f in enumerate(finishes_of(oracle, s, 3)) if f == 35] == [64, built[3][1][0][0]]
    assert running_at(oracle, *span(s, 3), 0) == (65, 65)  # row 3 holds more than it has lanes: job 64 is misplaced
    run_and_compare(engine, arrays, s, oracle, diag)


def test_misplaced_slot_and_batch_lane_due_in_one_second(engine, diag):
    """64 TINY jobs fill calendar row 3, the next batch's job due at 35 is misplaced at its batch end, and a
    job of the third batch, still in its lane, finishes at 35 as well: the one-second advance to 35 finds
    the misplaced slot due and scans every row, the batch lanes among them."""
    rows = tiny(0, [FAR + 3] * 64) + pad([(0, 35, *TINY)], 0, 0) + ticks(1, 30, 0) + [(30, 5, *TINY)] \
        + ticks(31, 41, 0)
    per = [rows + tiny(300, [5] * 90)] * 2
    arrays, s = uniform_for(per), streams_of(per)
    oracle = oracle_of(arrays, s)
    assert not oracle[3]["flags"].any() and not oracle[3]["waited"].any()  # (on the CPU, first)
    st, fin = starts_of(oracle, s, 0), finishes_of(oracle, s, 0)
    assert running_at(oracle, *span(s, 0), 0) == (65, 65)
    assert [i for i, f in enumerate(fin) if f == 35 and st[i] < 35] == [64, 157]
    assert batch_of(157) == batch_of(157 + 10) == 2
    run_and_compare(engine, arrays, s, oracle, diag)


# ---- the bulk move ---------------------------------------------------------------------------------------
def test_bulk_move(engine, diag):
    """0: a batch of 64 zero-duration jobs: nothing to move.
    1: 64 jobs of one residue into an empty row: they fill it exactly.
    2: 54 jobs of residue 0, then 64 more into the row's 10 free lanes: 54 spill into the next rows, and the
       clock then visits the seconds at which they are due one by one (the full scan, XMIN rebuilt).
    3: rows 0-6 hold 63 slots each and a batch brings two jobs for each of them: every one of those rows
       is short by one, and the seven left over end in row 7."""
    short = [(0, FAR + i % 7, *TINY) for i in range(7 * 63)]
    per = [
        [(0, 0, *TINY)] * 64 + tiny(1, [7] * 3),
        tiny(0, [80] * 64) + ticks(1, 90, 0),
        pad(tiny(0, [FAR] * 54), 0, 0) + tiny(0, [16 + 8 * (i % 6) for i in range(64)]) + ticks(1, 70, 0),
        pad(short, 0, 0) + [(0, FAR + i % 7, *TINY) for i in range(14)] + ticks(1, 20, 0),
    ]
    per = [rows + tiny(2000, [5] * 70) for rows in per]
    arrays, s = uniform_for(per), streams_of(per)
    oracle = oracle_of(arrays, s)
    assert not oracle[3]["flags"].any() and not oracle[3]["waited"].any()  # (on the CPU, first)
    assert running_at(oracle, *span(s, 1), 0) == (64, 64) and running_at(oracle, *span(s, 2), 0) == (118, 118)
    live = np.array(finishes_of(oracle, s, 3)[:7 * 63 + 64 - 7 * 63 % 64 + 14])
    assert np.bincount(live[live >= FAR] & 7, minlength=8).tolist() == [65] * 7 + [0]
    run_and_compare(engine, arrays, s, oracle, diag)


def test_bulk_move_keeps_each_entrys_request_and_node(engine, diag):
    """The three words of a moved entry.  Only 64 scattered nodes have cores; the 64 jobs of one batch ask
    for 17 ... 32 cores and 64 different amounts of memory, so each takes a node of its own and no two
    entries of the move carry the same request or the same node.  They finish at 23 different seconds in
    every calendar row (cluster 0), or at three seconds of row 0, which has four free lanes: 60 of them are
    surplus (cluster 1).  From the first finish on, a job that asks for a whole node (all its cores and all
    its memory) arrives every second: it fits a node only once that node has got back exactly what its job
    took, so a request or an address swapped between two entries shows in where and when those jobs run."""
    free = [3 * i + 1 for i in range(LANES)]
    batch = [(17 + i % 16, 1000 + 37 * i) for i in range(LANES)]
    whole = [(40 + i, 300, 32, 24000) for i in range(LANES)]
    per = [
        [(0, 40 + 5 * i % 23, *batch[i]) for i in range(LANES)] + whole,
        pad(tiny(0, [FAR] * 60), 0, 0) + [(0, 40 + 8 * (i % 3), *batch[i]) for i in range(LANES)] + whole,
    ]
    arrays, s = pack_clusters([only_free(200, free)] * 2), streams_of(per)
    oracle = oracle_of(arrays, s)
    stats = oracle[3]  # (on the CPU, first)
    assert not stats["flags"].any() and stats["placed"].tolist() == [len(r) for r in per]
    assert len(set(batch)) == LANES and min(b[0] for b in batch) > 16
    for c, first in enumerate((0, LANES)):
        nd, st, fin = nodes_of(oracle, s, c), starts_of(oracle, s, c), finishes_of(oracle, s, c)
        assert nd[first:first + LANES] == free and st[first:first + LANES] == [0] * LANES  # a node each
        assert sorted(nd[first + LANES:]) == free  # every node is whole again
        assert all(st[first + LANES + i] >= fin[first + free.index(n)] for i, n in enumerate(nd[first + LANES:]))
        rows = np.bincount(np.array(fin[first:first + LANES]) & 7, minlength=8).tolist()
        assert (min(rows) > 0) if c == 0 else (rows == [LANES] + [0] * 7)
    assert running_at(oracle, *span(s, 1), 0) == (60 + LANES, 60 + LANES)  # row 0: 124 for 64 lanes
    run_and_compare(engine, arrays, s, oracle, diag)


# ---- the pool --------------------------------------------------------------------------------------------
def test_pool_exactly_full_at_a_batch_end(engine, diag):
    """512 running when the eighth batch ends, of one residue and of all eight: no escalation; and 448 in
    the table with the eighth batch in its lanes, one of them released and the batch's last job placed at
    second 8 (an arrival gap: every row and the lanes are scanned): the batch end finds 511, the most a
    batch with a release inside it can leave."""
    per = [
        tiny(0, [80] * POOL) + ticks(1, 90, 0),
        tiny(0, [80 + i % 8 for i in range(POOL)]) + ticks(1, 90, 0),
        tiny(0, [80] * (POOL - 2) + [8]) + tiny(8, [72]) + ticks(9, 90, 0),
    ]
    per = [rows + tiny(200, [3] * 70) for rows in per]
    arrays, s = uniform_for(per), streams_of(per)
    oracle = oracle_of(arrays, s)
    stats = oracle[3]  # (on the CPU, first)
    assert stats["peak_running"].tolist() == [POOL, POOL, POOL - 1] and not stats["waited"].any() and not stats["flags"].any()
    assert batch_of(POOL - 2) == batch_of(POOL - 1) == 7 and running_at(oracle, *span(s, 2), 8)[0] == POOL - 1
    assert finishes_of(oracle, s, 2)[POOL - 2] == 8 == starts_of(oracle, s, 2)[POOL - 1]
    cs = run_and_compare(engine, arrays, s, oracle, diag)
    assert not cs["flags"].any()


@pytest.mark.parametrize("shift", [0, 1], ids=["table512_lane1", "table511_lanes2"])
def test_pool_of_513_escalates_once(diag, shift):
    """513 running jobs: with 512 in the table and one in its lane, and (a zero-duration job in front) with
    511 in the table and two in their lanes; the count passes the pool inside the batch, the batch end
    hands the cluster to a larger pool (an engine of its own: the larger pool stays with the engine)."""
    per = [[(0, 0, *TINY)] * shift + tiny(0, [80] * (POOL + 1)) + ticks(1, 90, 0) + tiny(90, [3] * 70)]
    arrays, s = uniform_for(per), streams_of(per)
    oracle = oracle_of(arrays, s)
    assert oracle[3]["peak_running"].tolist() == [POOL + 1]  # (on the CPU, first)
    with Engine(0) as eng:
        cs = run_and_compare(eng, arrays, s, oracle, diag, escalations=1)
    assert (cs["peak_running"] > POOL).all()


# ---- stream lengths ----------------------------------------------------------------------------------------
LENGTHS = (1, 63, 64, 65, 128, 129)


def test_stream_lengths(engine, diag):
    """Three jobs a second with durations 1 ... 13: the stream ends with jobs still in their lanes, at a
    batch end, and one job after it."""
    per = [[(i // 3, (i % 5) * 3 + 1, *TINY) for i in range(J)] for J in LENGTHS]
    for group in (per[:4], per[4:]):
        arrays, s = uniform_for(group), streams_of(group)
        oracle = oracle_of(arrays, s)
        assert not oracle[3]["flags"].any() and oracle[3]["placed"].tolist() == [len(r) for r in group]
        run_and_compare(engine, arrays, s, oracle, diag)


# ---- a batch-lane release hands its request back to the right node -------------------------------------------
def only_free(n, free):
    return Cluster(Id=1, Nodes=[Node(Id=i + 1, Cores=32, Memory=24000, CoresAvailable=32 if i in free else 0,
                                     MemoryAvailable=24000) for i in range(n)])


def test_batch_lane_release_returns_requests_to_edge_nodes(engine, diag):
    """Only nodes 0, 3, 252, 255 (and 0, 3, 128 of a 129-node cluster) have cores.  A 32-core job goes to
    each and they finish 3 s apart; each of the 32-core heads behind them, in the same batch, fails, sleeps
    to the next of those completions and fits that node only."""
    per, targets = [], ([0, 3, 252, 255], [0, 3, 128])
    for tg in targets:
        per.append([(0, 5 + 3 * i, *NODE) for i in range(len(tg))] + [(2, 300, *NODE)] * len(tg) + tiny(40, [5] * 10))
    arrays = pack_clusters([only_free(256, targets[0]), only_free(129, targets[1])])
    s = streams_of(per)
    oracle = oracle_of(arrays, s)
    stats = oracle[3]  # (on the CPU, first)
    assert not stats["flags"].any() and stats["waited"].tolist() == [4, 3]
    for c, tg in enumerate(targets):
        nd, st = nodes_of(oracle, s, c), starts_of(oracle, s, c)
        assert nd[:2 * len(tg)] == tg + tg and st[len(tg):2 * len(tg)] == [5 + 3 * i for i in range(len(tg))]
    run_and_compare(engine, arrays, s, oracle, diag)


# ---- fuzz ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [81, 85])
def test_fuzz_crowded_streams(engine, diag, seed):
    arrays, s = crowded(seed)
    oracle = oracle_of(arrays, s)
    assert not oracle[3]["flags"].any() and 5 * int(oracle[3]["waited"].sum()) >= int(s.job_off[-1])  # (a fifth wait)
    run_and_compare(engine, arrays, s, oracle, diag)


def test_fuzz_short_durations(engine, diag):
    """Durations of at most 8 s: most jobs finish before their batch ends."""
    arrays, s = fuzz_workload("w16r", 83, n_clusters=4, J=400, blocking=False)
    s = JobStreams(s.arrival, s.dur % 9, s.cores, s.mem, s.job_off)
    oracle = oracle_of(arrays, s)
    st, fin = oracle[1], oracle[2]  # (on the CPU, first)
    inside = sum(int(fin[i] > st[i] and (i - j0 | 63) + 1 < j1 - j0 and fin[i] <= st[j0 + (i - j0 | 63) + 1])
                 for c in range(4) for j0, j1 in [span(s, c)] for i in range(j0, j1))
    assert not oracle[3]["flags"].any() and 2 * inside > int(s.job_off[-1])
    run_and_compare(engine, arrays, s, oracle, diag)


def test_fuzz_one_residue_bursts(engine, diag):
    per = residue_workload(84, n_clusters=2, J=800)
    arrays = pack_clusters([uniform_cluster(256), uniform_cluster(129)])
    s = streams_of(per)
    oracle = oracle_of(arrays, s)
    stats = oracle[3]  # (on the CPU, first)
    assert not stats["flags"].any() and stats["waited"].all() and (stats["peak_running"] <= POOL).all()
    j0, j1 = span(s, 0)  # rows overflow: more than 64 running jobs are due in one calendar row
    assert max(running_at(oracle, j0, j1, int(t))[1] for t in np.unique(oracle[1][j0:j1])) > LANES
    run_and_compare(engine, arrays, s, oracle, diag)
