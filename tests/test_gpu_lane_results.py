"""The streamed W16R loop's result columns while a job runs in its batch lane ("Lane results"): a
live job has no start on record, only its finish in the LIVE column and its duration in the batch's records,
and the start is formed (finish - duration) where the lane leaves LIVE (the row blocks' batch-lane release,
the same in a waiting head's sleep, the full scan's ninth row), before the batch end's stores and at the exit;
the node and the finish are written for the job's own lane; and a calendar row is one register quad that the
bulk move's reads fill directly.  None of this shows in a placement unless it goes wrong, so every case is a
bit-exact parity run against the oracle (node, start, finish, t_end, placed, waited, peak_running, flags) on a
stream built to drive one of those places, on the production and the counting build, with the kernel asserted
and the counting build's iterations and release_scans checked against a replay of the clock (the helpers of
test_gpu_calendar_rows.py, test_gpu_wait_section.py and test_gpu_deferred_insert.py).  What a case relies on
(the job really leaves its lane inside its batch, the other lanes really are live at the batch end) is asserted
from the oracle's results on the CPU, in the case's builder, before the GPU runs.  The cases pin behaviour
that does not change: they pass on the loop that writes the start at the placement as well.  Run on a real
MI355X: ``pytest -m gpu``.

A batch is 64 consecutive jobs of a stream (job i runs in lane i & 63), and it ends when the job behind its
last one is read.  A job leaves its lane inside its batch when the clock reaches its finish before the
batch's last job is placed; a job placed by the pass in lane 63 never does, a WaitQueue head placed there
sleeps its second first, so it does with a duration of one second (test_gpu_deferred_insert.py)."""
import numpy as np
import pytest

from kat_util import fuzz_workload
from mcs_amd import MCS_FLAG_DEADLOCK, Engine, JobStreams, pack_clusters
from test_gpu_calendar_rows import (BIG, FAR, LANES, NEVER, POOL, TINY, big_node_clusters, diag,  # noqa: F401
                                    run_and_compare, running_at, streams_of, ticks, tiny, uniform_for)
from test_gpu_deferred_insert import (batch_of, finishes_of, misplaced_last_lane_head_stream, nodes_of,
                                      only_free, pad)
from test_gpu_wait_section import crowded, oracle_of, span, starts_of

pytestmark = pytest.mark.gpu

ROUND = 2048  # seconds between two rounds of a stream: whatever a round left running has finished
LIVE = 900    # a duration that outlasts its batch and ends before the next round


def last_of(i, n):
    """The last job of job i's batch in a stream of n jobs."""
    return min(i | 63, n - 1)


def leaves_inside(st, fin, i):
    """Job i's finish is reached by the clock before its batch's last job is placed."""
    return i != last_of(i, len(st)) and fin[i] > st[i] and fin[i] <= st[last_of(i, len(st))]


def live_at_batch_end(st, fin, i):
    return fin[i] > st[last_of(i, len(st))] and fin[i] > st[i]


# ---- the start is formed in every path out of LIVE -----------------------------------------------------------
PATHS = ("brel", "wbrel", "gap2", "gap600", "exact")


def leave_stream(lane):
    """One round per path, ROUND seconds apart.  A round is one batch: three TINY jobs that outlast it in its
    first lanes (fewer before lane 0 .. 2), zero-duration jobs up to `lane`, job X there, what makes X leave,
    two more TINY jobs that outlast the batch, and zero-duration jobs a few seconds on that end the batch.
    brel: X runs one second and the next job arrives a second on.  gap2 / gap600: the next job arrives 2 / 600
    s on and X finishes inside the gap (every row is scanned, the batch lanes as the ninth).  wbrel / exact: X
    is BIG and runs 3 / 20 s, the BIG head behind it fails, steps to X's finish second by second / jumps to
    it after eight steps (nothing but batch-lane jobs is running: the earlier rounds have finished), is let in
    by X's release from its lane and sleeps its second.  -> rows, {path: (X's index, start, finish)}"""
    rows, marks = [], {}
    for n, path in enumerate(PATHS):
        T = ROUND * (n + 1) + n  # (another residue of the clock each round)
        rows = pad(rows, 0, T - 2) + tiny(T - 2, [LIVE + 7 * i for i in range(min(lane, 3))])
        rows = pad(rows, lane, T - 2)
        x = len(rows)
        if path == "brel":
            rows += [(T, 1, *TINY), (T + 1, LIVE, *TINY)]
            marks[path], end = (x, T, T + 1), T + 3
        elif path in ("gap2", "gap600"):
            g = 2 if path == "gap2" else 600
            rows += [(T, g // 2, *TINY), (T + g, LIVE, *TINY)]
            marks[path], end = (x, T, T + g // 2), T + g + 2
        else:
            k = 3 if path == "wbrel" else 20
            rows += [(T, k, *BIG), (T, LIVE, *BIG)]
            marks[path], end = (x, T, T + k), T + k + 3
        rows += tiny(end - 1, [LIVE + 3, LIVE + 4][:LANES - len(rows) % LANES] if len(rows) % LANES else [])
        rows = pad(rows, 0, end)
    return rows + tiny(ROUND * (len(PATHS) + 2), [5] * 70), marks


def last_lane_stream():
    """Lane 63, placed as a WaitQueue head: B in lane 62 runs k seconds, the head H behind it runs one second,
    is let in by B's release and sleeps its second into the row block that finds its own expiry (k = 1: B left
    through the row block as well; k = 4: in H's sleep), three jobs of the batch still live.  (Lane 63 has no
    other way out of LIVE but this one and the full scan a misplaced slot asks for, which
    misplaced_last_lane_head_stream drives: a head behind it would lie in the next batch.)"""
    rows, marks = [], {}
    for n, k in enumerate((1, 4)):
        T = ROUND * (n + 1) + 3 * n
        rows = pad(rows, 0, T - 2) + tiny(T - 2, [LIVE, LIVE + 9, LIVE + 18])
        rows = pad(rows, 62, T - 2) + [(T, k, *BIG), (T, 1, *BIG)]
        marks[k] = (len(rows) - 1, T + k, T + k + 1)
        rows += [(T, 2, *TINY)]
    return rows + tiny(ROUND * 4, [5] * 70), marks


def case_leaving_paths():
    lanes = (0, 31, 62)
    built = [leave_stream(lane) for lane in lanes]
    per = [b[0] for b in built]
    arrays, s = big_node_clusters(per), streams_of(per)
    oracle = oracle_of(arrays, s)
    stats = oracle[3]
    assert not stats["flags"].any() and stats["waited"].tolist() == [2, 2, 2]
    for c, lane in enumerate(lanes):
        st, fin = starts_of(oracle, s, c), finishes_of(oracle, s, c)
        for path, (x, t0, t1) in built[c][1].items():
            assert x & 63 == lane and (st[x], fin[x]) == (t0, t1) and leaves_inside(st, fin, x), (lane, path)
            mates = [i for i in range(x & ~63, (x | 63) + 1) if i != x and live_at_batch_end(st, fin, i)]
            assert len(mates) >= 3 and len({st[i] for i in mates}) >= 2, (lane, path)  # live beside X, to the batch end
            if path in ("wbrel", "exact"):  # the head behind X waited for it, and nothing else finished meanwhile
                assert (st[x + 1], fin[x + 1]) == (t1, t1 + LIVE)
                assert not [i for i in range(len(st)) if i != x and t0 < fin[i] <= t1 and fin[i] > st[i]]
            if path == "exact":  # only batch-lane jobs are running: everything alive lies in X's batch
                assert all(batch_of(i) == batch_of(x) for i in range(len(st)) if st[i] <= t0 < fin[i])
    return arrays, s, oracle


def case_leaving_lane_63():
    built = [last_lane_stream(), misplaced_last_lane_head_stream()]
    per = [b[0] for b in built]
    arrays, s = big_node_clusters(per), streams_of(per)
    oracle = oracle_of(arrays, s)
    assert not oracle[3]["flags"].any() and oracle[3]["waited"].tolist() == [2, 1]
    st, fin = starts_of(oracle, s, 0), finishes_of(oracle, s, 0)
    for k, (h, t0, t1) in built[0][1].items():
        assert h & 63 == 63 and (st[h], fin[h]) == (t0, t1) and fin[h - 1] == t0 and st[h + 1] == t1
        assert sum(live_at_batch_end(st, fin, i) for i in range(h - 63, h)) == 3
    (h, F), = built[1][1]  # (the misplaced slot and the head in lane 63 are due in one second: the ninth row)
    assert h & 63 == 63 and finishes_of(oracle, s, 1)[h] == F == starts_of(oracle, s, 1)[h] + 1
    return arrays, s, oracle


def test_start_is_formed_in_every_path_out_of_live(engine, diag):
    run_and_compare(engine, *case_leaving_paths(), diag)


def test_start_is_formed_for_a_head_placed_in_lane_63(engine, diag):
    run_and_compare(engine, *case_leaving_lane_63(), diag)


# ---- the batch end ---------------------------------------------------------------------------------------------
def case_batch_end():
    """0: a batch whose 64 lanes are all live, placed at 64 different seconds.  1: live lanes, lanes released
    inside the batch (one second each, a release a second) and zero-duration lanes in turn.  2: a batch of 64
    zero-duration jobs: nothing is live, the batch end forms nothing; the batch behind it is all live."""
    per = [
        [(1 + i, LIVE + 5 * i, *TINY) for i in range(64)],
        [(1 + i, (LIVE + i, 1, 0)[i % 3], *TINY) for i in range(64)],
        [(i // 8, 0, *TINY) for i in range(64)] + [(8 + i // 2, LIVE - i, *TINY) for i in range(64)],
    ]
    per = [rows + tiny(70, [50] * 3) + tiny(ROUND, [5] * 70) for rows in per]
    arrays, s = uniform_for(per), streams_of(per)
    oracle = oracle_of(arrays, s)
    assert not oracle[3]["flags"].any() and not oracle[3]["waited"].any()
    st, fin = starts_of(oracle, s, 0), finishes_of(oracle, s, 0)
    assert len(set(st[:64])) == 64 and all(live_at_batch_end(st, fin, i) for i in range(64))
    st, fin = starts_of(oracle, s, 1), finishes_of(oracle, s, 1)
    kinds = [(live_at_batch_end(st, fin, i), leaves_inside(st, fin, i), fin[i] == st[i]) for i in range(64)]
    assert [k.index(True) for k in kinds] == [i % 3 for i in range(63)] + [0] and sum(map(sum, kinds)) == 64
    st, fin = starts_of(oracle, s, 2), finishes_of(oracle, s, 2)
    assert fin[:64] == st[:64] and all(live_at_batch_end(st, fin, i) for i in range(64, 128))
    return arrays, s, oracle


def test_batch_end_forms_the_live_lanes_starts(engine, diag):
    run_and_compare(engine, *case_batch_end(), diag)


# ---- the exit ----------------------------------------------------------------------------------------------------
LENGTHS = (1, 2, 63, 64, 65, 128, 129)


def case_stream_lengths(lengths):
    """Three jobs a second that all outlast the stream: its last batch's lanes are live at the exit."""
    per = [[(i // 3, LIVE + 11 * (i % 7), *TINY) for i in range(J)] for J in lengths]
    arrays, s = uniform_for(per), streams_of(per)
    oracle = oracle_of(arrays, s)
    assert not oracle[3]["flags"].any() and oracle[3]["placed"].tolist() == list(lengths)
    for c, J in enumerate(lengths):
        st, fin = starts_of(oracle, s, c), finishes_of(oracle, s, c)
        assert all(fin[i] > st[J - 1] for i in range(J)) and st == [i // 3 for i in range(J)]
    return arrays, s, oracle


@pytest.mark.parametrize("lengths", [LENGTHS[:4], LENGTHS[4:]], ids=["1_to_64", "65_to_129"])
def test_exit_with_the_last_batch_live(engine, diag, lengths):
    run_and_compare(engine, *case_stream_lengths(lengths), diag)


def case_flagged_exits():
    """A head that needs more than any node has, in lane 1 and in lane 63 of a partly decided batch (the jobs
    before it are placed at different seconds and run on in their lanes; the head steps and jumps from one
    completion to the next, each a release from a batch lane, and the run ends once nothing runs any more), and
    in lane 0 of the batch behind a stored one: the exit finds the cursor at the batch's first lane, the stored
    batch's starts and finishes in the result registers and no lane live."""
    per = [
        [(0, 30, *TINY), (1, 1, *NEVER), (2, 1, *TINY)],
        [(i // 2, 40 + 3 * (i % 9), *TINY) for i in range(63)] + [(31, 2, *NEVER)] + tiny(32, [1] * 5),
        [(i // 2, 40 + 3 * (i % 9), *TINY) for i in range(64)] + [(32, 2, *NEVER)] + tiny(33, [1] * 5),
    ]
    arrays, s = uniform_for(per), streams_of(per)
    oracle = oracle_of(arrays, s)
    stats = oracle[3]
    assert ((stats["flags"] & MCS_FLAG_DEADLOCK) != 0).all()
    assert stats["placed"].tolist() == [1, 63, 64] and stats["waited"].tolist() == [1, 1, 1]
    for c, n in enumerate((1, 63, 64)):
        st, fin = starts_of(oracle, s, c), finishes_of(oracle, s, c)
        assert st[:n] == [i // 2 for i in range(n)] and min(fin[:n]) > per[c][n][0]  # live when the head fails
    return arrays, s, oracle


def test_flagged_exits_keep_the_decided_lanes_starts(engine, diag):
    run_and_compare(engine, *case_flagged_exits(), diag)


def case_pool_of_513():
    per = [[(i // 8, LIVE - i // 8, *TINY) for i in range(POOL + 1)] + ticks(70, 90, 0) + tiny(ROUND, [3] * 70)]
    arrays, s = uniform_for(per), streams_of(per)
    oracle = oracle_of(arrays, s)
    assert oracle[3]["peak_running"].tolist() == [POOL + 1] and not oracle[3]["flags"].any()
    assert len(set(starts_of(oracle, s, 0)[:POOL + 1])) == 65
    return arrays, s, oracle


def test_pool_of_513_escalates_once_with_the_same_starts(diag):
    """513 running, placed at 65 different seconds: the count passes the pool inside the ninth batch, whose
    end hands the cluster to a larger pool; the re-run gives the same starts (an engine of its own: the
    larger pool stays with the engine)."""
    arrays, s, oracle = case_pool_of_513()
    with Engine(0) as eng:
        cs = run_and_compare(eng, arrays, s, oracle, diag, escalations=1)
    assert (cs["peak_running"] > POOL).all()


# ---- extreme values --------------------------------------------------------------------------------------------
TOP = 0xFFFFFFFD  # the largest finish of a one-job stream: the host admits last arrival + sum(dur + 1) <= 2^32 - 2


def case_extreme_values():
    """Start + duration = TOP with a start of 0, of 2^31 and of TOP - 1: finish - duration must not wrap, and
    the jobs are live at the exit.  Cluster 3: start 0 with duration 1, which leaves its lane when the long
    job behind it arrives; that one stays."""
    per = [[(0, TOP, *TINY)], [(1 << 31, TOP - (1 << 31), *TINY)], [(TOP - 1, 1, *TINY)],
           [(0, 1, *TINY), (5, TOP - 5 - 2, *TINY)]]
    arrays, s = uniform_for(per), streams_of(per)
    for c, rows in enumerate(per):
        assert rows[-1][0] + sum(r[1] + 1 for r in rows) <= 0xFFFFFFFE
    oracle = oracle_of(arrays, s)
    assert not oracle[3]["flags"].any()
    assert [(starts_of(oracle, s, c)[-1], finishes_of(oracle, s, c)[-1]) for c in range(4)] == \
        [(0, TOP), (1 << 31, TOP), (TOP - 1, TOP), (5, TOP - 2)]
    assert (starts_of(oracle, s, 3)[0], finishes_of(oracle, s, 3)[0]) == (0, 1)
    return arrays, s, oracle


def test_extreme_starts_and_durations(engine, diag):
    run_and_compare(engine, *case_extreme_values(), diag)


# ---- the node and the finish are written in the job's own lane -------------------------------------------------
def whole_nodes(t, n):
    """n requests for a whole node, one a second from t: each fits only a node that has got back all of it."""
    return [(t + i, 300, 32, 24000) for i in range(n)]


def case_fit_lane_and_batch_lane():
    """Only a few nodes have cores, and a job of 32 cores takes the lowest of them: node 20 (fit lane 5) from
    batch lane 5 and node 28 (fit lane 7) from lane 6: the same lane, and one apart; node 252 (fit lane 63)
    from batch lane 0 and node 3 (fit lane 0) from lane 63: 63 apart either way.  Each job asks for another
    amount of memory and finishes inside its batch or after it, and from second 40 on whole-node requests
    arrive, which fit a node only once it has got back exactly what its job took: a node word or a request
    written into a neighbouring lane shows in where and when those run."""
    frees = ([20, 28], [252], [3])
    per = [
        pad([], 5, 0) + [(0, 9, 32, 700), (0, 70, 32, 900), (10, 1, *TINY)] + whole_nodes(40, 2),
        [(0, 70, 32, 1100), (1, 1, *TINY)] + whole_nodes(40, 1),
        pad([], 63, 0) + [(0, 20, 32, 1300), (1, 1, *TINY)] + whole_nodes(40, 1),
    ]
    arrays, s = pack_clusters([only_free(256, f) for f in frees]), streams_of(per)
    oracle = oracle_of(arrays, s)
    assert not oracle[3]["flags"].any() and oracle[3]["placed"].tolist() == [len(r) for r in per]
    for c, (free, first) in enumerate(zip(frees, (5, 0, 63))):
        nd, st, fin = nodes_of(oracle, s, c), starts_of(oracle, s, c), finishes_of(oracle, s, c)
        n = len(free)
        assert nd[first:first + n] == free and sorted(nd[-n:]) == free
        assert all(st[len(nd) - n + i] >= fin[first + free.index(x)] for i, x in enumerate(nd[-n:]))
    return arrays, s, oracle


def test_fit_lane_and_batch_lane(engine, diag):
    run_and_compare(engine, *case_fit_lane_and_batch_lane(), diag)


def case_record_after_a_placement():
    """0: a zero-duration job is the next record after a placement of the pass (three in a row, the last one
    the batch's last job).  1: ... after a placed WaitQueue head.  2: a zero-duration WaitQueue head, and a
    normal job behind it.  3: the first job of a batch is placed as a WaitQueue head (it waits for the BIG job
    in lane 63 of the batch before, which the batch end has moved into its calendar row)."""
    per = [
        pad([], 60, 0) + [(0, 5, *TINY), (0, 0, *TINY), (0, 0, *TINY), (0, 0, *TINY), (0, 3, *TINY), (1, 4, *TINY)],
        [(0, 12, *BIG), (4, 5, *BIG), (4, 0, *TINY), (4, 2, *TINY)],
        [(0, 9, *BIG), (2, 0, *BIG), (2, 1, *TINY), (2, 6, *TINY)],
        pad([], 63, 0) + [(0, 7, *BIG), (0, 5, *BIG), (0, 2, *TINY)],
    ]
    per = [rows + tiny(ROUND, [5] * 70) for rows in per]
    arrays, s = big_node_clusters(per), streams_of(per)
    oracle = oracle_of(arrays, s)
    stats = oracle[3]
    assert not stats["flags"].any() and stats["waited"].tolist() == [0, 1, 1, 1]
    assert starts_of(oracle, s, 0)[60:66] == [0, 0, 0, 0, 0, 1]
    assert starts_of(oracle, s, 1)[:4] == [0, 12, 13, 13]
    assert starts_of(oracle, s, 2)[:4] == [0, 9, 10, 10]
    assert starts_of(oracle, s, 3)[63:66] == [0, 7, 8]
    return arrays, s, oracle


def test_record_after_a_placement(engine, diag):
    run_and_compare(engine, *case_record_after_a_placement(), diag)


# ---- a calendar row is one register quad -----------------------------------------------------------------------
def case_bulk_move_free_lanes():
    """Row 0 holds 0, 54, 63 and 64 slots that run on when a batch brings 64 jobs for it: the row has 64, 10, 1
    and no free lane, the rest is surplus and goes to the next rows.  The clock then visits the seconds at
    which the moved jobs are due one by one."""
    per = [pad(tiny(0, [FAR] * k), 0, 0) + tiny(0, [16 + 8 * (i % 6) for i in range(64)]) + ticks(1, 70, 0)
           for k in (0, 54, 63, 64)]
    per = [rows + tiny(ROUND, [5] * 70) for rows in per]
    arrays, s = uniform_for(per), streams_of(per)
    oracle = oracle_of(arrays, s)
    assert not oracle[3]["flags"].any() and not oracle[3]["waited"].any()
    for c, k in enumerate((0, 54, 63, 64)):
        assert running_at(oracle, *span(s, c), 0) == (k + 64, k + 64)
    return arrays, s, oracle


def test_bulk_move_into_rows_with_free_lanes(engine, diag):
    run_and_compare(engine, *case_bulk_move_free_lanes(), diag)


def case_one_instant_all_rows():
    """64 placements at one instant into lanes 0 ... 63, each with another duration: the batch brings eight jobs
    for each of the eight rows (cluster 0: the clock then visits their seconds one by one), or runs on for
    hundreds of seconds (cluster 1)."""
    per = [tiny(0, [40 + i for i in range(64)]) + ticks(1, 110, 0),
           tiny(0, [LIVE - 13 * i for i in range(64)]) + tiny(1, [7] * 3)]
    per = [rows + tiny(ROUND, [5] * 70) for rows in per]
    arrays, s = uniform_for(per), streams_of(per)
    oracle = oracle_of(arrays, s)
    assert not oracle[3]["flags"].any() and not oracle[3]["waited"].any()
    for c in range(2):
        assert starts_of(oracle, s, c)[:64] == [0] * 64 and len(set(finishes_of(oracle, s, c)[:64])) == 64
    assert np.bincount(np.array(finishes_of(oracle, s, 0)[:64]) & 7, minlength=8).tolist() == [8] * 8
    return arrays, s, oracle


def test_one_instant_into_every_lane_and_row(engine, diag):
    run_and_compare(engine, *case_one_instant_all_rows(), diag)


def case_lane_without_an_entry_keeps_its_slot():
    """64 nodes have cores and a batch of 64 jobs takes one each (17 ... 32 cores, 64 different amounts of
    memory), all due in calendar row 0: 53 of them at 800 and 11, scattered over the row's lanes, at 8.  Those
    are released, and the next batch brings 11 jobs for the freed nodes, due in row 0 again at 24 ... 104:
    the bulk move's read lands in the row's free lanes only, under the eyes of the 53 slots that stay.  Every
    job is then released at its second, and from 900 on whole-node requests arrive, which fit a node only
    once it has got back exactly what its job took."""
    free = [3 * i + 1 for i in range(LANES)]
    short = [i for i in range(LANES) if i % 6 == 0]
    first = [(0, 8 if i in short else FAR, 17 + i % 16, 1000 + 37 * i) for i in range(LANES)]
    second = [(8, 16 + 8 * k, 18 + k, 5000 + 41 * k) for k in range(len(short))]
    rows = first + second + ticks(9, 110, 0)
    rows = pad(rows, 0, 110) + whole_nodes(900, LANES)
    arrays, s = pack_clusters([only_free(200, free)] * 2), streams_of([rows, rows])
    oracle = oracle_of(arrays, s)
    assert not oracle[3]["flags"].any() and oracle[3]["placed"].tolist() == [len(rows)] * 2
    nd, st, fin = nodes_of(oracle, s, 0), starts_of(oracle, s, 0), finishes_of(oracle, s, 0)
    assert nd[:LANES] == free and nd[LANES:LANES + len(short)] == [free[i] for i in short]
    assert st[LANES:LANES + len(short)] == [8] * len(short) and all(f & 7 == 0 for f in fin[:LANES + len(short)])
    assert running_at(oracle, *span(s, 0), 8) == (LANES, LANES) and sorted(nd[-LANES:]) == free
    return arrays, s, oracle


def test_lane_without_an_entry_keeps_its_slot(engine, diag):
    run_and_compare(engine, *case_lane_without_an_entry_keeps_its_slot(), diag)


def case_surplus_rows():
    """The surplus of row r goes to row r + 1 and to row r + 7 (mod 8), for r = 0 and r = 7: the rows from r on
    are full (64 slots each, due at 800 + row) but the one the surplus ends in, and a batch brings 20 jobs
    for row r, which the clock then visits one by one."""
    per = []
    for r, k in ((0, 1), (0, 7), (7, 1), (7, 7)):
        rows = []
        for j in range(k):
            rows += tiny(0, [FAR + (r + j) % 8] * LANES)
        rows += tiny(0, [16 + r + 8 * (i % 5) for i in range(20)]) + ticks(1, 70, 0)
        per.append(rows + tiny(ROUND, [5] * 60))
    arrays, s = uniform_for(per), streams_of(per)
    oracle = oracle_of(arrays, s)
    assert not oracle[3]["flags"].any() and not oracle[3]["waited"].any()
    for c, (r, k) in enumerate(((0, 1), (0, 7), (7, 1), (7, 7))):
        fin = np.array(finishes_of(oracle, s, c)[:LANES * k + 20])
        want = [0] * 8
        for j in range(k):
            want[(r + j) % 8] = LANES
        want[r] += 20
        assert np.bincount(fin & 7, minlength=8).tolist() == want and running_at(oracle, *span(s, c), 0)[0] == len(fin)
    return arrays, s, oracle


def test_surplus_goes_to_the_next_free_row(engine, diag):
    run_and_compare(engine, *case_surplus_rows(), diag)


# ---- fuzz --------------------------------------------------------------------------------------------------------
def case_fuzz_crowded(seed):
    arrays, s = crowded(seed)
    oracle = oracle_of(arrays, s)
    assert not oracle[3]["flags"].any() and 5 * int(oracle[3]["waited"].sum()) >= int(s.job_off[-1])  # (a fifth wait)
    return arrays, s, oracle


@pytest.mark.parametrize("seed", [91, 95])
def test_fuzz_crowded_streams(engine, diag, seed):
    run_and_compare(engine, *case_fuzz_crowded(seed), diag)


def case_fuzz_short_durations():
    """Durations of at most 8 s: most jobs leave their lane before their batch ends."""
    arrays, s = fuzz_workload("w16r", 93, n_clusters=4, J=400, blocking=False)
    s = JobStreams(s.arrival, s.dur % 9, s.cores, s.mem, s.job_off)
    oracle = oracle_of(arrays, s)
    inside = 0
    for c in range(4):
        st, fin = starts_of(oracle, s, c), finishes_of(oracle, s, c)
        inside += sum(leaves_inside(st, fin, i) for i in range(len(st)))
    assert not oracle[3]["flags"].any() and 2 * inside > int(s.job_off[-1])
    return arrays, s, oracle


def test_fuzz_short_durations(engine, diag):
    run_and_compare(engine, *case_fuzz_short_durations(), diag)
