"""The streamed W16R loop's pass end and clock advances ("One loop test per pass"): the
record read after a placement yields the arrival 0xffffffff when the batch has no next job, when the next
job has zero duration, and when the job just placed was a WaitQueue head (a failed fit marks the next
job's arrival), so the pass closes on the arrival test alone and an out-of-line route tells the cases
apart; the row compare of a clock advance branches on vcc.  None of this shows in a placement unless it
goes wrong, so every case is a bit-exact parity run against the oracle (node, start, finish, t_end,
placed, waited, peak_running, flags) on a stream built to drive one of those places, on the production
and the counting build, with the kernel asserted and the counting build's iterations and release_scans
checked against a replay of the clock (the helpers of test_gpu_calendar_rows.py).  What a case relies on
is asserted from the oracle's results on the CPU before the GPU runs.  The cases pin behaviour that does
not change: they pass on the loop as it was before as well.  Run on a real MI355X: ``pytest -m gpu``.

Clusters as in test_gpu_calendar_rows.py: on one_big_node(n) a BIG job runs on node 0 alone, one at a
time, beside any number of TINY ones (node 0 as well) and MID ones (the other nodes)."""
import numpy as np
import pytest

import oracle_ref as O
from kat_util import fuzz_workload
from mcs_amd import MCS_FLAG_DEADLOCK, pack_clusters, uniform_cluster
from test_gpu_calendar_rows import (BIG, MID, NEVER, TINY, big_node_clusters, diag, residue_workload,  # noqa: F401
                                    run_and_compare, streams_of, ticks, tiny, uniform_for)

pytestmark = pytest.mark.gpu


def starts_of(oracle, s, c):
    j0, j1 = int(s.job_off[c]), int(s.job_off[c + 1])
    return oracle[1][j0:j1].tolist()


# ---- stream lengths: a last batch of 1 and of 63 jobs ------------------------------------------------
LENGTHS = (1, 63, 64, 65, 127, 128, 129)


def length_stream(J):
    """Two jobs a second with durations 1 ... 13; the stream's last job is placed a while after the rest."""
    rows = [(i // 2, (i % 5) * 3 + 1, *TINY) for i in range(J - 1)]
    return rows + [(J // 2 + 3, 2, *TINY)]


def test_stream_lengths(engine, diag):
    for group in (LENGTHS[:4], LENGTHS[4:]):
        per = [length_stream(J) for J in group]
        arrays, s = uniform_for(per), streams_of(per)
        oracle = O.fifo_run_batch(arrays, s, n_threads=4)
        assert not oracle[3]["flags"].any() and oracle[3]["placed"].tolist() == list(group)  # (on the CPU, first)
        run_and_compare(engine, arrays, s, oracle, diag)


# ---- lane 63 and the lane after it --------------------------------------------------------------------
def lane63_stream(mode, nxt):
    """Job 63 placed normally (at 21), as a WaitQueue head (fails at 20, placed at 26) or with zero
    duration (at 21); job 64, lane 0 of the next batch, arrives 5 s after that placement, or has arrived,
    with zero duration or not.  Returns the rows and the two start seconds."""
    rows = [(i // 3, 1 + (i % 5) * 3, *TINY) for i in range(62)]
    if mode == "head":
        rows += [(20, 6, *BIG), (20, 3, *BIG)]
        a63, p63, follow = 20, 26, 27  # (a placed head sleeps a second)
    else:
        rows += [(20, 4, *TINY), (21, 0 if mode == "zero" else 4, *TINY)]
        a63, p63, follow = 21, 21, 21
    if nxt == "later":
        rows.append((p63 + 5, 2, *TINY))
        follow = p63 + 5
    else:
        rows.append((a63, 0 if nxt == "zero" else 2, *TINY))
    assert len(rows) == 65
    return rows + ticks(follow + 1, follow + 6) + tiny(follow + 50, [5] * 80), p63, follow


@pytest.mark.parametrize("mode", ["normal", "head", "zero"])
def test_lane_63(engine, diag, mode):
    built = [lane63_stream(mode, nxt) for nxt in ("later", "arrived", "zero")]
    per = [b[0] for b in built]
    arrays, s = big_node_clusters(per), streams_of(per)
    oracle = O.fifo_run_batch(arrays, s, n_threads=4)
    stats = oracle[3]  # (on the CPU, first)
    assert not stats["flags"].any() and stats["waited"].tolist() == [int(mode == "head")] * 3
    for c, (_, p63, follow) in enumerate(built):
        assert starts_of(oracle, s, c)[63:65] == [p63, follow]
    run_and_compare(engine, arrays, s, oracle, diag)


# ---- the placed WaitQueue head ---------------------------------------------------------------------------
def head_stream(fails, nxt):
    """A head that fails once (at its arrival, 4; placed at 12) or at its arrival and three completions
    (4, 16, 37; placed at 47), and the job after it: arrived with the head, arriving 4 s after the head's
    placement (later than its one-second sleep), of zero duration, in the next batch (the head is job 63),
    or none (the head is the stream's last job).  Returns the rows, the head's index and the two starts."""
    if fails == 1:
        rows, head, placed = [(0, 12, *BIG)], (4, 5, *BIG), 12
    else:
        rows, head, placed = [(0, 47, *BIG), (0, 4, *MID), (0, 16, *MID), (0, 37, *MID)], (0, 5, *BIG), 47
    if nxt == "nextbatch":
        rows = tiny(0, [200] * (63 - len(rows))) + rows
    k = len(rows)
    rows.append(head)
    if nxt == "absent":
        return rows, k, placed, None
    if nxt == "later":
        rows.append((placed + 4, 1, *TINY))
        follow = placed + 4
    else:
        rows.append((head[0], 0 if nxt == "zero" else 2, *TINY))
        follow = placed + 1
    return rows + tiny(placed + 300, [5] * 70), k, placed, follow


def check_heads(oracle, s, built):
    stats = oracle[3]
    assert not stats["flags"].any() and stats["waited"].tolist()[:len(built)] == [1] * len(built)
    for c, (_, k, placed, follow) in enumerate(built):
        st = starts_of(oracle, s, c)
        assert st[k] == placed and (follow is None or st[k + 1] == follow)


@pytest.mark.parametrize("fails", [1, 4], ids=["once", "three_completions"])
def test_placed_head_and_the_job_after_it(engine, diag, fails):
    built = [head_stream(fails, nxt) for nxt in ("arrived", "later", "zero", "nextbatch")]
    assert built[3][1] == 63
    per = [b[0] for b in built]
    arrays, s = big_node_clusters(per), streams_of(per)
    oracle = O.fifo_run_batch(arrays, s, n_threads=4)
    check_heads(oracle, s, built)  # (on the CPU, first)
    run_and_compare(engine, arrays, s, oracle, diag)


def test_head_is_the_last_job_and_two_heads_in_a_row(engine, diag):
    """The head as the stream's last job (nothing to restore); two heads one after the other: the first
    fails at 2, is placed at 10 and sleeps to 11, where the second fails; it is placed at 15, and the job
    behind it at 16."""
    two = [(0, 10, *BIG), (2, 5, *BIG), (2, 5, *BIG), (2, 1, *TINY)] + tiny(400, [5] * 9)
    built = [head_stream(1, "absent"), head_stream(4, "absent")]
    per = [built[0][0], built[1][0], two]
    arrays, s = big_node_clusters(per), streams_of(per)
    oracle = O.fifo_run_batch(arrays, s, n_threads=4)
    check_heads(oracle, s, built)  # (on the CPU, first)
    assert oracle[3]["waited"].tolist() == [1, 1, 2] and starts_of(oracle, s, 2)[:4] == [0, 10, 15, 16]
    run_and_compare(engine, arrays, s, oracle, diag)


def test_deadlock_with_the_mark_set_and_the_guard_bound(engine, diag):
    """Deadlocks behind a failed fit (the next job's arrival is marked, and stays so): at the stream's
    only job (J = 1, the guard's bound 4J + 256 = 260), after earlier jobs ran, and at lane 63.  A head
    that fails at its arrival and at every one of 63 completions in a stream of 65 jobs stays far below
    the bound 516 and is placed."""
    many = [(0, 200, *BIG)] + [(0, 3 * (i + 1), *MID) for i in range(63)] + [(0, 2, *BIG)]
    per = [
        [(3, 2, *NEVER)],
        [(0, 10, *BIG), (0, 3, *TINY), (5, 1, *NEVER), (6, 1, *TINY)],
        tiny(0, [4] * 63) + [(2, 1, *NEVER), (2, 1, *TINY), (3, 0, *TINY)],
        many,
    ]
    arrays, s = big_node_clusters(per), streams_of(per)
    oracle = O.fifo_run_batch(arrays, s, n_threads=4)
    stats = oracle[3]  # (on the CPU, first)
    assert ((stats["flags"] & MCS_FLAG_DEADLOCK) != 0).tolist() == [True, True, True, False]
    assert stats["placed"].tolist() == [0, 2, 63, 65] and stats["waited"].tolist() == [1, 1, 1, 1]
    assert starts_of(oracle, s, 3)[64] == 200
    run_and_compare(engine, arrays, s, oracle, diag)


# ---- every residue of the clock, reached in every way ------------------------------------------------------
KINDS = ("headsleep", "step", "arrive1", "gap", "exactmin", "bend", "misplaced")


def residue_round(kind, T, r, rel, n0):
    """One way for the clock to reach S = T + 16 + r (T a multiple of 8 with nothing running: S & 7 = r),
    and what comes next: a second with a completion (rel) or without one.  n0 is the stream's length
    before the round.  Returns the rows and {index in the round: expected start}."""
    S = T + 16 + r
    if kind == "headsleep":  # the head is placed at S - 1 and sleeps to S
        rows = [(T, S - 1 - T, *BIG)] + ([(T, S - T, *TINY)] if rel else [])
        k = len(rows)
        return rows + [(T + 1, 2, *BIG), (T + 1, 3, *TINY)], {k: S - 1, k + 1: S}
    if kind == "step":  # the head fails at S - 3: steps to S - 2, S - 1 (empty), S (a release, the retry
        # fails), S + 1 (a release or none), S + 2 (the blocker's: placed)
        rows = [(T, S + 2 - T, *BIG), (T, S - T, *TINY)] + ([(T, S + 1 - T, *TINY)] if rel else [])
        k = len(rows)
        return rows + [(S - 3, 2, *BIG), (S - 3, 1, *TINY)], {k: S + 2, k + 1: S + 3}
    if kind == "arrive1":  # an arrival one second on
        rows = [(T, S - T, *TINY)] if rel else []
        k = len(rows)
        return rows + [(S - 1, 9, *TINY), (S, 1, *TINY)], {k: S - 1, k + 1: S}
    if kind == "gap":  # an arrival 6 s on (the full scan), then one a second on
        rows = [(T, S - T, *TINY), (T, S + 1 - T, *TINY)] if rel else []
        k = len(rows)
        return rows + [(S - 6, 20, *TINY), (S, 2, *TINY), (S + 1, 2, *TINY)], {k + 1: S, k + 2: S + 1}
    if kind == "exactmin":  # the head fails at S - 12: eight empty steps, then the jump to the blocker's S
        rows = [(T, S - T, *BIG)] + ([(T, S + 1 - T, *TINY)] if rel else [])
        k = len(rows)
        return rows + [(S - 12, 2, *BIG), (S - 12, 1, *TINY)], {k: S, k + 1: S + 1}
    if kind == "bend":  # lane 63 is placed at S, lane 0 of the next batch a second on
        rows = [(T, S + 1 - T, *TINY)] if rel else []
        rows += tiny(T, [0] * ((63 - n0 - len(rows)) % 64))
        k = len(rows)
        assert (n0 + k) % 64 == 63
        return rows + [(S, 5, *TINY), (S + 1, 1, *TINY)], {k: S, k + 1: S + 1}
    # a misplaced slot due at S: its row (64 slots that finish 800 s later, S & 7 as well) was full
    rows = tiny(T, [816 + r] * 64 + [S - T] * 3) + ticks(T + 1, S + 3 + int(rel), 1 if rel else 2)
    return rows, {67 + S - T - 1: S}


def residue_stream(r, rel):
    rows, expect, T = [], {}, 1024
    for kind in KINDS:
        part, exp = residue_round(kind, T, r, rel, len(rows))
        expect.update({len(rows) + k: v for k, v in exp.items()})
        rows += part
        T += 1024
    return rows + tiny(T, [5] * 90), expect


@pytest.mark.parametrize("r", range(8))
def test_clock_residue(engine, diag, r):
    built = [residue_stream(r, rel) for rel in (True, False)]
    per = [b[0] for b in built]
    for rows in per:
        assert all(a[0] <= b[0] for a, b in zip(rows, rows[1:]))
    arrays, s = big_node_clusters(per), streams_of(per)
    oracle = O.fifo_run_batch(arrays, s, n_threads=4)
    stats = oracle[3]  # (on the CPU, first)
    assert not stats["flags"].any() and stats["waited"].tolist() == [3, 3]
    for c, (_, expect) in enumerate(built):
        st = starts_of(oracle, s, c)
        assert {k: st[k] for k in expect} == expect
    run_and_compare(engine, arrays, s, oracle, diag)


# ---- releases hand their payloads back to the right nodes -------------------------------------------------
def test_release_returns_payloads_to_edge_nodes(engine, diag):
    """Every node full (a 32-core job each, first fit: job i on node i); the jobs on nodes 0, 3, 252, 255
    (and on node 128, the last real node of a 129-node cluster) finish early, and the next 32-core jobs
    fit those nodes only."""
    per, targets = [], ([0, 3, 252, 255], [0, 3, 128])
    for n, tg in zip((256, 129), targets):
        rows = [(0, 5 + tg.index(i) if i in tg else 500, 32, 1) for i in range(n)]
        per.append(rows + [(20, 3, 32, 1)] * len(tg) + tiny(40, [5] * 10))
    arrays, s = pack_clusters([uniform_cluster(256), uniform_cluster(129)]), streams_of(per)
    oracle = O.fifo_run_batch(arrays, s, n_threads=4)
    stats = oracle[3]  # (on the CPU, first)
    assert not stats["flags"].any() and not stats["waited"].any()
    for c, (n, tg) in enumerate(zip((256, 129), targets)):
        j0 = int(s.job_off[c])
        assert oracle[0][j0:j0 + n].tolist() == list(range(n))
        assert oracle[0][j0 + n:j0 + n + len(tg)].tolist() == tg
    run_and_compare(engine, arrays, s, oracle, diag)


# ---- fuzz ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [61, 62])
def test_fuzz_streams(engine, diag, seed):
    arrays, s = fuzz_workload("w16r", seed, n_clusters=4, J=400)
    oracle = O.fifo_run_batch(arrays, s, n_threads=4)
    assert oracle[3]["waited"].any()  # (failed fits happen)
    run_and_compare(engine, arrays, s, oracle, diag)


def test_fuzz_one_residue_bursts(engine, diag):
    per = residue_workload(53)
    arrays, s = uniform_for(per), streams_of(per)
    oracle = O.fifo_run_batch(arrays, s, n_threads=4)
    stats = oracle[3]  # (on the CPU, first)
    assert not stats["flags"].any() and stats["waited"].all()
    run_and_compare(engine, arrays, s, oracle, diag)
