"""The streamed W16R loop while a WaitQueue head waits ("The waiting head"): the failed
fit, the sleep to the next completion (second by second up to a limit, then the jump to the exact
earliest finish), the release that lets the head in or fails it again, the head's placement with the
record of the job behind it, and the one-second sleep after it; for a zero-duration head the same out
of line.  None of this shows in a placement unless it goes wrong, so every case is a bit-exact parity run
against the oracle (node, start, finish, t_end, placed, waited, peak_running, flags) on a stream built to
drive one of those places, on the production and the counting build, with the kernel asserted and the
counting build's iterations and release_scans checked against a replay of the clock (the helpers of
test_gpu_calendar_rows.py).  What a case relies on (the head really waited, the sleep really had that
length) is asserted from the oracle's results on the CPU before the GPU runs.  The cases pin behaviour
that does not change: they pass on the loop as it was before as well.  Run on a real MI355X:
``pytest -m gpu``.

Clusters as in test_gpu_calendar_rows.py: on one_big_node(n) a BIG job runs on node 0 alone, one at a
time, beside any number of TINY and MID ones, so a BIG head waits exactly for the BIG job before it.

A head can only wait for a job placed before it, so a stream of one job has no placed head: J = 1 is the
deadlock case, and the shortest stream whose last job is a placed head has two jobs."""
import numpy as np
import pytest

import oracle_ref as O
from kat_util import fuzz_workload
from mcs_amd import MCS_FLAG_DEADLOCK, Engine, JobStreams, pack_clusters, uniform_cluster
from test_gpu_calendar_rows import (BIG, FAR, LANES, MID, NEVER, POOL, TINY, big_node_clusters, diag,  # noqa: F401
                                    residue_workload, run_and_compare, running_at, streams_of, ticks, tiny)

pytestmark = pytest.mark.gpu


def span(s, c):
    return int(s.job_off[c]), int(s.job_off[c + 1])


def starts_of(oracle, s, c):
    j0, j1 = span(s, c)
    return oracle[1][j0:j1].tolist()


def completions_in(oracle, s, c, t0, t1):
    """The finish seconds of cluster c's jobs that lie in (t0, t1), jobs of zero duration left out."""
    j0, j1 = span(s, c)
    st, fin = oracle[1][j0:j1], oracle[2][j0:j1]
    return sorted(set(fin[(fin > st) & (fin > t0) & (fin < t1)].tolist()))


def oracle_of(arrays, s):
    return O.fifo_run_batch(arrays, s, n_threads=4)


# ---- every residue of the clock at the failed fit, every length of the sleep ---------------------------
AHEAD = (1, 2, 7, 8, 9, 10, 600)


def sleep_stream(r, order, background):
    """One round per sleep length k: the BIG job before the head finishes at T + k, the head arrives and
    fails at T (T & 7 = r), is placed at T + k and sleeps a second, and the TINY job behind it starts at
    T + k + 1.  Nothing else finishes inside a round (the background jobs run past the stream's end)."""
    rows, expect, base = (tiny(0, [1_000_000 + i for i in range(16)]) if background else []), {}, 2048
    for k in order:
        T = base + r
        expect[len(rows) + 1] = (T, T + k)
        rows += [(T - 3, 3 + k, *BIG), (T, 5, *BIG), (T, 1, *TINY)]
        base += 2048
    return rows + tiny(base, [5] * 40), expect


@pytest.mark.parametrize("r", range(8))
def test_sleep_lengths_at_every_residue(engine, diag, r):
    built = [sleep_stream(r, AHEAD, False), sleep_stream(r, AHEAD[::-1], True)]
    per = [b[0] for b in built]
    arrays, s = big_node_clusters(per), streams_of(per)
    oracle = oracle_of(arrays, s)
    stats = oracle[3]  # (on the CPU, first)
    assert not stats["flags"].any() and stats["waited"].tolist() == [len(AHEAD)] * 2
    for c, (_, expect) in enumerate(built):
        st = starts_of(oracle, s, c)
        for head, (T, placed) in expect.items():
            assert T & 7 == r and st[head - 1] == T - 3 and st[head:head + 2] == [placed, placed + 1]
            assert completions_in(oracle, s, c, T, placed) == []  # the sleep has that length
    run_and_compare(engine, arrays, s, oracle, diag)


# ---- a head that fails again -------------------------------------------------------------------------
def refail_stream(others, big):
    """The head fails at 4 and at each completion in others (MID jobs: no room for it), and is placed
    when the BIG job finishes."""
    return [(0, big, *BIG)] + [(0, d, *MID) for d in others] + [(4, 5, *BIG), (4, 2, *TINY)] \
        + tiny(big + 300, [5] * 70)


def test_head_fails_again_and_two_heads_in_a_row(engine, diag):
    """A head that fails again after one release (a step away) and after three (a step, the eighth step
    and the exact jump away); two heads one after the other: the first fails at 2, is placed at 10 and
    sleeps to 11, where the second fails; it is placed at 15, and the job behind it at 16."""
    two = [(0, 10, *BIG), (2, 5, *BIG), (2, 5, *BIG), (2, 1, *TINY)] + tiny(400, [5] * 9)
    per = [refail_stream([6], 12), refail_stream([6, 14, 37], 47), two]
    arrays, s = big_node_clusters(per), streams_of(per)
    oracle = oracle_of(arrays, s)
    stats = oracle[3]  # (on the CPU, first)
    assert not stats["flags"].any() and stats["waited"].tolist() == [1, 1, 2]
    assert starts_of(oracle, s, 0)[2:4] == [12, 13] and completions_in(oracle, s, 0, 4, 12) == [6]
    assert starts_of(oracle, s, 1)[4:6] == [47, 48] and completions_in(oracle, s, 1, 4, 47) == [6, 14, 37]
    assert starts_of(oracle, s, 2)[:4] == [0, 10, 15, 16]
    run_and_compare(engine, arrays, s, oracle, diag)


# ---- the job behind a placed head -----------------------------------------------------------------------
SUCCESSORS = ("arrived", "one_second", "later", "zero", "nextbatch")


def successor_stream(nxt):
    """The head fails at 4 and is placed at 12; the job behind it has arrived with it, arrives when the
    head's one-second sleep ends, arrives later than that, has zero duration, or lies in the next batch
    (the head is job 63).  Returns the rows, the head's index and the start of the job behind it."""
    rows = (tiny(0, [200] * 62) if nxt == "nextbatch" else []) + [(0, 12, *BIG), (4, 5, *BIG)]
    head = len(rows) - 1
    behind = {"one_second": (13, 2, *TINY), "later": (16, 1, *TINY), "zero": (4, 0, *TINY)}.get(nxt, (4, 2, *TINY))
    return rows + [behind] + tiny(400, [5] * 70), head, max(13, behind[0])


def last_job_stream(J):
    """The head is the stream's last job (J >= 2: see the module's note)."""
    return tiny(0, [200] * (J - 2)) + [(0, 12, *BIG), (4, 5, *BIG)]


def test_job_behind_a_placed_head(engine, diag):
    built = [successor_stream(nxt) for nxt in SUCCESSORS]
    assert built[4][1] == 63
    for per, heads in (([b[0] for b in built[:4]], built[:4]), ([built[4][0]], built[4:])):
        arrays, s = big_node_clusters(per), streams_of(per)
        oracle = oracle_of(arrays, s)
        stats = oracle[3]  # (on the CPU, first)
        assert not stats["flags"].any() and stats["waited"].tolist() == [1] * len(per)
        for c, (_, head, follow) in enumerate(heads):
            assert starts_of(oracle, s, c)[head:head + 2] == [12, follow]
        run_and_compare(engine, arrays, s, oracle, diag)


def test_placed_head_is_the_last_job(engine, diag):
    per = [last_job_stream(J) for J in (2, 64, 65)]
    arrays, s = big_node_clusters(per), streams_of(per)
    oracle = oracle_of(arrays, s)
    stats = oracle[3]  # (on the CPU, first)
    assert not stats["flags"].any() and stats["waited"].tolist() == [1, 1, 1]
    assert stats["placed"].tolist() == [2, 64, 65] and [starts_of(oracle, s, c)[-1] for c in range(3)] == [12] * 3
    run_and_compare(engine, arrays, s, oracle, diag)


# ---- a zero-duration head that waits ----------------------------------------------------------------------
def zero_head_stream(head, others, big):
    """Job number head (63: lane 63; 64: lane 0 of the next batch) is a BIG request of zero duration that
    arrives at 2 and waits for the BIG job, failing again at every completion in others on the way."""
    rows = [(0, big, *BIG)] + [(0, d, *MID) for d in others]
    rows += tiny(0, [1] * (head - len(rows))) + [(2, 0, *BIG), (2, 1, *TINY)]
    return rows + tiny(big + 300, [5] * 70)


@pytest.mark.parametrize("head", [64, 63], ids=["lane0", "lane63"])
def test_zero_duration_head_waits(engine, diag, head):
    """Let in by the first completion (7 s on) and by the third (3 s, then 8 s, then 17 s on)."""
    per = [zero_head_stream(head, [], 9), zero_head_stream(head, [5, 13], 30)]
    arrays, s = big_node_clusters(per), streams_of(per)
    oracle = oracle_of(arrays, s)
    stats = oracle[3]  # (on the CPU, first)
    assert not stats["flags"].any() and stats["waited"].tolist() == [1, 1]
    for c, (big, others) in enumerate(((9, []), (30, [5, 13]))):
        st, fin = starts_of(oracle, s, c), oracle[2][span(s, c)[0] + head]
        assert st[head:head + 2] == [big, big + 1] and fin == big
        assert completions_in(oracle, s, c, 2, big) == others
    run_and_compare(engine, arrays, s, oracle, diag)


# ---- a misplaced slot falls due in the sleep ---------------------------------------------------------------
def misplaced_stream(t0, regular):
    """65 TINY jobs at 0 whose finishes share calendar row 3: the last one, due at 35, finds the row
    full (regular: the row's last regular slot is due at 35 as well).  The head fails at t0 behind a BIG
    job that runs until 60, so the misplaced slot's second is a step of its sleep: the first (t0 = 34) or
    the eighth (t0 = 27); the retry fails, and the sleep goes on to 60."""
    rows = tiny(0, [FAR + 3] * (63 if regular else 64) + ([35] if regular else []) + [35]) + [(0, 60, *BIG)]
    return rows + ticks(1, t0) + [(t0, 4, *BIG), (t0, 2, *TINY)] + tiny(300, [5] * 90)


def test_misplaced_slot_due_in_the_sleep(engine, diag):
    cases = [(34, False), (27, False), (34, True)]
    per = [misplaced_stream(*c) for c in cases]
    arrays, s = big_node_clusters(per), streams_of(per)
    oracle = oracle_of(arrays, s)
    stats = oracle[3]  # (on the CPU, first)
    assert not stats["flags"].any() and stats["waited"].tolist() == [1, 1, 1]
    for c, (t0, regular) in enumerate(cases):
        j0, j1 = span(s, c)
        assert running_at(oracle, j0, j1, 0) == (66, 65)  # (more than 64 in row 3: one is misplaced)
        head = 66 + t0 - 1
        assert starts_of(oracle, s, c)[head:head + 2] == [60, 61]
        assert completions_in(oracle, s, c, t0, 60) == [35]
        assert int((oracle[2][j0:j1] == 35).sum()) == 1 + regular
    run_and_compare(engine, arrays, s, oracle, diag)


# ---- the head's insert and the pool ---------------------------------------------------------------------
def test_heads_insert_spills_and_pool_exactly_full(engine, diag):
    """0: the head is placed at 20 and finishes at 35, in calendar row 3, which 64 TINY jobs fill: its slot
       is misplaced, and the BIG job behind it waits for exactly that slot.
    1: 511 TINY jobs and the BIG job before the head fill the pool; the head is placed when that job
       leaves, into the one free lane (not of its row), and the pool is full again: no escalation."""
    per = [
        [(0, 20, *BIG)] + tiny(0, [FAR + 3] * 64) + [(5, 15, *BIG), (5, 2, *BIG)] + ticks(21, 50) + tiny(900, [5] * 80),
        [(0, 20, *BIG)] + tiny(0, [80] * (POOL - 1)) + [(5, 30, *BIG)] + ticks(6, 90, 0) + tiny(90, [3] * 70),
    ]
    arrays, s = big_node_clusters(per), streams_of(per)
    oracle = oracle_of(arrays, s)
    stats = oracle[3]  # (on the CPU, first)
    assert not stats["flags"].any() and stats["waited"].tolist() == [2, 1]
    assert starts_of(oracle, s, 0)[65:67] == [20, 35] and running_at(oracle, *span(s, 0), 20) == (65, 65)
    assert starts_of(oracle, s, 1)[POOL] == 20 and stats["peak_running"][1] == POOL
    assert running_at(oracle, *span(s, 1), 5)[0] == POOL and running_at(oracle, *span(s, 1), 20)[0] == POOL
    cs = run_and_compare(engine, arrays, s, oracle, diag)
    assert not cs["flags"].any()


def test_pool_of_513_while_a_head_waits_escalates_once(diag):
    """512 TINY jobs and the BIG job before the head: the last insert was skipped, the head waits and is
    placed with the count above the pool, and the cluster is run again with a larger pool (an engine of
    its own: the larger pool stays with the engine)."""
    per = [[(0, 20, *BIG)] + tiny(0, [80] * POOL) + [(5, 30, *BIG)] + ticks(6, 90, 0) + tiny(90, [3] * 70)]
    arrays, s = big_node_clusters(per), streams_of(per)
    oracle = oracle_of(arrays, s)
    stats = oracle[3]  # (on the CPU, first)
    assert stats["peak_running"].tolist() == [POOL + 1] and stats["waited"].tolist() == [1]
    assert starts_of(oracle, s, 0)[POOL + 1] == 20
    with Engine(0) as eng:
        cs = run_and_compare(eng, arrays, s, oracle, diag, escalations=1)
    assert (cs["peak_running"] > POOL).all()


# ---- deadlocks --------------------------------------------------------------------------------------------
def test_deadlock_with_nothing_running(engine, diag):
    """The stream's only job; after earlier jobs have run and finished (the head sleeps to the last
    completion, fails again, and nothing runs any more); the head at lane 63; and a zero-duration head.
    The flag, the final clock and the waited count (the head still waiting counts) are the oracle's."""
    per = [
        [(3, 2, *NEVER)],
        [(0, 10, *BIG), (0, 3, *TINY), (5, 1, *NEVER), (6, 1, *TINY)],
        tiny(0, [4] * 63) + [(2, 1, *NEVER), (2, 1, *TINY), (3, 0, *TINY)],
        [(0, 10, *BIG), (0, 3, *TINY), (5, 0, *NEVER), (6, 1, *TINY)],
    ]
    arrays, s = big_node_clusters(per), streams_of(per)
    oracle = oracle_of(arrays, s)
    stats = oracle[3]  # (on the CPU, first)
    assert ((stats["flags"] & MCS_FLAG_DEADLOCK) != 0).all()
    assert stats["placed"].tolist() == [0, 2, 63, 2] and stats["waited"].tolist() == [1, 1, 1, 1]
    assert stats["t_end"].tolist() == [3, 10, 4, 10]
    run_and_compare(engine, arrays, s, oracle, diag)


# ---- a release in the sleep hands its payload back to the right node -----------------------------------------
def test_release_in_the_sleep_returns_payloads_to_edge_nodes(engine, diag):
    """Every node full (a 32-core job each, first fit: job i on node i).  The jobs on nodes 0, 3, 252, 255
    (and on node 128, the last real node of a 129-node cluster) finish 3 s apart; each of the 32-core
    heads behind them fails, sleeps to the next of those completions and fits that node only."""
    per, targets = [], ([0, 3, 252, 255], [0, 3, 128])
    for n, tg in zip((256, 129), targets):
        rows = [(0, 5 + 3 * tg.index(i) if i in tg else 500, 32, 1) for i in range(n)]
        per.append(rows + [(2, 300, 32, 1)] * len(tg) + tiny(40, [5] * 10))
    arrays, s = pack_clusters([uniform_cluster(256), uniform_cluster(129)]), streams_of(per)
    oracle = oracle_of(arrays, s)
    stats = oracle[3]  # (on the CPU, first)
    assert not stats["flags"].any() and stats["waited"].tolist() == [4, 3]
    for c, (n, tg) in enumerate(zip((256, 129), targets)):
        j0 = span(s, c)[0]
        assert oracle[0][j0:j0 + n].tolist() == list(range(n))
        assert oracle[0][j0 + n:j0 + n + len(tg)].tolist() == tg
        assert oracle[1][j0 + n:j0 + n + len(tg)].tolist() == [5 + 3 * i for i in range(len(tg))]
    run_and_compare(engine, arrays, s, oracle, diag)


# ---- fuzz ---------------------------------------------------------------------------------------------------
def crowded(seed, squeeze=16, stretch=8):
    """The standard fuzz streams (no request that never fits) under a heavy load: the arrival gaps cut to
    a sixteenth, the durations eight times as long, and every request with resources at least half of the
    stream's largest, so that a node holds one job and the clusters are overloaded."""
    arrays, s = fuzz_workload("w16r", seed, n_clusters=4, J=400, blocking=False)
    arr, dur, cores = s.arrival.copy(), s.dur.copy(), s.cores.copy()
    for c in range(4):
        j0, j1 = span(s, c)
        arr[j0:j1] //= squeeze
        dur[j0:j1] *= stretch
        nothing = (cores[j0:j1] == 0) & (s.mem[j0:j1] == 0)
        cores[j0:j1] = np.where(nothing, 0, np.maximum(cores[j0:j1], cores[j0:j1].max() // 2 + 1))
    return arrays, JobStreams(arr, dur, cores, s.mem, s.job_off)


@pytest.mark.parametrize("seed", [71, 72])
def test_fuzz_crowded_streams(engine, diag, seed):
    arrays, s = crowded(seed)
    oracle = oracle_of(arrays, s)
    assert not oracle[3]["flags"].any() and 5 * int(oracle[3]["waited"].sum()) >= int(s.job_off[-1])  # (a fifth wait)
    run_and_compare(engine, arrays, s, oracle, diag)


def test_fuzz_one_residue_bursts(engine, diag):
    per = residue_workload(54, n_clusters=2, J=800)
    arrays = pack_clusters([uniform_cluster(256), uniform_cluster(129)])
    s = streams_of(per)
    oracle = oracle_of(arrays, s)
    stats = oracle[3]  # (on the CPU, first)
    assert not stats["flags"].any() and stats["waited"].all() and (stats["peak_running"] <= POOL).all()
    j0, j1 = span(s, 0)  # rows overflow: more than 64 running jobs are due in one calendar row
    assert max(running_at(oracle, j0, j1, int(t))[1] for t in np.unique(oracle[1][j0:j1])) > LANES
    run_and_compare(engine, arrays, s, oracle, diag)
