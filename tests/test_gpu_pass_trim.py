"""The streamed W16R loop's failed-fit path, runaway guard and released count ("pass
trim"): a failed fit falls straight into the release scan, the guard counts down from its bound, and
the scan's rows count their released slots out of the running count itself.  None of it shows in a
placement unless it goes wrong, so every case is a bit-exact parity run against the oracle (node,
start, finish, waited, peak_running, flags, t_end) on a stream built to drive one of those places; the
property a case relies on is asserted from the oracle's results on the CPU before the GPU runs.  Every
case runs the production and the counting build and asserts the kernel it ran on.  The cases pin
behaviour that does not change: they pass on the loop as it was before as well.  Run on a real
MI355X: ``pytest -m gpu``.

The clusters of the failed-fit cases are one_big_node(): node 0 holds 24000 MB and every other node
100 MB, so a BIG request (20000 MB) runs on node 0 alone, one at a time, a MID request (50 MB) on any
node, and SMALL ones (1 MB) share node 0 with a BIG one.  The slot a job takes is the loop's own policy
(tools/slot_model.py): from an empty pool the k-th insert takes lane k % 64 of slot row k // 64.
"""
import numpy as np
import pytest

import oracle_ref as O
from kat_util import fuzz_workload
from mcs_amd import MCS_FLAG_DEADLOCK, MCS_FLAG_OVERFLOW, Engine, JobStreams, pack_clusters, uniform_cluster
from mcs_amd.cluster import Cluster, Node

pytestmark = pytest.mark.gpu

W16R = "mcs::fifo_asm_kernel<16, true, 4, 8>"
NODES = (129, 200, 233, 255, 256)  # the W16R shape: padding lanes, padding chunks, none
BIG = (1, 20000)
MID = (1, 50)
SMALL = (0, 1)
NEVER = (1, 30000)  # no node holds it
POOL = 512


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


def burst(t, n, dur):
    return [(t, dur, *SMALL)] * n


def run_and_compare(engine, arrays, streams, oracle, escalations=0):
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
    assert st.escalations == escalations and not (cs["flags"] & MCS_FLAG_OVERFLOW).any()
    return cs


# ---- the failed-fit path -----------------------------------------------------------------------------
def failed_fit_streams():
    """(rows, index of the head under test, its start) per cluster."""
    def completions(k):  # the head fails at its arrival and at k completions, and fits at the next
        return [(0, 10 * (k + 1), *BIG)] + [(0, 10 * (i + 1), *MID) for i in range(k)] \
            + [(0, 5, *BIG), (0, 2, *SMALL), (10 * (k + 1) + 1, 1, *SMALL)]
    out = [(completions(k), k + 1, 10 * (k + 1)) for k in (1, 2, 3)]
    # the earliest finish is exactly t + 1, and later than t + 1
    out.append(([(0, 1, *BIG), (0, 4, *BIG), (0, 1, *SMALL)], 1, 1))
    out.append(([(0, 7, *BIG), (0, 4, *BIG), (0, 1, *SMALL)], 1, 7))
    # an arrival advance that releases nothing (0 -> 5, the earliest finish is 50), then the failed fit
    out.append(([(0, 50, *BIG), (5, 3, *BIG), (5, 1, *SMALL)], 1, 50))
    # the failing head is the last job of a batch (62 lanes of one slot row expire at its first retry)
    out.append(([(0, 30, *BIG)] + burst(0, 62, 5) + [(0, 3, *BIG)] + burst(0, 5, 2), 63, 30))
    # ... and the last job of the stream
    out.append(([(0, 30, *BIG)] + burst(0, 62, 5) + [(0, 3, *BIG)], 63, 30))
    return out


def test_failed_fit_falls_into_the_scan(engine, diag):
    cases = failed_fit_streams()
    per = [rows for rows, _, _ in cases]
    arrays, s = big_node_clusters(per), streams_of(per)
    oracle = O.fifo_run_batch(arrays, s, n_threads=4)
    stats = oracle[3]  # (on the CPU, first)
    assert not stats["flags"].any() and stats["placed"].tolist() == [len(rows) for rows in per]
    assert stats["waited"].tolist() == [1] * len(per)
    for c, (rows, head, start) in enumerate(cases):
        j0 = int(s.job_off[c])
        assert oracle[1][j0 + head] == start and oracle[0][j0 + head] == 0
        if head + 1 < len(rows):  # the job after a placed WaitQueue head starts a second later
            assert oracle[1][j0 + head + 1] == start + 1
    run_and_compare(engine, arrays, s, oracle)


def test_deadlocks(engine, diag):
    """A head no node holds with nothing running (the first job, and the only one), and after earlier
    jobs ran: the DEADLOCK flag, the waiting head counted once, nothing placed after it."""
    per = [
        [(0, 1, *NEVER), (1, 1, *SMALL)],
        [(3, 2, *NEVER)],
        [(0, 10, *BIG), (0, 10, *BIG), (0, 3, *SMALL), (5, 1, *NEVER), (6, 1, *SMALL)],
        [(0, 4, *SMALL)] * 64 + [(2, 1, *NEVER)] + burst(2, 3, 1),  # the head of a new batch
    ]
    arrays, s = big_node_clusters(per), streams_of(per)
    oracle = O.fifo_run_batch(arrays, s, n_threads=4)
    stats = oracle[3]  # (on the CPU, first)
    assert (stats["flags"] & MCS_FLAG_DEADLOCK).all()
    assert stats["placed"].tolist() == [0, 0, 3, 64] and stats["waited"].tolist() == [1, 1, 2, 1]
    run_and_compare(engine, arrays, s, oracle)


# ---- the runaway guard's bound -----------------------------------------------------------------------
def guard_stream(J):
    """Failed fits as dense as first fit allows: a failed fit either meets a head at its arrival or uses
    up a completion that frees nothing the head needs, and the job that completed there blocks no later
    head, so the BIG jobs alternate with MID ones that never wait.  Every BIG job but the first fails
    twice, once at its arrival (after an arrival advance that releases nothing) and once at the MID
    job's completion, and is placed at the completion of the BIG job before it."""
    rows, t = [], 0  # t: the placement of the last BIG job
    for k in range(J):
        if k % 2 == 0:
            rows.append((t + 2 if k else 0, 10, *BIG))
            t = t + 10 if k else 0
        else:
            rows.append((rows[-1][0], 4, *MID))  # (arrived long before it becomes the head)
    return rows


GUARD_J = (1, 63, 64, 65, 129)


def test_guard_bound_leaves_dense_failed_fits_alone(engine, diag):
    """No test trips the guard: these streams stay far below 4J + 256 and must end with flags 0."""
    per = [guard_stream(J) for J in GUARD_J]
    arrays, s = big_node_clusters(per), streams_of(per)
    oracle = O.fifo_run_batch(arrays, s, n_threads=4)
    stats = oracle[3]  # (on the CPU, first)
    assert not stats["flags"].any() and stats["placed"].tolist() == list(GUARD_J)
    assert stats["waited"].tolist() == [(J - 1) // 2 for J in GUARD_J]
    for c, J in enumerate(GUARD_J):
        j0 = int(s.job_off[c])
        # BIG job k starts when the one before it ends; the MID job after a placed head a second later
        assert oracle[1][j0:j0 + J:2].tolist() == [10 * i for i in range((J + 1) // 2)]
        assert oracle[1][j0 + 3:j0 + J:2].tolist() == [10 * i + 1 for i in range(1, J // 2)]
    if diag == "1":  # the counting build reports the passes: 2 failed fits and an arrival advance per BIG job
        cs = run_and_compare(engine, arrays, s, oracle)
        assert cs["iterations"].tolist() == [J + 3 * ((J - 1) // 2) for J in GUARD_J]
    else:
        run_and_compare(engine, arrays, s, oracle)


# ---- the released count --------------------------------------------------------------------------------
FILL = 456  # rows 0-6 and eight lanes of row 7


def row_pattern_streams():
    """(rows, released at t = 10, the burst that follows) per cluster: 456 jobs at t = 0, those in the
    slot rows of the pattern with finish 10 and the others 100; a burst at t = 10 then takes the count
    above 456 by exactly burst - released, so the new peak tells whether the scan counted its rows."""
    out = []
    for rows_out, extra in (((2,), 100), ((7,), 30), ((4, 5), 150), ((1, 6), 150), (tuple(range(8)), 470)):
        rows = [(0, 10 if k // 64 in rows_out else 100, *SMALL) for k in range(FILL)]
        released = sum(k // 64 in rows_out for k in range(FILL))
        rows += burst(10, extra, 200) + burst(400, 3, 1)
        out.append((rows, released, extra))
    # one lane of one row (the count of a row is 1), and one lane in each row of a pair
    for lanes, extra in (((130,), 3), ((130, 200), 5)):
        rows = [(0, 10 if k in lanes else 100, *SMALL) for k in range(FILL)]
        rows += burst(10, extra, 200) + burst(400, 3, 1)
        out.append((rows, len(lanes), extra))
    return out


def test_rows_count_their_released_slots(engine, diag):
    """One scan releasing one row, two rows (both of a pair; one each of two pairs) and all eight, whole
    rows (64 or 8 lanes in a row's count) and single lanes; the peak is reached by the burst after it."""
    cases = row_pattern_streams()
    per = [rows for rows, _, _ in cases]
    arrays, s = uniform_for(per), streams_of(per)
    oracle = O.fifo_run_batch(arrays, s, n_threads=4)
    want = [max(FILL, FILL - released + extra) for _, released, extra in cases]  # (on the CPU, first)
    assert want == [492, 478, 478, 478, 470, 458, 459] and oracle[3]["peak_running"].tolist() == want
    for c, (rows, released, _) in enumerate(cases):
        j0 = int(s.job_off[c])
        assert (oracle[2][j0:j0 + FILL] == 10).sum() == released and (oracle[1][j0 + FILL:j0 + len(rows) - 3] == 10).all()
    run_and_compare(engine, arrays, s, oracle)


def test_peak_of_exactly_the_pool_and_at_a_batch_end(engine, diag):
    """512 running, in the middle of a batch, taken before the scan at t = 20; and a peak reached at a
    batch's last job (64, 128) with no scan after it: the batch end's and the exit's candidates."""
    per = [
        burst(0, 7, 3) + burst(5, POOL, 10) + burst(20, 5, 1),
        burst(0, 64, 10),
        burst(0, 30, 2) + burst(3, 98, 10),
    ]
    arrays, s = uniform_for(per), streams_of(per)
    oracle = O.fifo_run_batch(arrays, s, n_threads=4)
    assert oracle[3]["peak_running"].tolist() == [POOL, 64, 98]  # (on the CPU, first)
    assert not oracle[3]["waited"].any() and not oracle[3]["flags"].any()
    run_and_compare(engine, arrays, s, oracle)


def test_peak_of_513_escalates_once(diag):
    """513 jobs running at once: the insert of the last finds no slot and is skipped, the count stays
    above the pool, and the cluster is run again with a larger pool (an engine of its own: the larger
    pool stays with the engine)."""
    per = [burst(0, 7, 3) + burst(5, POOL + 1, 10) + burst(20, 5, 1)] * 2
    arrays, s = uniform_for(per), streams_of(per)
    oracle = O.fifo_run_batch(arrays, s, n_threads=4)
    assert (oracle[3]["peak_running"] == POOL + 1).all()  # (on the CPU, first)
    with Engine(0) as eng:
        cs = run_and_compare(eng, arrays, s, oracle, escalations=1)
    assert (cs["peak_running"] > POOL).all()


@pytest.mark.parametrize("seed", [31, 32])
def test_fuzz_streams(engine, diag, seed):
    arrays, s = fuzz_workload("w16r", seed, n_clusters=8, J=400)
    oracle = O.fifo_run_batch(arrays, s, n_threads=4)
    assert oracle[3]["waited"].any()  # (failed fits happen)
    run_and_compare(engine, arrays, s, oracle)
