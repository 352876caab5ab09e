"""The streamed W16R loop's bookkeeping ("scan trim"): the running-slot count and its
peak, the release scan's row tests (in pairs of slot rows), the re-pick of a slot row, and the
WaitQueue statistic (counted where the placed head is handled, and at the exits that leave a head
waiting).  None of it shows in a placement, so every case is a bit-exact parity run against the
oracle (node, start, finish and the five per-cluster statistics) on a stream built to drive one place
the bookkeeping can go wrong; a property a case relies on is asserted from the oracle's results on
the CPU before the GPU runs.  Every case runs the production and the counting build.  The cases pin
behaviour that any form of this bookkeeping must keep (they pass on the loop as it was before the
trim as well).  Run on a real MI355X: ``pytest -m gpu``.

The slot a job takes is the loop's own policy (tools/slot_model.py): from an empty pool the k-th
insert takes lane k % 64 of slot row k // 64, and a re-pick takes the next row with a free lane.  The
cases that aim at particular rows use bursts of one-MB jobs at t = 0, which all fit node 0.
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
BIG = (1, 20000)  # a request only node 0 of one_big_node() holds
SMALL = (0, 1)
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
    """Node 0 holds 24000 MB, every other node 100 MB: BIG requests queue up behind node 0."""
    return Cluster(Id=1, Nodes=[Node(Id=i + 1, Cores=32, Memory=24000 if i == 0 else 100, CoresAvailable=32,
                                     MemoryAvailable=24000 if i == 0 else 100) for i in range(n)])


def uniform_for(per_cluster):
    return pack_clusters([uniform_cluster(NODES[i % len(NODES)]) for i in range(len(per_cluster))])


def run_and_compare(engine, arrays, streams, oracle, escalations=0):
    on, os_, of, osd = oracle
    engine.load_clusters(arrays)
    engine.submit_jobs(streams)
    st = engine.run()
    node, start, fin = engine.placements()
    cs = engine.cluster_stats()
    if escalations == 0:
        assert engine.last_kernel == W16R
    bad = np.nonzero((node != on) | (start != os_) | (fin != of))[0]
    assert bad.size == 0, f"{bad.size} mismatches, first at job {bad[:5]}: gpu {node[bad[:5]]},{start[bad[:5]]} " \
                          f"oracle {on[bad[:5]]},{os_[bad[:5]]}"
    for key in ("t_end", "placed", "waited", "peak_running", "flags"):
        np.testing.assert_array_equal(cs[key], osd[key], err_msg=key)
    assert st.escalations == escalations and not (cs["flags"] & MCS_FLAG_OVERFLOW).any()
    return cs


def burst(t, n, dur):
    return [(t, dur, *SMALL)] * n


# ---- the peak, at every place it is taken ------------------------------------------------------------
def peak_streams():
    """(rows, the peak) per cluster."""
    zeros = {61, 63, 64, 66}
    return [
        # reached in the middle of the second batch, with no scan after it: the exit's candidate
        (burst(0, 100, 10), 100),
        # reached at a batch's last job: the batch end's candidate; everything is released before job 64
        (burst(0, 64, 10) + burst(20, 10, 5), 64),
        # reached right before a scan (the advance to t = 5 releases all 40), in the middle of a batch
        (burst(0, 40, 5) + burst(5, 11, 5), 40),
        # exactly the pool, in the middle of a batch (job 518, batch position 6), taken before the scan at 20
        (burst(0, 7, 3) + burst(5, POOL, 10) + burst(20, 5, 1), POOL),
        # zero-duration jobs on either side of the first batch boundary between inserts: they take no slot
        ([(0, 0 if i in zeros else 10, *SMALL) for i in range(70)]
         + [(10, 0 if i % 3 == 0 else 7, *SMALL) for i in range(30)], 66),
    ] + [(burst(0, n, 5), n) for n in (1, 63, 64, 65, 129)]  # stream lengths: the last batch's candidates


def test_peak_at_every_place_it_is_taken(engine, diag):
    """One cluster per stream of peak_streams(); the peak each one must report is asserted from the
    oracle first."""
    per = [rows for rows, _ in peak_streams()]
    arrays, s = uniform_for(per), streams_of(per)
    oracle = O.fifo_run_batch(arrays, s, n_threads=4)
    assert oracle[3]["peak_running"].tolist() == [p for _, p in peak_streams()]  # (on the CPU, first)
    assert not oracle[3]["waited"].any() and not oracle[3]["flags"].any()
    cs = run_and_compare(engine, arrays, s, oracle)
    assert cs["placed"].tolist() == [len(rows) for rows in per]


def test_peak_of_513_escalates_once(diag):
    """513 jobs running at once: the insert of the last finds no slot and is skipped, the count stays
    above the pool, and the cluster is run again with a larger pool (an engine of its own: the larger
    pool stays with the engine)."""
    per = [burst(0, 7, 3) + burst(5, POOL + 1, 10) + burst(20, 5, 1)] * 3
    arrays, s = uniform_for(per), streams_of(per)
    oracle = O.fifo_run_batch(arrays, s, n_threads=4)
    assert (oracle[3]["peak_running"] == POOL + 1).all()  # (on the CPU, first)
    with Engine(0) as eng:
        cs = run_and_compare(eng, arrays, s, oracle, escalations=1)
    assert (cs["peak_running"] > POOL).all()


# ---- expiries across the slot rows -------------------------------------------------------------------
FILL = 456  # rows 0-6 and eight lanes of row 7


def row_pattern_streams():
    """(rows, released at t = 10, the burst that follows) per cluster: 456 jobs at t = 0, those in the
    slot rows of the pattern with finish 10 and the others 100; a burst at t = 10 then takes the count
    above 456 by exactly burst - released, so the new peak tells whether the scan counted its rows."""
    out = []
    for rows_out, extra in (((0, 1), 150), ((2, 5), 150), ((7,), 30), (tuple(range(8)), 470)):
        rows = [(0, 10 if k // 64 in rows_out else 100, *SMALL) for k in range(FILL)]
        released = sum(k // 64 in rows_out for k in range(FILL))
        rows += burst(10, extra, 200) + burst(400, 3, 1)
        out.append((rows, released, extra))
    return out


def test_expiries_across_the_slot_rows(engine, diag):
    """One scan with expiries in both rows of one pair of slot rows, in one row each of two pairs, in
    row 7 only and in all eight rows; the peak is reached by the burst after the scan."""
    cases = row_pattern_streams()
    per = [rows for rows, _, _ in cases]
    arrays, s = uniform_for(per), streams_of(per)
    oracle = O.fifo_run_batch(arrays, s, n_threads=4)
    want = [max(FILL, FILL - released + extra) for _, released, extra in cases]  # (on the CPU, first)
    assert want == [478, 478, 478, 470] and oracle[3]["peak_running"].tolist() == want
    for c, (rows, released, _) in enumerate(cases):
        j0 = int(s.job_off[c])
        assert (oracle[2][j0:j0 + FILL] == 10).sum() == released and (oracle[1][j0 + FILL:j0 + len(rows) - 3] == 10).all()
    run_and_compare(engine, arrays, s, oracle)


# ---- the re-pick of a slot row --------------------------------------------------------------------------
def repick_streams():
    refill = burst(200, POOL, 10) + burst(300, 2, 1)  # the whole pool once more: a slot lost earlier overflows here
    return [
        # the pool full (current row 7, every lane handed out), row 7 released at t = 10: the re-pick of the
        # insert at t = 10 walks rows 0-6, all taken, and comes back to row 7
        [(0, 10 if k // 64 == 7 else 100, *SMALL) for k in range(POOL)] + burst(10, 64, 90) + refill,
        # lanes 0-9 of the current row 0 handed out and freed at t = 5; 502 inserts use up row 0 and fill rows
        # 1-7; the next ten come back to row 0 and must find those lanes: 512 running
        burst(0, 10, 5) + burst(5, 502, 100) + burst(6, 10, 99) + refill,
        # exactly full, one release (job 300, at t = 10), one insert
        [(0, 10 if k == 300 else 100, *SMALL) for k in range(POOL)] + burst(10, 1, 90) + refill,
    ]


def test_repick_finds_the_free_slots(engine, diag):
    per = repick_streams()
    arrays, s = uniform_for(per), streams_of(per)
    oracle = O.fifo_run_batch(arrays, s, n_threads=4)
    assert (oracle[3]["peak_running"] == POOL).all() and not oracle[3]["waited"].any()  # (on the CPU, first)
    for c, rows in enumerate(per):  # every job starts when it arrives: the pool is never the limit
        j0 = int(s.job_off[c])
        assert oracle[1][j0:j0 + len(rows)].tolist() == [r[0] for r in rows]
    run_and_compare(engine, arrays, s, oracle)


# ---- the WaitQueue statistic -------------------------------------------------------------------------
def test_waited(engine, diag):
    """one_big_node clusters: every job but the first waits (the first meets an empty cluster); none
    waits; the stream ends with a head waiting on a request no node can hold (the deadlock flag, the
    head counted); one head fails at its arrival and at three completions before it fits at the fourth."""
    everyone = [(0, 10, *BIG)] * 70
    nobody = [(3 * i, 2, *SMALL) for i in range(70)]
    stuck = [(0, 10, *BIG), (0, 10, *BIG), (0, 3, *SMALL), (5, 1, 1, 30000), (6, 1, *SMALL)]
    again = [(0, 40, *BIG), (0, 10, 1, 50), (0, 20, 1, 50), (0, 30, 1, 50), (0, 5, *BIG), (0, 2, *SMALL), (41, 1, *SMALL)]
    per = [everyone, nobody, stuck, again]
    arrays = pack_clusters([one_big_node(n) for n in (129, 200, 255, 256)])
    s = streams_of(per)
    oracle = O.fifo_run_batch(arrays, s, n_threads=4)
    off = [int(x) for x in s.job_off]
    stats = oracle[3]  # (on the CPU, first)
    assert stats["waited"].tolist()[:2] == [69, 0] and stats["placed"].tolist() == [70, 70, 3, 7]
    assert stats["flags"][2] & MCS_FLAG_DEADLOCK and stats["waited"][2] == 2 and not stats["flags"][[0, 1, 3]].any()
    a0 = off[3]
    assert sorted(oracle[2][a0 + 1:a0 + 4].tolist()) == [10, 20, 30] and oracle[1][a0 + 4] == 40
    assert stats["waited"][3] == 1 and oracle[1][a0 + 5] == 41
    run_and_compare(engine, arrays, s, oracle)


@pytest.mark.parametrize("seed", [21, 22])
def test_fuzz_streams_through_the_trimmed_loop(engine, diag, seed):
    arrays, s = fuzz_workload("w16r", seed, n_clusters=64, J=2000)
    oracle = O.fifo_run_batch(arrays, s, n_threads=8)
    assert (oracle[3]["peak_running"] <= POOL).all() and oracle[3]["waited"].any()
    run_and_compare(engine, arrays, s, oracle)
