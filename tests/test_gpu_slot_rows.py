"""The streamed W16R loop's running-slot rows: written for the loop before calendar
rows, whose insert took a lane of the current row from a scalar mask and re-picked a row when the
mask ran out; the calendar loop takes a lane of row finish & 7 and spills to the next row with a free
lane, and the same streams fill and cycle its rows.  Which slot a job gets
never shows in a result, so each case is a plain parity run against the oracle (node, start, finish
and the per-cluster statistics, bit-exact) on a stream that drives the pool through the paths of the
re-pick: rows cycling with the pool near full, the pool exactly full and then a release, and
randomised streams whose batch ends and zero-duration jobs fall anywhere in a row.  Pools over 512
slots are the escalation test's (tests/test_gpu_parity.py).  Run on a real MI355X: ``pytest -m gpu``.
"""
import numpy as np
import pytest

import oracle_ref as O
from kat_util import fuzz_workload
from mcs_amd import MCS_FLAG_OVERFLOW, JobStreams, pack_clusters, uniform_cluster

pytestmark = pytest.mark.gpu

W16R = "mcs::fifo_asm_kernel<16, true, 4, 8>"
POOL = 64 * 8  # slots of the hand-scheduled loop: 64 lanes x 8 rows
NODES = (200, 233, 255, 256)  # 129-256 nodes: the W16R shape, with and without padding lanes


def steady_stream(n_clusters, n_jobs, per_second, dur):
    """Zero-core 1-MB jobs, per_second arrivals each second, durations dur (a scalar, or one array
    per cluster): nothing ever waits, and per_second * dur jobs run at once."""
    a = np.repeat(np.arange(n_jobs // per_second + 1, dtype=np.uint32), per_second)[:n_jobs]
    durs = [np.full(n_jobs, d, np.uint32) if np.isscalar(d) else d.astype(np.uint32)
            for d in (dur if isinstance(dur, list) else [dur] * n_clusters)]
    return JobStreams(np.tile(a, n_clusters), np.concatenate(durs), np.zeros(n_clusters * n_jobs, np.uint32),
                      np.ones(n_clusters * n_jobs, np.uint32), np.arange(n_clusters + 1, dtype=np.uint64) * n_jobs)


def run_and_compare(engine, arrays, streams, oracle=None):
    """The engine's run against the oracle's (computed once per case), bit-exact; returns the run's
    stats, the per-cluster stats and the oracle's per-cluster stats."""
    on, os_, of, osd = oracle if oracle is not None else O.fifo_run_batch(arrays, streams, n_threads=8)
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
    return st, cs, osd


def test_rows_cycle_with_the_pool_near_full(engine):
    """5 arrivals per second of duration 100: about 500 of the 512 slots are taken, so a row's free
    lanes are the few a release has just returned and every row is re-picked again and again over
    the 3000 jobs (600 s, six turnovers of the pool).  Two clusters release in insert order (one
    duration); two with durations of 90-110 release out of order, from several rows per scan."""
    n = 3000
    rng = np.random.default_rng(0x51)
    dur = [100, 100, rng.integers(90, 111, n), rng.integers(90, 111, n)]
    arrays = pack_clusters([uniform_cluster(k) for k in NODES])
    s = steady_stream(len(NODES), n, 5, dur)
    oracle = O.fifo_run_batch(arrays, s, n_threads=4)
    peak = oracle[3]["peak_running"]
    assert (peak >= 480).all() and (peak <= POOL).all(), peak  # (the stream's own property, on the CPU)
    st, cs, _ = run_and_compare(engine, arrays, s, oracle)
    assert st.escalations == 0
    assert not (cs["flags"] & MCS_FLAG_OVERFLOW).any()


def test_pool_exactly_full_then_a_release(engine):
    """8 arrivals per second of duration 64: from second 63 on, every second's 8 inserts fill the pool
    to exactly 512 and the next second's release frees 8 slots (some in the current row, whose mask
    is empty) that the following inserts must find by a re-pick.  No insert is ever skipped: no
    overflow, no escalation."""
    n = 2000
    arrays = pack_clusters([uniform_cluster(k) for k in NODES])
    s = steady_stream(len(NODES), n, 8, 64)
    oracle = O.fifo_run_batch(arrays, s, n_threads=4)
    assert (oracle[3]["peak_running"] == POOL).all(), oracle[3]["peak_running"]  # on the CPU, first
    st, cs, _ = run_and_compare(engine, arrays, s, oracle)
    assert (cs["peak_running"] == POOL).all()
    assert st.escalations == 0
    assert not (cs["flags"] & MCS_FLAG_OVERFLOW).any()


@pytest.mark.parametrize("seed", [7, 8])
def test_fuzz_streams_through_the_slot_rows(engine, seed):
    """Randomised clusters and streams (bursts, idle stretches, zero-duration and zero-resource jobs,
    a request that fits no node): re-picks fall on batch ends, after zero-duration jobs and after
    scans that free several rows.  No cluster's peak passes the pool (the oracle's statistics, on
    the CPU), so every cluster runs the hand-scheduled loop to its end."""
    arrays, s = fuzz_workload("w16r", seed, n_clusters=64, J=2000)
    oracle = O.fifo_run_batch(arrays, s, n_threads=8)
    peak = oracle[3]["peak_running"]
    assert peak.max() > 64 and (peak <= POOL).all() and (s.dur == 0).any()  # more than one row in use
    st, cs, _ = run_and_compare(engine, arrays, s, oracle)
    assert st.escalations == 0
    assert not (cs["flags"] & MCS_FLAG_OVERFLOW).any()
