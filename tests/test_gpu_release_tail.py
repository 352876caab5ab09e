"""The streamed W16R loop's release scan and what rides on it ("release tail"): the LDS
node copy as one 16-byte word per lane with the node index as the decision's kx, the head job's fit
test carried in the scan's DPP wait states, and zero-duration jobs routed through the arrival test.
None of it shows in a result, so every case is a bit-exact parity run against the oracle (node,
start, finish and the five per-cluster statistics) on a stream built to drive one of those paths;
where a case names a property of its stream, that property is asserted from the oracle's results on
the CPU before the GPU runs.  Every case runs the production and the counting build.  A non-zero
job arriving at 0xffffffff is not a case: the engine rejects such a stream (its clock bound), and
without the bound it runs the compiled kernel.  Run on a real MI355X: ``pytest -m gpu``.
"""
import numpy as np
import pytest

import oracle_ref as O
from kat_util import fuzz_workload
from mcs_amd import MCS_FLAG_DEADLOCK, MCS_FLAG_OVERFLOW, JobStreams, pack_clusters, uniform_cluster
from mcs_amd.cluster import Cluster, Node

pytestmark = pytest.mark.gpu

W16R = "mcs::fifo_asm_kernel<16, true, 4, 8>"
NODES = (129, 200, 233, 255, 256)  # the W16R shape: padding lanes, padding chunks, none
BIG = (1, 20000)  # a request only node 0 of one_big_node() holds
SMALL = (0, 1)


@pytest.fixture(params=["0", "1"], ids=["prod", "diag"])
def diag(request, monkeypatch):
    monkeypatch.setenv("MCS_FIFO_DIAG", request.param)
    return request.param


def streams_of(per_cluster):
    """JobStreams from one list of (arrival, duration, cores, memory) rows per cluster."""
    cols = [np.array([r[f] for rows in per_cluster for r in rows], np.uint32) for f in range(4)]
    off = np.cumsum([0] + [len(rows) for rows in per_cluster]).astype(np.uint64)
    return JobStreams(*cols, off)


def ramp_cluster(n):
    """Node i holds 32 cores and 100 + i MB: a request of 100 + i MB first-fits node i while it is
    free, so a wrong chunk / lane mapping of a node word changes a placement."""
    return Cluster(Id=1, Nodes=[Node(Id=i + 1, Cores=32, Memory=100 + i, CoresAvailable=32, MemoryAvailable=100 + i)
                                for i in range(n)])


def one_big_node(n):
    """Node 0 holds 24000 MB, every other node 100 MB: BIG requests queue up behind node 0."""
    return Cluster(Id=1, Nodes=[Node(Id=i + 1, Cores=32, Memory=24000 if i == 0 else 100, CoresAvailable=32,
                                     MemoryAvailable=24000 if i == 0 else 100) for i in range(n)])


def run_and_compare(engine, arrays, streams, oracle):
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
    assert st.escalations == 0 and not (cs["flags"] & MCS_FLAG_OVERFLOW).any()
    return cs


# ---- the node copy's layout ------------------------------------------------------------------------
def test_layout_one_scan_releases_to_every_chunk(engine, diag):
    """Ramp clusters.  Eight jobs at t = 0 take all four chunks of lane 2 (nodes 8-11) and the last
    lane's nodes (lane 63 chunks 0-3 of the 256-node cluster: node 255 is lane 63 chunk 3), all with
    finish 5; at t = 5 one scan hands them back and the same requests come again and must find the
    same nodes.  A random tail follows (requests across the ramp, durations 0-40, some waiting)."""
    rng = np.random.default_rng(0xA1)
    per, marks = [], []
    for n in NODES:
        ks = [8, 9, 10, 11] + list(range(n - 4, n))
        rows = [(0, 5, 1, 100 + k) for k in ks] + [(5, 7, 1, 100 + k) for k in ks]
        arr = 5 + np.cumsum(rng.poisson(0.3, 2400))
        rows += [(int(a), int(rng.integers(0, 41)), int(rng.integers(0, 33)), int(rng.integers(0, 100 + n)))
                 for a in arr]
        per.append(rows)
        marks.append(ks)
    arrays, s = pack_clusters([ramp_cluster(n) for n in NODES]), streams_of(per)
    oracle = O.fifo_run_batch(arrays, s, n_threads=4)
    for c, ks in enumerate(marks):  # (on the CPU, first)
        j0 = int(s.job_off[c])
        assert oracle[0][j0:j0 + 16].tolist() == ks + ks
        assert (oracle[2][j0:j0 + 8] == 5).all() and (oracle[1][j0 + 8:j0 + 16] == 5).all()
    assert marks[-1][-1] == 255 and (oracle[3]["waited"] > 0).any()
    run_and_compare(engine, arrays, s, oracle)


def test_layout_stream_lengths(engine, diag):
    """Streams of 1, 63, 64, 65, 129 and 2049 jobs (the last batch's store in the loop and in the
    epilogue, which takes the node index as it is) on 129-node ramp clusters, whose lanes 33-63 and
    chunks 1-3 of lane 32 are padding: requests across the ramp, so node indices of every lane and
    chunk are stored."""
    rng = np.random.default_rng(0xA2)
    lens = (1, 63, 64, 65, 129, 2049)
    per = []
    for J in lens:
        arr = np.cumsum(rng.poisson(0.4, J))
        per.append([(int(a), int(rng.integers(1, 30)), 1, int(rng.integers(0, 229))) for a in arr])
    arrays, s = pack_clusters([ramp_cluster(129)] * len(lens)), streams_of(per)
    oracle = O.fifo_run_batch(arrays, s, n_threads=4)
    assert oracle[0].max() == 128 and len(np.unique(oracle[0] % 4)) == 4
    cs = run_and_compare(engine, arrays, s, oracle)
    assert cs["placed"].tolist() == list(lens)


# ---- what follows a scan ---------------------------------------------------------------------------
def tail_stream():
    pad = [(61, 100, *SMALL)] * 52
    rows = [(0, 10, *BIG), (0, 11, *SMALL),
            (0, 10, *BIG),  # 2: fails at 0; the scan at 10 is followed by a head that fits
            # (its one-second sleep ends at 11 with a scan, and the head, job 3, arrives at 12)
            (12, 3, *SMALL), (12, 5, *SMALL), (13, 9, *SMALL),
            (50, 10, *BIG),  # 6: the arrival advance 13 -> 50 releases finishes 15, 17, 20 and 22
            (50, 5, *SMALL),
            (50, 10, *BIG)]  # 8: fails at 50, again after the scan at 55, placed at 60
    rows += pad + [(61, 20, *SMALL),  # 61: finishes at 81
                        (61, 10, *BIG),  # 62: waits for job 8 (70)
                        (61, 10, *BIG)]  # 63: placed at 80 as the batch's last job; the scan at 81 has no job left
    rows += [(100, 10, *BIG), (100, 21, *SMALL), (100, 10, *BIG),
             (100, 10, *BIG)]  # 67: the stream's last job, placed at 120 from the WaitQueue; scan at 121
    return rows


def test_tail_heads_after_a_scan(engine, diag):
    """one_big_node clusters: BIG jobs queue behind node 0, SMALL ones set the finish seconds.  In turn
    a scan is followed by a head that fits (job 2), a head that has not arrived after a placed
    WaitQueue head's sleep (job 3), a head that fails twice in a row (job 8), no job left in the batch
    (after job 63) and the end of the stream (after job 67); the advance to job 6 releases finishes
    of four different seconds."""
    rows = tail_stream()
    assert len(rows) == 68
    arrays, s = pack_clusters([one_big_node(n) for n in NODES]), streams_of([rows] * len(NODES))
    oracle = O.fifo_run_batch(arrays, s, n_threads=4)
    start, fin = oracle[1][:68], oracle[2][:68]  # (on the CPU, first)
    assert start[[2, 3, 6, 8, 62, 63, 66, 67]].tolist() == [10, 12, 50, 60, 70, 80, 110, 120]
    assert sorted(fin[[2, 3, 4, 5]].tolist()) == [15, 17, 20, 22] and fin[1] == 11 and fin[7] == 55
    assert fin[61] == 81 and fin[65] == 121 and (oracle[0][:68][[0, 2, 6, 8, 62, 63, 64, 66, 67]] == 0).all()
    assert (oracle[3]["waited"] == 6).all() and not oracle[3]["flags"].any()  # (jobs 2, 8, 62, 63, 66, 67)
    run_and_compare(engine, arrays, s, oracle)


def test_tail_burst_expires_all_eight_rows(engine, diag):
    """500 one-MB jobs at t = 0 with one finish fill slot rows 0-6 and most of row 7; the advance to
    the next arrival at t = 10 expires all eight rows in one scan, and its head then fits.  A second
    burst with durations 1-8 is released by one advance across eight finish seconds."""
    rows = [(0, 10, *SMALL)] * 500 + [(10, int(1 + i % 8), *SMALL) for i in range(500)]
    rows += [(100, 3, 1, 50)] * 400
    arrays, s = pack_clusters([uniform_cluster(n) for n in NODES]), streams_of([rows] * len(NODES))
    oracle = O.fifo_run_batch(arrays, s, n_threads=4)
    assert (oracle[3]["peak_running"] == 500).all()  # (on the CPU, first: rows 0-7 in use, 7 x 64 + 52)
    assert (oracle[2][:500] == 10).all() and (oracle[1][500:1000] == 10).all() and (oracle[1][1000:1400] == 100).all()
    run_and_compare(engine, arrays, s, oracle)


# ---- zero-duration jobs ------------------------------------------------------------------------------
def zero_stream():
    rows = [(0, 0, *SMALL),  # 0: batch position 0
            (0, 10, *BIG), (0, 11, *SMALL),
            (0, 0, *BIG),  # 3: a WaitQueue head that fits only after the release at 10
            (30, 0, *SMALL),  # 4: not arrived when the head's sleep ends (scan at 11)
            (30, 0, *SMALL), (30, 0, *SMALL), (30, 0, *BIG)]  # several in a row
    rows += [(30, 50, *SMALL)] * 55
    rows += [(31, 0, *SMALL), (31, 0, 1, 60)]  # batch positions 63 and 64
    rows += [(32, 5, *SMALL), (32, 0, *BIG), (40, 0, *SMALL)]
    return rows


def test_zero_durations(engine, diag):
    """Zero-duration jobs at batch positions 0, 63 and 64, four in a row, as a WaitQueue head that
    fits only after a release, and not yet arrived after a one-second sleep (one_big_node clusters);
    a last cluster ends on a zero-duration request no node can hold: the deadlock flag, the jobs
    after it unplaced."""
    rows = zero_stream()
    assert len(rows) == 68 and rows[63][1] == 0 and rows[64][1] == 0
    stuck = [(0, 3, *SMALL), (0, 0, 1, 30000), (0, 1, *SMALL)]
    clusters = [one_big_node(n) for n in NODES] + [one_big_node(129)]
    arrays, s = pack_clusters(clusters), streams_of([rows] * len(NODES) + [stuck])
    oracle = O.fifo_run_batch(arrays, s, n_threads=4)
    start, fin = oracle[1][:68], oracle[2][:68]  # (on the CPU, first)
    z = [i for i, r in enumerate(rows) if r[1] == 0]
    assert (start[z] == fin[z]).all() and start[[0, 3, 4, 7, 63, 64]].tolist() == [0, 10, 30, 30, 31, 31]
    assert (oracle[3]["waited"][:-1] == 1).all()
    assert oracle[3]["flags"][-1] & MCS_FLAG_DEADLOCK and oracle[3]["placed"][-1] == 1
    run_and_compare(engine, arrays, s, oracle)


@pytest.mark.parametrize("seed", [11, 12])
def test_fuzz_streams_through_the_release_tail(engine, diag, seed):
    arrays, s = fuzz_workload("w16r", seed, n_clusters=64, J=2000)
    assert (s.dur == 0).any()
    oracle = O.fifo_run_batch(arrays, s, n_threads=8)
    assert (oracle[3]["peak_running"] <= 64 * 8).all()
    run_and_compare(engine, arrays, s, oracle)
