"""The DELAY edge workloads (tests/delay_edges.py) on the CPU: each one reaches the edge it is built for
(read from the trace of tests/delay_ref.py, the plain per-second restatement of Scheduler.Delay), and the
oracle (oracle/mcs_oracle_delay.c, fast-forward and literal) equals that reference on every output and
statistic, so tests/test_gpu_delay_edges.py compares the hand-scheduled loop with an oracle that a second,
independent restatement and hand-worked cases pin on the same streams.  No GPU needed."""
import json
import os

import numpy as np
import pytest

import delay_edges as E
import oracle_ref as O
from delay_ref import delay_ref
from kat_util import GOLDEN

DKATS = json.load(open(os.path.join(GOLDEN, "kats_delay.json")))["delay"]
CASES = [(fam, c) for fam, f in E.FAMILIES.items() if fam != "mixed" for c in f()] + \
        [("mixed", c) for c in E.mixed_family() if c.name in ("quiet", "one_node")]
STATS = ("t_end", "placed", "moved_l1", "placed_l1", "peak_l1", "peak_running", "flags", "l1_left",
         "total_wait_ms", "jobs_count", "ticks")


def columns(c):
    j = np.array(c.jobs, np.uint32).reshape(-1, 4)
    return j[:, 0], j[:, 1], j[:, 2], j[:, 3]


def assert_same(got, ref, what):
    for x, y, nm in zip(got[:3], ref[:3], ("node", "start", "finish")):
        np.testing.assert_array_equal(x, y, err_msg=f"{what}: {nm}")
    for k in STATS:
        assert got[3][k] == ref[3][k], f"{what}: {k}"


def check(c, max_wait_s=10):
    cols = columns(c)
    ref = delay_ref(c.free_c, c.free_m, *cols, max_wait_s=max_wait_s)
    st, tr = ref[3], ref[4]
    if c.hit is not None:
        assert c.hit(st, tr), f"{c.name} misses its edge: {st}"
    assert_same(O.delay_run(c.free_c, c.free_m, *cols, max_wait_s=max_wait_s), ref, "oracle")
    if st["t_end"] < 100_000:  # one iteration per second, in C
        assert_same(O.delay_run(c.free_c, c.free_m, *cols, literal=True, max_wait_s=max_wait_s), ref, "literal oracle")
    if st["t_end"] * (1 + st["peak_l1"]) < 40_000:  # and in Python, without the reference's one shortcut
        assert_same(delay_ref(c.free_c, c.free_m, *cols, max_wait_s=max_wait_s, jump=False), ref, "reference, no jump")
    return ref


@pytest.mark.parametrize("fam,c", CASES, ids=[c.name for _, c in CASES])
def test_edge_is_hit_and_oracle_equals_reference(fam, c):
    check(c)


@pytest.mark.parametrize("mw", [1, 1000])
def test_rows_at_other_max_wait(mw):
    for c in E.rows_family(mw):
        st = check(c, mw)[3]
        assert st["moved_l1"] == len(c.jobs) - 1 and st["t_end"] > mw + len(c.jobs)


@pytest.mark.parametrize("fam", list(E.FAMILIES))
def test_packed_family_equals_single_clusters(fam):
    """the launches the GPU tests make (delay_edges.pack) hold the clusters the cases describe"""
    cases = E.FAMILIES[fam]()
    assert len(cases) <= 16 and max(len(c.jobs) for c in cases) <= 1500
    assert all(129 <= len(c.free_c) <= 256 for c in cases if c.name != "one_node")
    arrays, streams = E.pack(cases)
    node, start, fin, ds = O.delay_run_batch(arrays, streams, n_threads=4)
    for k, c in enumerate(cases):
        one = O.delay_run(c.free_c, c.free_m, *columns(c))
        js = streams.of(k)
        assert_same((node[js], start[js], fin[js], {n: ds[n][k] for n in STATS}), one, c.name)


def test_hand_worked_even_positions():
    """rows(3): node 0 has 700 cores, the 255 others nothing.  J0 (700 cores, 43 s) starts at t = 0.  J1-J3
    (1 core, 3 s, all arrived at 0) fail as Level0 heads: J1 moves at t = 10 (waited 10 >= 10), J2 at 11, J3
    at 12.  At t = 43 J0 leaves and the pass over [J1, J2, J3] places J1 (position 0), steps over J2 (it
    slid into slot 0) and places J3 (position 2).  At t = 44 the pass places J2.  The iteration at t = 45
    finds every job placed.  TotalTime = 1000 * (43 + 43 + 44); three jobs run at t = 44."""
    c = E.rows(3)
    ref = check(c)
    exp = (np.array([0, 0, 0, 0]), np.array([0, 43, 44, 43]), np.array([43, 46, 47, 46]))
    for got in (ref, O.delay_run(c.free_c, c.free_m, *columns(c))):
        for x, y in zip(got[:3], exp):
            np.testing.assert_array_equal(x, y)
        assert {k: got[3][k] for k in STATS[:-1]} == dict(
            t_end=45, placed=4, moved_l1=3, placed_l1=3, peak_l1=3, peak_running=3, flags=0, l1_left=0,
            total_wait_ms=130000, jobs_count=4)
    assert ref[4]["place"] == [(43, 0, 3, 0), (43, 2, 3, 0), (44, 0, 1, 0)] and ref[4]["skip"] == [(43, 1)]


def test_hand_worked_odd_positions_and_deadlock():
    """rows(2, P=1): J1 asks for 701 cores and fits no node; J2, J3 are one-core 3 s jobs.  Moves at t = 10,
    11, 12.  At t = 43 the pass over [J1, J2, J3] fails J1, places J2 (position 1) and steps over J3; at 44
    it fails J1 and places J3 (position 1 of [J1, J3]).  J2 leaves at 46, J3 at 47: the passes at 45, 46 and 47
    fail J1, and at 47 nothing runs, queues or is still to come: J1 stays unplaced, flags = deadlock, t_end = 47.
    TotalTime = 1000 * (43 + 44 + 47)."""
    c = E.rows(2, 1)
    ref = check(c)
    none = 0xFFFFFFFF
    exp = (np.array([0, -1, 0, 0]), np.array([0, none, 43, 44]), np.array([43, none, 46, 47]))
    for got in (ref, O.delay_run(c.free_c, c.free_m, *columns(c))):
        for x, y in zip(got[:3], exp):
            np.testing.assert_array_equal(x, y)
        assert {k: got[3][k] for k in STATS[:-1]} == dict(
            t_end=47, placed=3, moved_l1=3, placed_l1=2, peak_l1=3, peak_running=2, flags=1, l1_left=1,
            total_wait_ms=134000, jobs_count=4)
    assert ref[4]["place"] == [(43, 1, 3, 0), (44, 1, 2, 0)] and ref[4]["skip"] == [(43, 2)]
    assert [p for p in ref[4]["pass"] if p[0] >= 43] == [(43, 3, 1), (44, 2, 0), (45, 1, 0), (46, 1, 1), (47, 1, 1)]


def test_hand_worked_retest_after_commit():
    """rows(5, gate_c=1, jd=7): node 0 has one core.  J0 holds it for 45 s; J1-J5 (1 core, 7 s) move to
    Level1 at t = 10-14.  At t = 45 the pass places J1 and steps over J2; J3-J5 fitted the grown node before
    the commit and fail after it.  At 46 J2 (untested) fails.  J1 leaves at 52: J2 is placed, J3 stepped
    over, and so on every 7 s: one placement per release, always at position 0."""
    c = E.rows(5, gate_c=1, jd=7)
    ref = check(c)
    np.testing.assert_array_equal(ref[1], [0, 45, 52, 59, 66, 73])
    assert ref[4]["place"] == [(45 + 7 * i, 0, 5 - i, 0) for i in range(5)]
    assert ref[4]["skip"] == [(45 + 7 * i, 1) for i in range(4)]
    assert ref[3]["t_end"] == 74 and ref[3]["total_wait_ms"] == 1000 * (45 + 52 + 59 + 66 + 73)


def test_grown_node_pass_model_on_the_edges():
    """tools/delay_g_model.py, the Python statement of the loop's pass (candidates from the grown nodes and
    the untested marks alone, the D6 skip on list positions), gives the oracle's placements on every edge
    workload: the algorithm holds there, so a GPU mismatch is the assembly's."""
    import importlib.util

    spec = importlib.util.spec_from_file_location("delay_g_model", os.path.join(os.path.dirname(GOLDEN), "..", "tools",
                                                                                "delay_g_model.py"))
    M = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(M)
    for fam, f in E.FAMILIES.items():
        for c in f():
            on, os_, _, _ = O.delay_run(c.free_c, c.free_m, *columns(c))
            gn, gs = M.model(list(c.free_c), list(c.free_m), [tuple(int(v) for v in j) for j in c.jobs])
            np.testing.assert_array_equal(np.array(gn, np.int32).reshape(-1), on, err_msg=c.name)
            np.testing.assert_array_equal(np.array(gs, np.uint32).reshape(-1), os_, err_msg=c.name)


def test_embedded_kats_keep_their_hand_derived_answers():
    """DKAT1-5 inside 256-node clusters (nodes with nothing free behind and, where no job asks for
    nothing, ahead of the real ones): the golden expectations, node indices shifted by the padding"""
    emb = E.embedded_kats(DKATS)
    assert len(emb) == 4 * 5 + 1
    for (c, en, es, ef), k in zip(emb, [k for k in DKATS for _ in range(5 if k["name"] != "DKAT2" else 1)]):
        for got in (delay_ref(c.free_c, c.free_m, *columns(c)), O.delay_run(c.free_c, c.free_m, *columns(c))):
            np.testing.assert_array_equal(got[0], en, err_msg=c.name)
            np.testing.assert_array_equal(got[1], es, err_msg=c.name)
            np.testing.assert_array_equal(got[2], ef, err_msg=c.name)
            for key, v in k["stats"].items():
                assert got[3][key] == v, (c.name, key)
