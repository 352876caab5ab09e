"""The slicing guarantee of a trading session (online mode of a DELAY trading system, DESIGN.md §14
"Trading sessions"), pinned on the CPU oracle (oracle/mcs_oracle_dtrade.c).  No GPU needed.

A session's mcs_run(h) executes every lock-step tick T < h.  Its reference is the batch run over ALL
the jobs the session ever receives, truncated after its last tick below h: at a tick T < h the
next-tick rule takes the minimum of the next sample tick, the trader due times and the next arrival, and
arrivals the session has not been given yet are >= h, so they neither create nor remove a tick below h.
With h = 1 (mod sample_period_s) a tick exists at h - 1 (every multiple of the sample period is one), so
t_max = h - 1 truncates the oracle exactly there.  The run over only the jobs with arrival < h makes the
same decisions but stops once those jobs are decided, which is why a finite horizon must not stop at
"every job decided" and why the subset run is not the reference of a slice."""
import numpy as np
import pytest

import oracle_ref as O
from kat_util import fuzz_workload
from mcs_amd import JobStreams

TRADE_F = ("t", "requester", "winner", "approvals", "policy", "cores", "mem", "time_s", "failed")
FOREIGN_F = ("requester", "responder", "node", "start", "finish", "c", "m")
NONE = 0xFFFFFFFF


def subset(streams, h):
    """the jobs of every cluster with arrival < h (a prefix of its stream) and their rows in `streams`"""
    parts, off, rows = [[], [], [], []], [0], []
    for k in range(len(streams.job_off) - 1):
        sl = streams.of(k)
        n = int((streams.arrival[sl] < h).sum())
        for i, f in enumerate(("arrival", "dur", "cores", "mem")):
            parts[i].append(getattr(streams, f)[sl][:n])
        rows.append(np.arange(sl.start, sl.start + n))
        off.append(off[-1] + n)
    return JobStreams(*[np.concatenate(p).astype(np.uint32) for p in parts], np.array(off, np.uint64)), \
        np.concatenate(rows).astype(np.int64)


def log_equal(got, want, fields, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for f in fields:
        np.testing.assert_array_equal(got[f], want[f], err_msg=f"{what}.{f}")


@pytest.fixture(scope="module", params=[(4, 900), (6, 1500)], ids=["seed4_J900", "seed6_J1500"])
def system(request):
    seed, J = request.param
    arrays, streams = fuzz_workload("w16s", seed, n_clusters=8, J=J, blocking=False)
    full = O.dtrade_run(arrays, streams)
    assert (full["trades"]["winner"] >= 0).sum() >= 50  # (75 and 134 winning trades)
    tf = int(full["t_final"])
    late = [5 * (tf // 10) + 1, 5 * (tf * 9 // 50) + 1]  # about 0.5 and 0.9 of the run
    assert 400 < late[0] < late[1] < tf
    return arrays, streams, full, list(range(1, 400, 5)) + late


def test_truncated_run_over_all_jobs_is_the_full_runs_prefix(system):
    arrays, streams, full, horizons = system
    for h in horizons:
        t = O.dtrade_run(arrays, streams, t_max=h - 1)
        dec = (full["start"] < h) & (full["node"] >= 0)
        for k in ("node", "start", "finish"):
            np.testing.assert_array_equal(t[k][dec], full[k][dec], err_msg=f"h={h} {k}")
        assert (t["node"][~dec] == -1).all() and (t["start"][~dec] == NONE).all(), h
        log_equal(t["trades"], full["trades"][full["trades"]["t"] < h], TRADE_F, f"h={h} trades")
        log_equal(t["foreign"], full["foreign"][full["foreign"]["start"] < h], FOREIGN_F, f"h={h} foreign")
        assert t["t_final"] == h - 1, h


def test_subset_run_differs_only_by_stopping_early(system):
    arrays, streams, full, horizons = system
    runs = []
    for h in horizons:
        sub, rows = subset(streams, h)
        runs.append((h, rows, O.dtrade_run(arrays, sub, t_max=h - 1)))
    # the difference exists: some horizon lies after the decision of the last job that arrived below it
    assert any(int(s["t_final"]) < h - 1 for h, _, s in runs)
    for h, rows, s in runs:
        tf = int(s["t_final"])
        assert tf <= h - 1
        for k in ("node", "start", "finish"):  # its jobs' rows: the full run's, where decided below h
            want = full[k][rows].copy()
            und = ~((full["start"][rows] < h) & (full["node"][rows] >= 0))
            want[und] = -1 if k == "node" else NONE
            np.testing.assert_array_equal(s[k], want, err_msg=f"h={h} {k}")
        if tf < h - 1:  # it stopped early: every job of it is decided, the logs end at its last tick
            assert (s["node"] >= 0).all(), h
        log_equal(s["trades"], full["trades"][full["trades"]["t"] <= tf], TRADE_F, f"h={h} trades")
        log_equal(s["foreign"], full["foreign"][full["foreign"]["start"] <= tf], FOREIGN_F, f"h={h} foreign")
