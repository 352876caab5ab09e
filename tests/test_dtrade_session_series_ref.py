"""The guarantee of mcs_trade_session_state_series and mcs_trade_session_level1_series
(include/mcs_trade.h, DESIGN.md §14 "The Start stream of a trading session"), pinned on the CPU oracle
alone.  No GPU needed.

After mcs_run(h) a trading session holds what the batch run over ALL the jobs it ever receives holds
after that run's last tick below h (tests/test_dtrade_session_ref.py): every start below h, the Foreign
records logged below h and the virtual nodes received below h; every other own row reads undecided.
With h = 1 (mod sample_period_s) the oracle's run with t_max = h - 1 is that state.  A sample at a
second t < h taken from it must equal, bit for bit, the sample taken from the whole run, for the
ClusterState record (tests/dtrade_state_ref.py), the wait statistics (tests/wait_ref.py) and the Level1
samples (tests/level1_ref.py), at every second below h.  The host references walk every second of
every cluster in Python, so ("big", 8, 800), whose run is 12426 s long, is compared at every second
of the 600 s below each h and at the reference cadence (every 5th second) before that, and its wait
and Level1 replays cover the two clusters the GPU suite replays for the same reason (0 and 5).

Each case first asserts that it exercises the four pieces of the derivation, below an h it uses:
  - an undecided job that arrived below h (it must read "queued for good, never running");
  - a Foreign record with start_s = h - 1 (logged by the last executed tick; it holds only above h - 1);
  - a virtual node received at or after h (absent in the session, present in the whole run, term +0);
  - a Foreign job that holds, below h, a virtual row of its responder.
("small", 4, 120) with the default seed has no Foreign job on a virtual row at all; seed 2 of the same
shape has two, so it runs as a third case, and the default seed asserts the other three."""
import numpy as np
import pytest

import dtrade_state_ref as D
import level1_ref as L1
import oracle_ref as O
import wait_ref as W
from kat_util import seeded_workload

MAX_WAIT = 10  # the engine's default max_wait_s, which the oracle's DELAY trading run uses
PERIOD = 5     # sample_period_s

# (kind, clusters, jobs, seed or None, horizons, a Foreign job holds a virtual row below one of them,
#  every second of every cluster)
CASES = [
    ("small", 4, 120, None, (51, 61, 806, 3861, 4111, 4301), False, True),
    ("small", 4, 120, 2, (51, 3971, 4021), True, True),
    ("big", 8, 800, None, (121, 10841, 12371), True, False),
]


def ranges(h, dense):
    """(t0, period, n) covering the seconds below h that a case compares"""
    if dense or h <= 600:
        return [(0, 1, h)]
    return [(0, PERIOD, (h - 600 + PERIOD - 1) // PERIOD), (h - 600, 1, 600)]


@pytest.fixture(scope="module", params=CASES, ids=["small", "small_seed2", "big"])
def case(request):
    kind, C, J, seed, hs, vrow, dense = request.param
    arrays, streams, _ = seeded_workload(kind, C, J) if seed is None else seeded_workload(kind, C, J, seed=seed)
    full = O.dtrade_run(arrays, streams)
    assert all(h % PERIOD == 1 and 0 < h <= int(full["t_final"]) for h in hs)
    runs = {h: O.dtrade_run(arrays, streams, t_max=h - 1) for h in hs}
    return arrays, streams, full, runs, vrow, dense


def test_the_cases_exercise_the_derivation(case):
    arrays, streams, full, runs, vrow, _ = case
    nphys = np.diff(arrays.node_off)
    f = full["foreign"]
    won = full["trades"][full["trades"]["winner"] >= 0]
    seen = dict(undecided=False, foreign_at_h1=False, vnode_later=False, foreign_on_vrow=False)
    for h, cut in runs.items():
        assert cut["t_final"] == h - 1
        und = (streams.arrival < h) & (cut["node"] < 0)
        seen["undecided"] |= bool(und.any())
        seen["foreign_at_h1"] |= bool((cut["foreign"]["start"] == h - 1).any())
        later = [len(a) > len(b) for a, b in zip(full["vnodes"], cut["vnodes"])]
        seen["vnode_later"] |= any(later) and bool((won["t"] >= h - 1).any())
        fc = cut["foreign"]
        on_v = (fc["node"] >= nphys[fc["responder"]]) & (fc["start"] + 1 < np.minimum(fc["finish"], h))
        seen["foreign_on_vrow"] |= bool(on_v.any())
        # what the session holds: the whole run's rows where decided below h, its log below h
        dec = (full["start"] < h) & (full["node"] >= 0)
        np.testing.assert_array_equal(cut["node"][dec], full["node"][dec])
        assert (cut["node"][~dec] == -1).all() and (cut["start"][~dec] == W.TIME_NONE).all()
        assert len(cut["foreign"]) == int((f["start"] < h).sum())
    want = dict(undecided=True, foreign_at_h1=True, vnode_later=True, foreign_on_vrow=vrow)
    assert seen == want, seen


def test_state_samples_below_the_horizon_are_final(case):
    arrays, streams, full, runs, _, dense = case
    busy = False
    for h, cut in runs.items():
        for t0, period, n in ranges(h, dense):
            want = D.series_ref(arrays, streams, full, t0, period, n)
            got = D.series_ref(arrays, streams, cut, t0, period, n)
            busy |= want["running"].max() > 0 and want["queued"].max() > 0
            bad = np.nonzero((D.bits(got) != D.bits(want)).any(-1))
            assert len(bad[0]) == 0, f"h {h}: first (cluster, k) of t0 {t0} period {period} " \
                                     f"{[(int(c), int(k)) for c, k in zip(*bad)][:3]}"
    assert busy


def test_a_sample_at_the_horizon_is_not_final(case):
    """The rule is sharp: at t = h some horizon's sample differs (a start at h reads undecided)."""
    arrays, streams, full, runs, _, _ = case
    differs = False
    for h, cut in runs.items():
        got = D.series_ref(arrays, streams, cut, h, 1, 1)
        want = D.series_ref(arrays, streams, full, h, 1, 1)
        differs |= bool((D.bits(got) != D.bits(want)).any())
    assert differs


def test_wait_and_level1_samples_below_the_horizon_are_final(case):
    arrays, streams, full, runs, _, dense = case
    hmax = max(runs)
    for c in range(arrays.n_clusters) if dense else (0, 5):
        js = streams.of(c)
        arr, dur, cores, mem = (getattr(streams, k)[js] for k in ("arrival", "dur", "cores", "mem"))
        wrep = W.replay(arr, full["start"][js], MAX_WAIT, hmax - 1)
        lrep = L1.replay(arr, full["start"][js], MAX_WAIT, hmax - 1)
        lwant = L1.series(lrep, dur, cores, mem, 0, 1, hmax)
        for h, cut in runs.items():
            wcut = W.replay(arr, cut["start"][js], MAX_WAIT, h - 1)
            np.testing.assert_array_equal(wcut["total_ms"], wrep["total_ms"][:h], err_msg=f"h {h} cluster {c}")
            np.testing.assert_array_equal(wcut["count"], wrep["count"][:h], err_msg=f"h {h} cluster {c}")
            lcut = L1.replay(arr, cut["start"][js], MAX_WAIT, h - 1)
            lgot = L1.series(lcut, dur, cores, mem, 0, 1, h)
            assert lgot.tobytes() == lwant[:h].tobytes(), f"h {h} cluster {c}"
