"""The guarantee of mcs_online_state_series (include/mcs.h), pinned without a GPU.

After mcs_run(h) an online session knows every start below h and every job that arrived below h; the
other starts read "never placed".  A sample at a second t < h taken from that truncated knowledge must
equal the sample taken from the whole run.  Here the whole run is the oracle's DELAY run of seeded
small hot clusters; the truncation replaces every start >= h by "never placed" and drops the arrivals
>= h.  The wait statistics come from tests/wait_ref.py's replay of the Go loop, the state samples from
the brute-force series_ref of tests/test_gpu_state_series.py (a numpy restatement per sample).

Each case first asserts that it is not vacuous: there are undecided jobs that arrived below h, and
Level1 placements with a D6 skip both below and at or above h."""
import numpy as np
import pytest

import oracle_ref as O
import wait_ref as R
from mcs_amd import JobStreams
from test_gpu_state_series import assert_samples_equal, series_ref
from test_gpu_wait_series import hot_clusters

W = 10
SIZES = [300, 257, 120, 300]


@pytest.fixture(scope="module")
def full():
    arrays, streams = hot_clusters(SIZES, 0x4F4E4C, nodes=[3, 2, 4, 5])
    node, start, fin, stats = O.delay_run_batch(arrays, streams, n_threads=4, max_wait_s=W)
    T = int(stats["t_end"].max()) + 3
    reps = [R.replay(streams.arrival[streams.of(c)], start[streams.of(c)], W, T) for c in range(len(SIZES))]
    return arrays, streams, node, start, fin, T, reps


def truncate(streams, node, start, fin, h):
    """What the session holds after mcs_run(h): the jobs that arrived below h, with the starts below h."""
    keep = streams.arrival < h
    und = start >= h  # (a never-placed job reads MCS_TIME_NONE already)
    n2 = np.where(und, np.int32(-1), node)[keep]
    s2 = np.where(und, np.uint32(R.TIME_NONE), start)[keep]
    f2 = np.where(und, np.uint32(R.TIME_NONE), fin)[keep]
    off = np.concatenate([[0], np.cumsum([int(keep[streams.of(c)].sum()) for c in range(len(streams.job_off) - 1)])])
    sub = JobStreams(*(getattr(streams, f)[keep] for f in ("arrival", "dur", "cores", "mem")), off.astype(np.uint64))
    return sub, n2, s2, f2


def horizons(streams, start, node):
    """Seconds spread over the busy part of the run, one of them a start second + 1 (a job that starts
    at h - 1 is decided) and one an arrival second + 1."""
    placed = start[node >= 0].astype(np.int64)
    hs = {int(np.percentile(placed, p)) for p in (20, 45, 70)}
    hs.add(int(np.sort(placed)[len(placed) // 2]) + 1)
    hs.add(int(np.sort(streams.arrival)[len(streams.arrival) // 2]) + 1)
    return sorted(hs)


def test_the_cases_are_not_vacuous_and_wait_samples_below_the_horizon_are_final(full):
    arrays, streams, node, start, fin, T, reps = full
    hs = horizons(streams, start, node)
    assert len(hs) >= 4 and 0 < hs[0] and hs[-1] < T
    for h in hs:
        sub, n2, s2, f2 = truncate(streams, node, start, fin, h)
        # first: the case is not vacuous
        undecided = int(((streams.arrival < h) & (start >= h)).sum())
        below = sum(1 for rep in reps for _, t in rep["skips"] if t < h)
        above = sum(1 for rep in reps for _, t in rep["skips"] if t >= h)
        assert undecided > 0, f"h {h}: every job that arrived below the horizon is decided"
        assert below > 0 and above > 0, f"h {h}: D6 skips below {below}, at or above {above}"
        for c in range(len(SIZES)):
            js, j2 = streams.of(c), sub.of(c)
            cut = R.replay(sub.arrival[j2], s2[j2], W, h - 1)
            np.testing.assert_array_equal(cut["total_ms"], reps[c]["total_ms"][:h], err_msg=f"h {h} cluster {c}")
            np.testing.assert_array_equal(cut["count"], reps[c]["count"][:h], err_msg=f"h {h} cluster {c}")
            assert [x for x in cut["skips"]] == [x for x in reps[c]["skips"] if x[1] < h]


def test_state_samples_below_the_horizon_are_final(full):
    arrays, streams, node, start, fin, T, _ = full
    hs = horizons(streams, start, node)
    want = series_ref(arrays, streams, node, start, fin, 0, 1, hs[-1])
    assert want["running"].max() > 0 and want["queued"].max() > 0
    for h in hs:
        sub, n2, s2, f2 = truncate(streams, node, start, fin, h)
        und = (streams.arrival < h) & (start >= h)
        assert und.any()
        # an undecided job is queued from its arrival on and never running below h
        assert (want["queued"][:, h - 1].sum()) >= int((und & (streams.arrival <= h - 1)).sum()) > 0
        got = series_ref(arrays, sub, n2, s2, f2, 0, 1, h)
        assert_samples_equal(got, want[:, :h], f"h {h}")


def test_a_sample_at_the_horizon_is_not_final(full):
    """The rule is sharp: at t = h some case differs (a job that starts at h reads undecided)."""
    arrays, streams, node, start, fin, T, _ = full
    differs = False
    for h in horizons(streams, start, node):
        sub, n2, s2, f2 = truncate(streams, node, start, fin, h)
        # (arrivals at h are dropped as well: compare running, which they cannot touch at h)
        got = series_ref(arrays, sub, n2, s2, f2, h, 1, 1)
        want = series_ref(arrays, streams, node, start, fin, h, 1, 1)
        differs |= bool((got["running"] != want["running"]).any())
    assert differs
