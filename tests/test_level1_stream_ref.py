"""The carry rule of Level1 samples on the start-stream cursors (mcs_stream_next_level1; DESIGN.md §14
"Level1 on the cursors"), pinned without a GPU.

A cursor opened with Level1 keeps, per batch of 256 rows, the batch's Level1 summary (the largest s among
the rows that move; frozen once the batch is final) and, per cluster, the scan bounds {lo, hi} of the
last sample it handed out.  A sample at t is computed from the rows in [lo, hi(t)) that lie in a batch at
or above first_live whose kept summary exceeds t.  Here that computation is restated in numpy (class
Cursor) over the oracle's DELAY run of tests/test_online_stream_ref.py's workload, truncated at a chain
of horizons as tests/test_online_series_ref.py truncates it, and compared at every second of every
[F, h) with level1_ref.replay / level1_ref.series over the whole run.  The horizons are picked from the
run so that the cases the rule has to survive occur, and each is asserted.

The same restatement counts the rows a call scans.  cost_case() computes that count for the cost case
of tests/test_gpu_level1_stream.py, and the cap of 3 R is asserted here first, on the rule alone."""
import functools

import numpy as np
import pytest

import level1_ref as R
import oracle_ref as O
from mcs_amd import JobStreams, replicate, uniform_cluster
from test_online_series_ref import truncate
from test_online_stream_ref import BATCH, W, workload

NONE = R.TIME_NONE
INF = 1 << 62  # level1_ref.closed_form's s of a row without a start


class Cursor:
    """What the engine keeps for one cluster between calls, and one call's samples from it."""

    def __init__(self, max_wait=W):
        self.W = max_wait
        self.lo = self.hi = 0
        self.summ, self.final, self.retired = {}, set(), set()
        self.first_live = 0
        self.last_len = None   # len of the last sample handed out
        self.seen = set()      # the cases met, by name
        self.walk_skips = 0

    def small_time(self, m, s, dur, head, last, t):
        """level1_small_time: the walk back from the last member to the head, batches that have left
        Level1 stepped over by their kept summary."""
        cur, run, j = int(dur[last]), 0, last - 1
        while j >= head:
            b = j // BATCH
            if self.summ[b] <= t:
                assert b != head // BATCH
                self.walk_skips += 1
                j = b * BATCH - 1
                continue
            if m[j] <= t < s[j]:
                if int(dur[j]) >= cur:
                    run, cur = run + 1, int(dur[j])
                else:
                    break
            j -= 1
        return int(dur[last]) if run % 2 == 0 else 0

    def call(self, arr, dur, cores, mem, n2, s2, f2, hor, ts, frontier):
        """The samples at the seconds ts (all below hor) from the session's rows as mcs_run(hor) left
        them; frontier: the stream's next sample second after the call.  Returns (samples, rows)."""
        J = len(arr)
        m, s = R.closed_form(arr, s2, self.W)
        assert (np.diff(m) >= 0).all()
        d = np.minimum(m, s)
        below = d < hor
        p = J if below.all() else int(np.argmin(below))  # d ascends: a prefix
        if p < J and (m[p:] >= hor).any():
            self.seen.add("past_d_prefix")
        assert (m[p + 1:] >= hor).all()  # h_j > d_{j-1} >= hor: no row behind the prefix is a candidate
        nb = (J + BATCH - 1) // BATCH
        for b in range(nb):
            rows = slice(b * BATCH, min(J, (b + 1) * BATCH))
            mv = s[rows] > m[rows]
            now = int(s[rows][mv].max()) if mv.any() else 0
            if b in self.final:
                assert self.summ[b] == now, "a final batch's kept summary went stale"
                continue
            if b < self.first_live:
                continue
            self.summ[b] = now  # stream_level1_summ_kernel: every batch prep loaded
            if (b + 1) * BATCH <= min(J, p) and (n2[rows] >= 0).all() and (f2[rows] != NONE).all():
                self.final.add(b)
        out, count = np.zeros(len(ts), R.LEVEL1), 0
        for k, t in enumerate(ts):
            assert t < hor
            hi = self.hi
            while hi < J and m[hi] <= t:
                hi += 1
            if k == 0 and ((m[self.hi:hi] == t) & (s[self.hi:hi] > t)).any():
                self.seen.add("m_at_F")
            if k == 0 and self.last_len and s[self.lo] == t:
                self.seen.add("head_starts_at_F")
            lo, members, skipped = self.lo, [], []
            if lo < hi:
                for b in range(max(lo // BATCH, self.first_live), (hi - 1) // BATCH + 1):
                    if self.summ[b] <= t:
                        skipped.append(b)
                        continue
                    x0, x1 = max(lo, b * BATCH), min(hi, (b + 1) * BATCH)
                    count += x1 - x0
                    members += [j for j in range(x0, x1) if m[j] <= t < s[j]]
                assert not any(b in self.retired and self.summ[b] > t for b in range(lo // BATCH, (hi - 1) // BATCH + 1))
            if skipped and members and s[members[0]] == INF and members[0] == lo and max(skipped) > lo // BATCH:
                self.seen.add("starved_pins_lo")
            if any(b in self.retired for b in skipped):
                self.seen.add("retired_inside")
            small = 0
            if members and len(members) % 20 == 0:
                small = self.small_time(m, s, dur, members[0], members[-1], t)
            out[k] = (len(members), sum(int(cores[j]) for j in members) & R.M32,
                      sum(int(mem[j]) for j in members) & R.M32, max((int(dur[j]) for j in members), default=0),
                      small, members[0] if members else NONE)
            if k == 0 and self.last_len == 0 and members:
                self.seen.add("empty_then_not")
            self.lo, self.hi, self.last_len = (members[0] if members else hi), hi, len(members)
        for b in self.final:  # stream_retire_kernel
            if int(f2[b * BATCH:(b + 1) * BATCH].astype(np.int64).max()) < frontier:
                self.retired.add(b)
        self.first_live = next((b for b in range(nb) if b not in self.retired), nb)
        return out, count


def follow(streams, node, start, fin, hs, t0=0, period=1, reps=None, T=None):
    """One Cursor per cluster over the chain of horizons hs, one call per horizon; with reps (the whole
    run's replays) every sample is compared.  Returns the cursors and the rows scanned per call."""
    C = len(streams.job_off) - 1
    curs, t, per_call = [Cursor() for _ in range(C)], t0, []
    for h in hs:
        ts = list(range(t, h, period))
        if not ts:
            per_call.append(0)
            continue
        sub, n2, s2, f2 = truncate(streams, node, start, fin, h)
        rows = 0
        for c in range(C):
            j2, js = sub.of(c), streams.of(c)
            got, cnt = curs[c].call(sub.arrival[j2].astype(np.int64), sub.dur[j2], sub.cores[j2], sub.mem[j2], n2[j2],
                                    s2[j2], f2[j2], h, ts, ts[-1] + period)
            rows += cnt
            if reps is not None:
                want = R.series(reps[c], streams.dur[js], streams.cores[js], streams.mem[js], ts[0], period, len(ts))
                assert got.tobytes() == want.tobytes(), f"cluster {c} h {h} samples {ts[0]}..{ts[-1]}"
        per_call.append(rows)
        t = ts[-1] + period
    return curs, per_call


@pytest.fixture(scope="module")
def full():
    arrays, streams = workload("DELAY")
    node, start, fin, stats = O.delay_run_batch(arrays, streams, n_threads=4, max_wait_s=W)
    assert int((node < 0).sum()) == 1
    T = int(stats["t_end"].max()) + 3
    st = np.where(node >= 0, start, NONE)
    reps = [R.replay(streams.arrival[streams.of(c)], st[streams.of(c)], W, T) for c in range(2)]
    return streams, node, start, fin, T, reps


def picked_horizons(streams, start, T, reps):
    """A chain up to T: every 37 s, and the seconds at which a call has to begin for the cases."""
    hs = set(range(40, T, 37)) | {T}
    lists = reps[0]["lists"]
    st0 = start[streams.of(0)].astype(np.int64)
    hs.add(next(t for t in range(100, T) if not lists[t - 1] and lists[t]))                      # empty, then not
    hs.add(next(t for t in range(100, T) if lists[t - 1] and st0[lists[t - 1][0]] == t))          # the head starts at F
    m, s = R.closed_form(streams.arrival[streams.of(0)], st0, W)
    hs.add(int(next(m[j] for j in range(200, len(m)) if s[j] > m[j])))                            # m == F
    return sorted(hs)


@pytest.mark.parametrize("open_at", [0, 9])
def test_carried_bounds_and_kept_summaries_give_the_whole_runs_lists(full, open_at):
    streams, node, start, fin, T, reps = full
    hs = picked_horizons(streams, start, T, reps)
    t0 = hs[open_at - 1] if open_at else 0  # opened mid-session: the first call catches up from row 0
    curs, _ = follow(streams, node, start, fin, hs[open_at:], t0, 1, reps)
    seen = curs[0].seen | curs[1].seen
    need = {"starved_pins_lo", "retired_inside", "past_d_prefix"}
    if not open_at:
        need |= {"empty_then_not", "head_starts_at_F", "m_at_F"}
    assert need <= seen, f"the inputs do not exercise {sorted(need - seen)}"
    assert "starved_pins_lo" in curs[1].seen and curs[1].lo == 600  # the row that starves for good
    assert max(len(x) for rep in reps for x in rep["lists"]) < 20   # (the walk-back has its own case below)


def walk_system():
    """One 32-core node.  Row 0 holds one core for 2000 s, so a whole-node job fits nowhere before then:
    rows 1-10 and 612-621 ask for the whole node and wait in Level1, the 601 one-core jobs between them
    are placed as they arrive.  Batch 1 (rows 256-511) never holds a member: its summary is 0, and the
    walk back from row 621 to the head, row 1, steps over it while the list has 20 entries."""
    arrays = replicate(uniform_cluster(1, cores=32, memory=24000), 1)
    n = 622
    arr = np.arange(n, dtype=np.int64)
    dur, cores = np.ones(n, np.int64), np.ones(n, np.int64)
    dur[0] = 2000
    whole = np.r_[1:11, 612:622]
    cores[whole] = 32
    # durations that never rise from row 2 on: the run of falls the walk follows reaches back over batch 1
    dur[whole] = [1, 9, 9, 9, 9, 8, 8, 8, 8, 8, 7, 7, 6, 6, 5, 5, 4, 4, 3, 3]
    s = JobStreams(*(x.astype(np.uint32) for x in (arr, dur, cores, np.ones(n, np.int64))), np.array([0, n], np.uint64))
    return arrays, s


def test_walk_back_crosses_a_skipped_batch():
    arrays, streams = walk_system()
    node, start, fin, stats = O.delay_run_batch(arrays, streams, n_threads=1, max_wait_s=W)
    assert (node >= 0).all()
    T = int(stats["t_end"].max()) + 3
    rep = R.replay(streams.arrival, start, W, T)
    lens = [len(x) for x in rep["lists"]]
    assert max(lens) == 20 and lens.count(20) > 100
    hs = [300, 640, 700, 1500, 1999, 2003, 2040, T]
    curs, _ = follow(streams, node, start, fin, hs, 0, 1, [rep])
    assert curs[0].walk_skips > 100
    want = R.series(rep, streams.dur, streams.cores, streams.mem, 0, 1, T)
    mult = (want["len"] > 0) & (want["len"] % 20 == 0)
    assert mult.sum() > 100 and (want["small_time_s"][mult] == 3).any()  # 18 falls, then the rise at row 1


# ---- the cost case of tests/test_gpu_level1_stream.py ------------------------------------------------

COST_JOBS, COST_CLUSTERS, COST_SLICES, COST_PERIOD = 8000, 4, 40, 5


def cost_workload(seed):
    arrays = replicate(uniform_cluster(5, cores=32, memory=24000), COST_CLUSTERS)
    rng = np.random.default_rng(seed)
    parts = []
    for _ in range(COST_CLUSTERS):
        arr = np.cumsum(rng.poisson(1.0, COST_JOBS))
        dur, cores, mem = rng.integers(0, 20, COST_JOBS), rng.integers(0, 25, COST_JOBS), rng.integers(0, 12001, COST_JOBS)
        cores[45::90] = 32
        parts.append((arr, dur, cores, mem))
    off = (np.arange(COST_CLUSTERS + 1) * COST_JOBS).astype(np.uint64)
    return arrays, JobStreams(*(np.concatenate([p[f] for p in parts]).astype(np.uint32) for f in range(4)), off)


@functools.lru_cache(maxsize=None)
def cost_case(seed):
    """(arrays, streams, horizons, rows the rule scans per call, facts about the run)."""
    arrays, streams = cost_workload(seed)
    node, start, fin, _ = O.delay_run_batch(arrays, streams, n_threads=4, max_wait_s=W)
    top = int(streams.arrival.max()) + 1
    hs = [top * k // COST_SLICES for k in range(1, COST_SLICES + 1)]
    curs, per_call = follow(streams, node, start, fin, hs, 0, COST_PERIOD)
    m_s = [R.closed_form(streams.arrival[streams.of(c)], np.where(node >= 0, start, NONE)[streams.of(c)], W)
           for c in range(COST_CLUSTERS)]
    moved = sum(int((s > m).sum()) for m, s in m_s)
    return arrays, streams, hs, per_call, dict(unplaced=int((node < 0).sum()), moved=moved)


@pytest.mark.parametrize("seed", [7, 8])
def test_cost_case_stays_below_the_cap_under_the_rule_alone(seed):
    _, streams, hs, per_call, facts = cost_case(seed)
    rows = int(streams.job_off[-1])
    assert len(per_call) == COST_SLICES and facts["unplaced"] == 0
    assert facts["moved"] > rows // 5  # Level1 is busy: more than a fifth of the jobs move
    print(f"seed {seed}: the rule scans {sum(per_call)} rows = {sum(per_call) / rows:.2f} R over {COST_SLICES} calls")
    assert 0 < sum(per_call) <= 3 * rows
