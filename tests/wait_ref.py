"""Time-resolved WaitTime of a DELAY run — TEST INFRASTRUCTURE ONLY.

The CPU oracle reports WaitTime once, at t_end.  The references here restate Scheduler.Delay
(pkg/scheduler/scheduler.go:298-369) with the "/delay" handler (pkg/scheduler/server.go:67-74) as the
loop is written, and record WaitTime.TotalTime and WaitTime.JobsCount after every iteration.  Serialized
semantics SDELAY: at second t, releases, then arrivals <= t, then the Level1 pass,
then the Level0 head.

    replay(arrival, start, W, T)   the loop driven by known start seconds: an examined entry is placed
                                   at t iff start == t (MCS_TIME_NONE: never)
    literal(nodes, jobs, W, T)     the same loop with real first-fit tests (tiny cases)

Neither uses the closed form of mcs_wait_time_series: they keep Level0, Level1 and the
JobsMap and walk every second.  replay_no_gate and replay_no_skip are two WRONG restatements, kept so
that a test can show that its inputs tell them from the right one.
"""
from __future__ import annotations

import numpy as np

TIME_NONE = 0xFFFFFFFF


def _loop(arrival, W, T, decide, tick=None, gate=True, skip=True):
    """Iterations t = 0..T.  decide(j, t) -> True when ScheduleJob places job j at t (and commits).
    Returns a dict: total_ms and count after every second (int64 arrays of T + 1), the skip events
    (job, t) of D6, the longest run of consecutive seconds at which one job was skipped, and the
    queues left."""
    J = len(arrival)
    arrival = [int(a) for a in arrival]
    level0, level1, jobs_map = [], [], {}
    total = count = nxt = 0
    totals, counts = np.zeros(T + 1, np.int64), np.zeros(T + 1, np.int64)
    skips, run, longest = [], {}, 0

    def touch(j, t):  # scheduler.go:309-312 / 338-341
        nonlocal total
        total -= jobs_map.get(j, 0)
        jobs_map[j] = 1000 * (t - arrival[j])  # time.Since(WaitTime).Milliseconds(), whole seconds
        total += jobs_map[j]

    for t in range(T + 1):
        if tick is not None:
            tick(t)  # Node.RunJob completions (cluster.go:153-157) precede the decisions
        while nxt < J and arrival[nxt] <= t:  # server.go:67-74
            level0.append(nxt)
            jobs_map[nxt] = 0
            count += 1
            nxt += 1
        i = 0
        while i < len(level1):  # for i := 0; i < len(sched.Level1); i++ (:305)
            j = level1[i]
            ok = decide(j, t)  # :307
            touch(j, t)
            if ok:
                del jobs_map[j]  # :316
                del level1[i]    # :319 — the next entry slides into slot i
                if skip:
                    if i < len(level1):  # ... and i++ steps over it (D6)
                        s = level1[i]
                        skips.append((s, t))
                        prev = run.get(s)
                        n = prev[1] + 1 if prev and prev[0] == t - 1 else 1
                        run[s] = (t, n)
                        longest = max(longest, n)
                else:
                    i -= 1
            i += 1
        if level0:
            if not gate:  # WRONG on purpose: every queued job counts, not only the head
                for j in level0[1:]:
                    touch(j, t)
            j = level0[0]
            ok = decide(j, t)  # :335
            touch(j, t)
            if ok:
                del jobs_map[j]  # :346
                level0.pop(0)
            elif t - arrival[j] >= W:  # :353
                level1.append(j)
                level0.pop(0)
        totals[t], counts[t] = total, count
    return dict(total_ms=totals, count=counts, skips=skips, longest_skip_run=longest, level0=level0,
                level1=level1, admitted=nxt)


def replay(arrival, start, W, T, gate=True, skip=True):
    """The Go loop over known start seconds.  A skipped entry must not start at that second (it was
    not examined): asserted."""
    start = [int(s) for s in start]

    def decide(j, t):
        assert start[j] >= t, f"job {j} is still queued at {t} but started at {start[j]}"
        return start[j] == t

    out = _loop(arrival, int(W), int(T), decide, gate=gate, skip=skip)
    for j, t in out["skips"]:
        assert start[j] != t, f"job {j} was skipped at {t}, yet it started then"
    return out


def replay_no_gate(arrival, start, W, T):
    """WRONG: every arrived pending job counts t - arrival, as if the whole of Level0 were examined."""
    return replay(arrival, start, W, T, gate=False)


def replay_no_skip(arrival, start, W, T):
    """WRONG: the Level1 pass with the i-- the reference lacks, so no entry is stepped over.  (Only the
    statistics differ: the placements are the given ones.)"""
    start = [int(s) for s in start]
    return _loop(arrival, int(W), int(T), lambda j, t: start[j] == t, skip=False)


def steady_after(out, arrival, start, T):
    """True when, after iteration T of `out`, the loop has reached its fixed point: every job has
    arrived, Level0 is empty and nothing queued is ever placed.  Every later second then examines
    each Level1 entry and places none (no removal, so no D6 skip): TotalTime grows by
    1000 * len(Level1) per second and JobsCount stays."""
    return out["admitted"] == len(arrival) and not out["level0"] and \
        all(int(start[j]) == TIME_NONE for j in out["level1"])


def literal(nodes, jobs, W, T):
    """The loop with ScheduleJob as written (first fit with >=, scheduler.go:127-139; commit of
    Node.RunJob done at once, D2).  nodes: (free_cores, free_mem) per node; jobs: arrays (arrival,
    dur, cores, mem).  Returns _loop's dict plus `start` (TIME_NONE: not placed by T)."""
    arrival, dur, cores, mem = ([int(x) for x in v] for v in jobs)
    free = [[int(c), int(m)] for c, m in nodes]
    running = []  # (finish, node, cores, mem)
    start = [TIME_NONE] * len(arrival)

    def tick(t):
        for r in [r for r in running if r[0] <= t]:
            free[r[1]][0] += r[2]
            free[r[1]][1] += r[3]
            running.remove(r)

    def decide(j, t):
        for k, f in enumerate(free):
            if f[0] >= cores[j] and f[1] >= mem[j]:
                start[j] = t
                if dur[j] > 0:  # a zero-duration RunJob releases before the next scheduler step
                    f[0] -= cores[j]
                    f[1] -= mem[j]
                    running.append((t + dur[j], k, cores[j], mem[j]))
                return True
        return False

    out = _loop(arrival, int(W), int(T), decide, tick=tick)
    out["start"] = np.array(start, np.uint32)
    return out


def samples(out, t0, period, n, tail=None):
    """(total_ms, count) of replay's result at t0 + k * period, k < n.  tail = (T, n_left): past
    replay's last second T the fixed point of steady_after holds with n_left Level1 entries."""
    tot, cnt = np.zeros(n, np.int64), np.zeros(n, np.int64)
    T = len(out["total_ms"]) - 1
    for k in range(n):
        t = t0 + k * period
        if t <= T:
            tot[k], cnt[k] = out["total_ms"][t], out["count"][t]
        else:
            assert tail is not None and tail[0] == T, "sample past the replayed seconds"
            tot[k], cnt[k] = int(out["total_ms"][T]) + 1000 * (t - T) * tail[1], out["count"][T]
    return tot, cnt


def average(total_ms, count):
    """WaitTime.GetAverage() (scheduler.go:56-63): float64(TotalTime) / float64(JobsCount), 0 for no jobs."""
    total_ms, count = np.asarray(total_ms, np.int64), np.asarray(count, np.int64)
    out = np.zeros(total_ms.shape, np.float64)
    nz = count != 0
    out[nz] = total_ms[nz].astype(np.float64) / count[nz].astype(np.float64)
    return out
