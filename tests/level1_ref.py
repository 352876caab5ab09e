"""The Level1 list of a DELAY run, second by second, and the two contract sizes the trader takes
from it — TEST INFRASTRUCTURE ONLY.

ProvideJobs (pkg/scheduler/trader_server.go:69-94, over GetLevel1, scheduler.go:204-214) hands the
trader sched.Level1 in batches of 20, the last one padded with zero jobs (D9), and the trader sizes
its contract from that list (calculateFastNodeSize / calculateSmallNodeSize,
pkg/trader/scheduler_client.go:126-289).  The reference here restates Scheduler.Delay
(scheduler.go:298-369) with the "/delay" handler (server.go:67-74) as the loop is written, driven by
known start seconds like wait_ref.replay, and keeps a copy of Level1 after every iteration.
Serialized semantics SDELAY: at second t the arrivals <= t, then the Level1 pass
(the removal without i--, D6), then the Level0 head.

    replay(arrival, start, W, T)     Level1 after the iterations t = 0..T (lists of stream rows)
    contract_fast / contract_small   the literal recurrences over the padded list
    sample(members, dur, cores, mem) one mcs_level1_sample as a tuple
    series(...)                      the samples of one cluster as a LEVEL1 structured array

Nothing here uses the closed form of mcs_level1_series: the lists are kept and every
second is walked.
"""
from __future__ import annotations

import numpy as np

TIME_NONE = 0xFFFFFFFF
BATCH = 20  # jobs per ProvideJobs message (trader_server.go:76)
M32 = 0xFFFFFFFF

LEVEL1 = np.dtype([("len", "<u4"), ("cores", "<u4"), ("mem", "<u4"), ("fast_time_s", "<u4"),
                   ("small_time_s", "<u4"), ("head", "<u4")])


def replay(arrival, start, W, T):
    """The Go loop over known start seconds: an examined entry is placed at t iff start == t.
    Returns a dict: lists[t] = Level1 after iteration t (a tuple of rows, list order), moved = every
    row that ever entered Level1 (in order), level0 = the queue left after T, admitted."""
    J = len(arrival)
    arrival = [int(a) for a in arrival]
    start = [int(s) for s in start]
    W, T = int(W), int(T)
    level0, level1, moved, lists = [], [], [], []
    nxt = 0
    for t in range(T + 1):
        while nxt < J and arrival[nxt] <= t:  # server.go:67-74
            level0.append(nxt)
            nxt += 1
        i = 0
        while i < len(level1):  # for i := 0; i < len(sched.Level1); i++ (:305)
            j = level1[i]
            assert start[j] >= t, f"job {j} is still in Level1 at {t} but started at {start[j]}"
            if start[j] == t:
                del level1[i]  # :319 — the next entry slides into slot i and i++ steps over it (D6)
            i += 1
        if level0:
            j = level0[0]
            assert start[j] >= t, f"job {j} heads Level0 at {t} but started at {start[j]}"
            if start[j] == t:  # :335
                level0.pop(0)
            elif t - arrival[j] >= W:  # :353
                level1.append(j)
                moved.append(j)
                level0.pop(0)
        lists.append(tuple(level1))
    return dict(lists=lists, moved=moved, level0=level0, admitted=nxt)


def steady_after(rep, arrival, start):
    """True when the loop has reached its fixed point after replay's last second: every job has
    arrived, Level0 is empty and no Level1 entry is ever placed.  Level1 then never changes."""
    return rep["admitted"] == len(arrival) and not rep["level0"] and \
        all(int(start[j]) == TIME_NONE for j in rep["lists"][-1])


def padded(jobs):
    """ProvideJobs' messages joined: the list, its last batch filled with zero jobs (D9).  An empty
    list sends nothing."""
    jobs = list(jobs)
    return jobs + [(0, 0, 0)] * (-len(jobs) % BATCH)


def _i32(x):
    x &= M32
    return x - (1 << 32) if x >> 31 else x


def contract_fast(jobs):
    """calculateFastNodeSize (scheduler_client.go:126-185) over (cores, mem, dur_s) jobs: uint32 sums
    and the longest duration.  MaximimumCoreCost and MemoryCost are never set and Budget is -1
    (trader.go:34-35,53), so the price is 0 and the budget never ends the loop.
    Returns (cores, mem, time_s)."""
    cc = cm = ct = 0
    for c, m, d in padded(jobs):
        ct = d if d > ct else ct  # :144-148
        cc = (cc + c) & M32       # :150
        cm = (cm + m) & M32
    return cc, cm, ct


def contract_small(jobs):
    """calculateSmallNodeSize (scheduler_client.go:201-289): atTime only ever holds {0, 0, 0}, so each
    job yields one candidate: cores and memory grow by the job's in int32 arithmetic (:238-250), and
    the time is the job's duration if the contract's time so far is below it, else 0 (:263-265).
    Returns (cores, mem, time_s)."""
    cc = cm = ct = 0
    for c, m, d in padded(jobs):
        dc, dm = _i32(0 - c), _i32(0 - m)  # currState.cores - int32(CoresNeeded), currState = {0, 0}
        if dc < 0:
            cc = _i32(cc - dc)
        if dm < 0:
            cm = _i32(cm - dm)
        ct = d if ct < d else 0
    return cc & M32, cm & M32, ct


def sample(members, dur, cores, mem):
    """mcs_level1_sample of one list (rows of the cluster's stream, list order)."""
    jobs = [(int(cores[j]), int(mem[j]), int(dur[j])) for j in members]
    fc, fm, ft = contract_fast(jobs)
    sc, sm, st = contract_small(jobs)
    assert (fc, fm) == (sc, sm), "the two sizings add the same requests (every one below 2^31)"
    return len(jobs), fc, fm, ft, st, (members[0] if members else TIME_NONE)


def series(rep, dur, cores, mem, t0, period, n, steady=False):
    """The samples t0 + k * period, k < n, of replay's result.  steady: seconds past replay's last
    one read its last list (the caller has asserted steady_after)."""
    out = np.zeros(n, LEVEL1)
    T = len(rep["lists"]) - 1
    memo = {}
    for k in range(n):
        t = t0 + k * period
        if t > T:
            assert steady, "sample past the replayed seconds"
            t = T
        members = rep["lists"][t]
        if members not in memo:
            memo[members] = sample(members, dur, cores, mem)
        out[k] = memo[members]
    return out


def closed_form(arrival, start, W):
    """(m, s) per job as int arrays (s = 2^62 for none), the membership rule of DESIGN.md §13:
    Level1(t) = { j : m_j <= t < s_j }.  Only the CPU tests compare it with replay; no GPU test's
    expectation comes from it."""
    J = len(arrival)
    m, s = np.zeros(J, np.int64), np.zeros(J, np.int64)
    d = -1
    for j in range(J):
        a = int(arrival[j])
        sj = int(start[j]) if int(start[j]) != TIME_NONE else 1 << 62
        h = max(a, d + 1)
        mj = max(h, a + int(W))
        m[j], s[j] = mj, sj
        d = min(sj, mj)
    return m, s
