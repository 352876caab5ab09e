"""A plain per-second restatement of Scheduler.Delay under SDELAY, with a trace.
TEST INFRASTRUCTURE ONLY: the third voice beside oracle/mcs_oracle_delay.c and the GPU kernels, written
from the Go loop's semantics (pkg/scheduler/scheduler.go:298-369) and kept small enough to read in one go.

One Delay iteration at second t: releases (finish <= t, D3) and arrivals (<= t, JobsMap = 0,
JobsCount++); the Level1 pass in list order, a placed entry removed with no i-- (D6: the entry sliding
into its slot is not examined); the Level0 head, moved to the Level1 tail once it has waited max_wait_s;
Sleep(1 s).  An examined job's JobsMap entry becomes 1000 * (t - arrival); TotalTime keeps the last
value of every job.  The run ends at the top of the iteration that finds every job placed, or after an
iteration that changed nothing with nothing running, Level0 empty and every job arrived (the Level1
jobs left are retried forever: unplaced, flags = 1).

The one shortcut: after an iteration that changed nothing, the seconds before the next release, the next
arrival and the head's move repeat it exactly, so they are taken at once (their examinations stamp the
last of them).  jump=False runs them one by one.
"""
import numpy as np

NONE = 0xFFFFFFFF


def delay_ref(free_c, free_m, arrival, dur, cores, mem, max_wait_s=10, jump=True):
    """Returns (node, start, finish, stats, trace).  trace = {"place": [(t, position, len(Level1) before
    the pass, node)], "skip": [(t, position)] (the D6-skipped entries), "pass": [(t, len(Level1), nodes
    grown since the previous pass)]}; positions count in the list as the pass found it."""
    fc, fm = np.array(free_c, np.int64), np.array(free_m, np.int64)
    arrival, dur, cores, mem = ([int(x) for x in v] for v in (arrival, dur, cores, mem))
    J = len(arrival)
    node, start, finish = [-1] * J, [NONE] * J, [NONE] * J
    running, level0, level1, jobs_map = [], [], [], {}
    trace = {"place": [], "skip": [], "pass": []}
    st = dict(t_end=0, placed=0, moved_l1=0, placed_l1=0, peak_l1=0, peak_running=0, flags=0, l1_left=0,
              total_wait_ms=0, jobs_count=0, ticks=0)
    snap_c, snap_m = fc.copy(), fm.copy()
    t = nxt = 0

    def touch(j, at):  # scheduler.go:309-312 / 338-341
        st["total_wait_ms"] += 1000 * (at - arrival[j]) - jobs_map.get(j, 0)
        jobs_map[j] = 1000 * (at - arrival[j])

    def schedule(j):  # ScheduleJob (first fit, >=) and Node.RunJob's commit
        fit = np.nonzero((fc >= cores[j]) & (fm >= mem[j]))[0]
        if fit.size == 0:
            return -1
        k = int(fit[0])
        if dur[j] > 0:  # (a zero-duration job is released before the next ScheduleJob)
            fc[k] -= cores[j]
            fm[k] -= mem[j]
            running.append((t + dur[j], k, j))
            st["peak_running"] = max(st["peak_running"], len(running))
        node[j], start[j], finish[j] = k, t, t + dur[j]
        jobs_map.pop(j)  # delete(JobsMap, id): TotalTime keeps its share
        st["placed"] += 1
        return k

    while True:
        st["ticks"] += 1
        for r in [r for r in running if r[0] <= t]:
            running.remove(r)
            fc[r[1]] += cores[r[2]]
            fm[r[1]] += mem[r[2]]
        while nxt < J and arrival[nxt] <= t:
            jobs_map[nxt] = 0
            st["jobs_count"] += 1
            level0.append(nxt)
            nxt += 1
        if st["placed"] == J:
            break
        changed = False
        if level1:
            n0, removed, i = len(level1), 0, 0
            trace["pass"].append((t, n0, int(((fc > snap_c) | (fm > snap_m)).sum())))
            while i < len(level1):
                j = level1[i]
                touch(j, t)
                k = schedule(j)
                if k >= 0:
                    del level1[i]  # append(Level1[:i], Level1[i+1:]...)
                    trace["place"].append((t, i + removed, n0, k))
                    if i < len(level1):
                        trace["skip"].append((t, i + removed + 1))
                    removed += 1
                    st["placed_l1"] += 1
                    changed = True
                i += 1  # no i--
        snap_c, snap_m = fc.copy(), fm.copy()
        if level0:
            j = level0[0]
            touch(j, t)
            if schedule(j) >= 0:
                level0.pop(0)
                changed = True
            elif t - arrival[j] >= max_wait_s:
                level1.append(level0.pop(0))
                st["moved_l1"] += 1
                st["peak_l1"] = max(st["peak_l1"], len(level1))
                changed = True
        if not changed and not running and not level0 and nxt == J:
            st["flags"] |= 1
            break
        tn = t + 1
        if jump and not changed:
            ev = [r[0] for r in running] + ([arrival[nxt]] if nxt < J else []) + \
                 ([arrival[level0[0]] + max_wait_s] if level0 else [])
            if min(ev) > tn:
                tn = min(ev)
                for j in level1 + level0[:1]:
                    touch(j, tn - 1)
                st["ticks"] += tn - (t + 1)
        assert tn < NONE, "the clock left the u32 range"
        t = tn
    st["t_end"], st["l1_left"] = t, len(level1)
    return (np.array(node, np.int32), np.array(start, np.uint32), np.array(finish, np.uint32), st, trace)
