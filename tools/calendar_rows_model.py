"""Calendar slot rows of the streamed W16R loop (W16C, DESIGN.md §4 "Calendar rows") on the C4 stream:
what the loop's clock advances compare and release when a running slot lives in row finish & 7.

The loop's control flow is replayed from the oracle's start and finish seconds as in
tools/scan_rows_model.py (the clock moves to a head's arrival, from a failed fit to the next
completion, and by one second after a placed WaitQueue head), with the slot policy of the loop:
  insert    row r = finish & 7, its lowest free lane; the row full: the first row r+1 ... r+7 (mod 8)
            with a free lane (a misplaced slot; XMIN = the earliest finish of the misplaced slots);
  advance   by one second (a placed head, a step of a failed fit's sleep, an arrival one second on):
            t >= XMIN -> the full scan (every row, then XMIN rebuilt), else row t & 7 alone;
            an arrival more than one second on: the full scan (XMIN rebuilt only if t >= XMIN);
  failed    the head steps a second at a time until a step releases something; after eight steps
  fit       without a release the clock jumps to the exact earliest finish.  The steps, the release that
            ends them and the head's placement run in the waiting-head section of the copy (DESIGN.md §4,
            "The waiting head"; WAIT below holds its counts beside those of the loop before it).
Two insert policies are replayed side by side ("Running jobs stay in their batch lane"):
  per-job   the slot is taken at the placement (the loop before);
  deferred  a placed job stays in its batch lane (the LIVE column, compared at every clock advance beside the
            calendar row) until it finishes there or its batch of 64 ends; then the live lanes go to their rows
            together, each row's candidates to its free lanes, and a row's surplus spills as a per-job insert did.
DEFER holds the instructions the deferred policy adds and removes, counted from the listing; LANE those of the
three steps of "Lane results"  on top of it, FITC those of "Fit and commit" on top of those, per step, from
the deferred replay's events.
Printed per job: release scans and what they compared, spills, failed fits and the seconds their sleeps
cross, the compares that release nothing, the running slots; and the instructions a scan issues, counted
from the listing of the loop as built (COST below; the pair scan of the loop before it from
tools/scan_rows_model.py's figures and MCS_FA_SCAN16Q / MCS_FA_SCANEND16Q).  Test infrastructure (the oracle).
usage: python tools/calendar_rows_model.py [clusters]"""
import collections
import heapq
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "multi-cluster-simulator_amd"), os.path.join(REPO, "tests")]
import oracle_ref as O  # noqa: E402
from mcs_amd import GenParams  # noqa: E402
from mcs_amd.engine import gen_cluster_host, scaled_lambda  # noqa: E402

N, J, LANES, ROWS = 256, 16384, 64, 8

# instructions issued, from the listing (scalar and branch | vector | LDS)
COST = {
    # the advance's XMIN test (2; a branch more from the placed head and an arrival) + the copy's row block
    # with an expiry (4 | 2 | 2) + mcsfa_reltail (7 | 10 | 1)
    "one-row scan": {"scalar": 2 + 4 + 7, "vector": 2 + 10, "lds": 3},
    # a step of a waiting head's sleep that finds nothing (the usual empty compare): s_add, the limit's compare
    # and branch, the row's branch; after a placed head or an arrival: the XMIN test (2, a branch more from an
    # arrival) and the block's branch, mcsfa_norel being empty
    "empty compare": {"scalar": 4, "vector": 1, "lds": 0},
    # MCS_FC_FULL: the advance's test (2-4) + 8 x (1 | 1) + per expiring row (5 | 1 | 1) + 5 + the computed
    # jump back into the copy (4 and the table's branch) + mcsfa_reltail
    "full scan": {"scalar": 4 + 1 + 8 + 5 * 1.7 + 5 + 5 + 7, "vector": 8 + 1.7 + 10, "lds": 2 + 1.7},
    # ... and XMIN's rebuild after one a misplaced slot asked for (32 vector, v_mov, 6 DPP, v_readlane | 7 s_nop)
    "XMIN rebuild": {"scalar": 7, "vector": 40, "lds": 0},
    # MCS_FA_SCAN16Q + MCS_FA_SCANEND16Q + the pair blocks (tools/scan_rows_model.py: 14.8 scalar and branch
    # for the pairs) + the peak and exec (2) + two instructions of a row's body scalar, two vector, per
    # expiring row (1.63) + the tail's 6 scalar, 4 + 7 vector of the minimum and 10 of the fit test
    "pair scan before": {"scalar": 14.8 + 2 + 2 * 1.63 + 6, "vector": 8 + 2 * 1.63 + 4 + 7 + 10, "lds": 2 + 1.63},
}


# the paths of a waiting WaitQueue head, per event: (scalar and branch, vector) before the waiting-head section
# and with it, from the two listings.  The step before: s_add, the carry branch, the countdown and its
# branch, the XMIN test (2), the row's branch; with it: s_add, the limit's compare and branch, the row's branch.
# The release that ends a sleep: mcsfa_reltail's 7 and mcsfa_fitted's branch before, the section's tail of 6
# with it.  The placed head: the record read's two tests (4), mcsfa_zarrp (6), the restore (s_nop and two
# lane accesses), the step with its carry branch (2), the XMIN test and the branch (3); with it: the two
# counts, s47, the step, the XMIN test (and a branch after copy 7).
WAIT = {
    "failed-fit entry": ("failed fits", (6, 1), (7, 0)),
    "sleep step": ("sleep steps", (7, 1), (4, 1)),
    "mcsfa_norel after a step on an empty row": ("empty compares: failed fit", (2, 0), (0, 0)),
    "release that ends a sleep": ("failed fits", (8, 10), (6, 10)),
    "placed head": ("waited", (17, 5), (7.125, 3)),
    "mcsfa_norel of the other advances": ("empty compares: other", (2, 0), (0, 0)),
}


# the deferred insert against the per-job one, from the two listings: (scalar, branch, vector, LDS) per event
DEFER = {
    # the pass's decision: the slot insert's 11 scalar instructions and its spill branch go (s_and s49, s_lshl m0,
    # s_movrels, s_ff1 s85, s_lshl s[62:63], s_andn2, s_and, s_movreld, s_mov exec, s_lshl2_add s79,
    # s_set_gpr_idx_idx; s_cbranch_scc0), and the three indexed v_mov; one v_writelane (LIVE) comes
    "placement": ("inserts", (-11, -1, -2, 0)),
    # every row compare is preceded by LIVE's: v_cmp and an untaken s_cbranch_vccnz
    "row compare": ("row compares", (0, 1, 1, 0)),
    # the out-of-line batch-lane release with nothing in the calendar row, against the row block's in-line body:
    # the same exec / count / exec, one taken branch more, v_lshl_add and the second v_cmp
    "batch-lane release, row empty": ("batch-lane scans, row empty", (0, 1, 2, 0)),
    # ... with the row expiring as well: its body (4 scalar: exec, count, FREE, the sum), a branch back
    "batch-lane release and row": ("batch-lane scans, row expires", (4, 2, 3, 1)),
    # the bulk move of a batch with a live lane (MCS_FC_BMOVE): 2 + 8 x 4 + 2 + 8 x 3 + 1 scalar, 1 + 8 + 1 branch,
    # 7 + 8 x 5 + 1 + 8 + 8 x 5 + 8 x 4 + 1 vector, the write and eight reads
    "bulk move": ("bulk moves", (61, 10, 129, 9)),
    # a batch end with no live lane: v_cmp and the branch
    "bulk move, nothing live": ("bulk moves, nothing live", (0, 1, 1, 0)),
    # a surplus job's insert at the batch end (mcsfa_bmo / mcsfa_bml: about one row searched), per spill of the
    # deferred replay
    "surplus insert": ("spills", (22, 5, 7, 0)),
    # the per-job insert's spill, which goes, per spill of the per-job replay (MCS_FC_SPILL beside the insert that
    # "placement" has taken off already, about one row searched: s_and s76; s_add, s_and, s_cmp, s_lshl m0, s_nop,
    # s_movrels, s_cmp_lg and the loop's two branches; s_ff1, s_lshl, s_andn2, s_movreld, s_min and the branch back)
    "per-job spill": ("spills", (-13, -3, 0, 0), "per-job insert"),
}


# "Lane results" (DESIGN.md §4), per step and event: (scalar, branch, vector, LDS), from the listings
LANE = {
    # A: a live job's start is formed when its lane leaves LIVE.  The placement loses v_writelane v92; a
    # batch-lane release (mcsfa_brel / mcsfa_wbrel, the full scan's ninth row) gains a v_sub; every stored batch
    # and the exit gain v_cmp, v_sub, v_cndmask (MCS_FA_STARTS16C)
    "A": {
        "placement": ("inserts", (0, 0, -1, 0)),
        "batch-lane release": ("batch-lane releases", (0, 0, 1, 0)),
        "stored batch": ("batch ends", (0, 0, 3, 0)),
        "exit": ("exits", (0, 0, 3, 0)),
    },
    # B (built and measured, not kept): node and finish written under exec = the job's lane.  The placement:
    # s_mov exec, s_mov m0, s_add s80, two v_writelane, three v_readlane -> s_lshl exec, v_mov, v_add, s_mov exec,
    # two v_readlane; the fit test's s_add s55 becomes s_add s80, taken back by an s_sub at a failed fit; the
    # zero route reads the duration itself; MCS_FC_SHIFT loses v90's two instructions per batch
    "B": {
        "placement": ("inserts", (-1, 0, -1, 0)),
        "failed fit": ("failed fits", (1, 0, 0, 0)),
        "zero route": ("zero-duration jobs", (0, 0, 1, 0)),
        "batch taken": ("batch ends", (0, 0, -2, 0)),
    },
    # C: a row is one register quad and the bulk move reads into it: eight v_mov -1 and eight times v_cmp and
    # three v_cndmask go; a surplus insert gains the s_lshl of its register index
    "C": {
        "bulk move": ("bulk moves", (0, 0, -40, 0)),
        "surplus insert": ("spills", (1, 0, 0, 0)),
    },
}


# "Fit and commit" (DESIGN.md §4), per step and event: (scalar, branch, vector, LDS), from the listings
FITC = {
    # F: the fit test in nine vector instructions (two v_perm that sign-replicate the guard bits, two SDWA ANDs)
    # for ten (four SDWA ANDs, one v_perm).  A job's own fit test runs once where it is placed (the pass, a
    # release's tail, the zero route), once more per failed fit, and a release behind a placed head runs one
    # for nothing when no job is ready
    "F": {
        "placement": ("inserts", (0, 0, -1, 0)),
        "zero-duration job": ("zero-duration jobs", (0, 0, -1, 0)),
        "failed fit": ("failed fits", (0, 0, -1, 0)),
        "tail's fit test dropped": ("placed-head releases, no ready job behind", (0, 0, -1, 0)),
    },
    # C: the commit is a v_cndmask under a scalar lane mask: s_lshl_b64 exec + v_mov + s_mov_b64 exec ->
    # s_lshl_b64 s[60:61] + v_cndmask (the pass's decision and the waiting head's placement)
    "C": {
        "placement": ("inserts", (-1, 0, 0, 0)),
    },
    # U (counted, not built): the running count from the cursor.  The placement loses s_add s80; a release scan
    # gains one instruction, a batch end one
    "U": {
        "placement": ("inserts", (-1, 0, 0, 0)),
        "release scan": ("release scans", (1, 0, 0, 0)),
        "batch end": ("batch ends", (1, 0, 0, 0)),
    },
}


def replay(arr, dur, start, finish, st, deferred=False):
    free = np.ones((ROWS, LANES), bool)
    heap = []  # (finish, job)
    slot = {}  # job -> (row, lane, misplaced), or None while it sits in its batch lane
    mis = []  # finishes of the misplaced slots alive (a heap)
    t = 0

    def release():
        """-> rows released at t (-1: the batch lanes), misplaced among them"""
        rows, m = set(), 0
        while heap and heap[0][0] <= t:
            f, j = heapq.heappop(heap)
            where = slot.pop(j)
            if where is None:
                if -1 not in rows:
                    st["batch-lane releases"] += 1
                rows.add(-1)
                st["jobs that finish in their batch lane"] += 1
                continue
            row, lane, x = where
            free[row, lane] = True
            rows.add(row)
            if x:
                m += 1
                mis.remove(f)
                heapq.heapify(mis)
        return rows, m

    def insert(j, f, bulk=False):
        r, x = f & 7, 0
        if not free[r].any():
            st["spills"] += 1
            x = 1
            for i in range(1, ROWS):
                if free[(f + i) & 7].any():
                    r = (f + i) & 7
                    break
            else:
                raise AssertionError("pool full")
            heapq.heappush(mis, f)
        lane = int(np.argmax(free[r]))
        free[r, lane] = False
        slot[j] = (r, lane, x)
        return x

    def bulk_move():
        live = sorted(j for j, w in slot.items() if w is None)
        st["bulk moves" if live else "bulk moves, nothing live"] += 1
        st["batch ends"] += 1
        # each row's candidates first (the rows' own free lanes), then the surplus one at a time
        left = []
        for j in live:
            f = int(finish[j])
            if free[f & 7].any():
                insert(j, f)
            else:
                left.append(j)
        for j in left:
            insert(j, int(finish[j]))
        st["batches with a surplus"] += bool(left)

    def full(why):
        rows, _ = release()
        st["full scans: " + why] += 1
        if rows:
            st["release scans"] += 1
            st["scans of all eight rows"] += 1
        else:
            st["full scans that release nothing"] += 1
        return bool(rows)

    def adv1(kind):
        if mis and t >= mis[0]:
            return full("a misplaced slot is due")
        due = heap and heap[0][0] <= t
        st["row compares"] += 1
        if due:
            rows, m = release()
            assert rows <= {t & 7, -1} and not m, (rows, t)
            st["release scans"] += 1
            st["scans of one row"] += 1
            if -1 in rows:
                st["batch-lane scans, row expires" if len(rows) == 2 else "batch-lane scans, row empty"] += 1
        else:
            st["empty compares: " + kind] += 1
        return bool(due)

    for k in range(len(arr)):
        if deferred and k and k % LANES == 0:
            bulk_move()
        if arr[k] > t:
            gap, t = int(arr[k]) - t, int(arr[k])
            st["arrival advances"] += 1
            if gap == 1:
                adv1("arrival")
            else:
                st["arrival gaps of 2-7 s" if gap < 8 else "arrival gaps of 8 s and more"] += 1
                full("an arrival gap")
        w = False
        while int(start[k]) != t:  # a failed fit: the head sleeps to the next completion
            assert int(start[k]) > t and heap
            st["failed fits"] += 1
            w = True
            steps, sleep0 = 0, t
            while True:
                if steps == 8:
                    st["exact-minimum jumps"] += 1
                    t = heap[0][0]
                    st["row compares"] -= 1  # (the jump lands in the row block; counted with the step)
                    assert adv1("failed fit")
                    break
                t += 1
                steps += 1
                st["sleep steps"] += 1
                if adv1("failed fit"):
                    break
            st["longest sleep"] = max(st["longest sleep"], t - sleep0)
        st["zero-duration jobs"] += not dur[k]
        if dur[k]:
            f = int(finish[k])
            heapq.heappush(heap, (f, k))
            if deferred:
                slot[k] = None
            else:
                insert(k, f)
            st["inserts"] += 1
        st["running"].append(sum(w is not None for w in slot.values()) if deferred else len(heap))
        if w:  # a placed WaitQueue head sleeps one second
            st["waited"] += 1
            t += 1
            if adv1("placed head") and not (k + 1 < len(arr) and arr[k + 1] <= t):
                st["placed-head releases, no ready job behind"] += 1  # (the tail's fit test is dropped)
    st["exits"] += 1


def main():
    gp = GenParams(seed=0x4D43535F53494D31, arrival_mode=1, lam=scaled_lambda(N, load=0.9))
    nc = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    st, sd = collections.Counter(), collections.Counter()
    st["running"], sd["running"] = [], []
    jobs = 0
    for ci in range(nc):
        a, d, c, m = gen_cluster_host(gp, ci, 32, 24000, J)
        node, start, finish = O.fifo_run(np.full(N, 32, np.uint32), np.full(N, 24000, np.uint32), a, d, c, m)[:3]
        assert (node >= 0).all()
        replay(a, d, start, finish, st)
        replay(a, d, start, finish, sd, deferred=True)
        jobs += len(a)
    drun = np.array(sd.pop("running"))
    sd.pop("longest sleep")
    run = np.array(st.pop("running"))
    longest = st.pop("longest sleep")
    scans = st["release scans"]
    out = {"clusters": nc, "jobs": jobs, "per_job": {k: round(v / jobs, 4) for k, v in sorted(st.items())},
           "share_of_release_scans": {k: round(st[k] / scans, 4) for k in ("scans of one row", "scans of all eight rows")},
           "longest_failed_fit_sleep_s": longest,
           "running_slots": {"mean": round(float(run.mean()), 1), "p99": int(np.percentile(run, 99)), "max": int(run.max())},
           "instructions_per_scan": {k: {f: round(x, 1) for f, x in v.items()} for k, v in COST.items()}}
    one, full_, emp = st["scans of one row"], st["scans of all eight rows"], sum(v for k, v in st.items() if k.startswith("empty"))
    for f in ("scalar", "vector", "lds"):
        new = (one * COST["one-row scan"][f] + (full_ + st["full scans that release nothing"]) * COST["full scan"][f]
               + st["full scans: a misplaced slot is due"] * COST["XMIN rebuild"][f] + emp * COST["empty compare"][f]) / jobs
        old = scans * COST["pair scan before"][f] / jobs
        out.setdefault("clock_advance_instructions_per_job", {})[f] = {"calendar rows": round(new, 2), "pair scan before": round(old, 2)}
    st["empty compares: other"] = st["empty compares: placed head"] + st["empty compares: arrival"]
    rows = {k: {"per_job": round(st[n] / jobs, 4), "before": list(b), "with the section": list(a)} for k, (n, b, a) in WAIT.items()}
    for i, f in enumerate(("scalar", "vector")):
        rows["change per job: " + f] = round(sum(st[n] * (a[i] - b[i]) for n, b, a in WAIT.values()) / jobs, 2)
    out["waiting_head_paths"] = rows
    keys = ("row compares", "release scans", "jobs that finish in their batch lane", "batch-lane scans, row expires",
            "batch-lane scans, row empty", "spills", "full scans: a misplaced slot is due", "bulk moves",
            "bulk moves, nothing live", "batches with a surplus")
    both = {k: {"per-job insert": round(st[k] / jobs, 4), "deferred": round(sd[k] / jobs, 4)} for k in keys}
    both["slots in the table"] = {"per-job insert": {"mean": round(float(run.mean()), 1), "max": int(run.max())},
                                  "deferred": {"mean": round(float(drun.mean()), 1), "max": int(drun.max())}}
    batches = sd["bulk moves"] + sd["bulk moves, nothing live"]
    both["share of batches with a surplus"] = round(sd["batches with a surplus"] / max(batches, 1), 4)
    change = {}
    for name, (n, cost, *of) in DEFER.items():
        count = (st if of else sd)[n]  # the deferred replay's events, but for what the per-job insert alone did
        change[name] = {"per_job": round(count / jobs, 4), "scalar, branch, vector, lds": list(cost)}
        for i, f in enumerate(("scalar", "branch", "vector", "lds")):
            change.setdefault("change per job", dict.fromkeys(("scalar", "branch", "vector", "lds"), 0.0))[f] += count * cost[i] / jobs
    change["change per job"] = {f: round(x, 2) for f, x in change["change per job"].items()}
    out["deferred_insert"] = {"replay": both, "instructions": change}
    steps = {}
    for step, events in LANE.items():
        rows = {name: {"per_job": round(sd[n] / jobs, 4), "scalar, branch, vector, lds": list(cost)}
                for name, (n, cost) in events.items()}
        rows["change per job"] = {f: round(sum(sd[n] * cost[i] for n, cost in events.values()) / jobs, 2)
                                  for i, f in enumerate(("scalar", "branch", "vector", "lds"))}
        steps[step] = rows
    steps["kept (A + C): change per job"] = {f: round(steps["A"]["change per job"][f] + steps["C"]["change per job"][f], 2)
                                             for f in ("scalar", "branch", "vector", "lds")}
    out["lane_results"] = steps
    steps = {}
    for step, events in FITC.items():
        rows = {name: {"per_job": round(sd[n] / jobs, 4), "scalar, branch, vector, lds": list(cost)}
                for name, (n, cost) in events.items()}
        rows["change per job"] = {f: round(sum(sd[n] * cost[i] for n, cost in events.values()) / jobs, 2)
                                  for i, f in enumerate(("scalar", "branch", "vector", "lds"))}
        steps[step] = rows
    steps["kept (F + C): change per job"] = {f: round(steps["F"]["change per job"][f] + steps["C"]["change per job"][f], 2)
                                             for f in ("scalar", "branch", "vector", "lds")}
    out["fit_commit"] = steps
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
