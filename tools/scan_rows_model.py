"""Which slot rows expire in a release scan of the streamed W16R loop (W16Q), from the
oracle's placements of the C4 stream, and what testing the rows in pairs would issue.
(The loop modelled here, W16Q, was removed once calendar rows replaced it; its last tree is e98c6d7.)

The loop's control flow is replayed from the oracle's start and finish seconds: the clock moves to a
head's arrival, from a failed fit to max(t + 1, the earliest finish) until the head's start second,
and by one second after a placed WaitQueue head; an advance that reaches the earliest finish is a
release scan.  The slots are handed out by the loop's policy (tools/slot_model.py: a current row, its
free lanes in order, a re-pick of the next row with a free lane), so each scan's expiries fall in
known rows.  Printed: advances, scans, failed fits and waited jobs per job, the distribution of
expiring rows per scan, and the scalar and branch instructions the row tests and returns issue per
scan (the bodies' own instructions are the same either way):
  today   8 x (s_and_b64 exec + s_cbranch) and one s_branch back per expiring row;
  pairs   4 x (s_or_b64 + s_cbranch); a pair with an expiry runs, out of line, s_and_b64 exec +
          s_cbranch for each of its two rows, and an s_branch back when its second row expires (when it
          does not, the second row's s_cbranch is the return);
and the taken branches of each.  Test infrastructure (the oracle).
usage: python tools/scan_rows_model.py [clusters]"""
import collections
import heapq
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "multi-cluster-simulator_amd"), os.path.join(REPO, "tests")]
import oracle_ref as O  # noqa: E402
from mcs_amd import GenParams  # noqa: E402
from mcs_amd.engine import gen_cluster_host, scaled_lambda  # noqa: E402

N, J, LANES, ROWS = 256, 16384, 64, 8


def replay(arr, dur, start, finish):
    """-> (advances, failed fits, waited, [the set of expiring rows of each scan])"""
    free = np.ones((LANES, ROWS), bool)
    cur, R = list(range(LANES)), 0
    heap, scans = [], []
    t = adv = failed = waited = 0

    def advance():
        nonlocal adv
        adv += 1
        if heap and heap[0][0] <= t:
            rows = set()
            while heap and heap[0][0] <= t:
                _, lane, row = heapq.heappop(heap)
                free[lane, row] = True
                rows.add(row)
            scans.append(rows)

    for k in range(len(arr)):
        if arr[k] > t:
            t = int(arr[k])
            advance()
        w = False
        while int(start[k]) != t:  # a failed fit: the head sleeps to the next completion
            assert int(start[k]) > t and heap
            failed += 1
            w = True
            t = max(t + 1, heap[0][0])
            advance()
        if dur[k]:
            if not cur:  # the re-pick
                for i in range(1, ROWS + 1):
                    p = (R + i) % ROWS
                    lanes = np.nonzero(free[:, p])[0]
                    if len(lanes):
                        cur, R = [int(x) for x in lanes], p
                        break
            if cur:
                lane = cur.pop(0)
                free[lane, R] = False
                heapq.heappush(heap, (int(finish[k]), lane, R))
        if w:  # a placed WaitQueue head sleeps one second
            waited += 1
            t += 1
            advance()
    return adv, failed, waited, scans


def cost_today(rows):
    """-> (scalar, branch, taken branches)"""
    return 8, 8 + len(rows), 2 * len(rows)


def cost_pairs(rows):
    salu, branch, taken = 4, 4, 0
    for a in range(0, ROWS, 2):
        if a in rows or a + 1 in rows:
            salu += 2
            branch += 2 + (a + 1 in rows)
            taken += 2 + (a not in rows)
    return salu, branch, taken


def main():
    gp = GenParams(seed=0x4D43535F53494D31, arrival_mode=1, lam=scaled_lambda(N, load=0.9))
    nc = int(sys.argv[1]) if len(sys.argv) > 1 else 4
    adv = failed = waited = jobs = 0
    hist = collections.Counter()
    tot = [0] * 6
    nscans = nrows = 0
    for ci in range(nc):
        a, d, c, m = gen_cluster_host(gp, ci, 32, 24000, J)
        node, start, finish = O.fifo_run(np.full(N, 32, np.uint32), np.full(N, 24000, np.uint32), a, d, c, m)[:3]
        assert (node >= 0).all()
        r = replay(a, d, start, finish)
        adv, failed, waited, jobs = adv + r[0], failed + r[1], waited + r[2], jobs + len(a)
        for rows in r[3]:
            hist[len(rows)] += 1
            nrows += len(rows)
            tot = [x + y for x, y in zip(tot, [*cost_today(rows), *cost_pairs(rows)])]
        nscans += len(r[3])
    print({"clusters": nc, "advances_per_job": round(adv / jobs, 3), "scans_per_job": round(nscans / jobs, 3),
           "failed_fits_per_job": round(failed / jobs, 3), "waited_per_job": round(waited / jobs, 3),
           "rows_per_scan": round(nrows / nscans, 3),
           "scans_by_expiring_rows": {k: round(v / nscans, 4) for k, v in sorted(hist.items())},
           "today_per_scan": {"scalar": round(tot[0] / nscans, 2), "branch": round(tot[1] / nscans, 2),
                              "taken": round(tot[2] / nscans, 2)},
           "pairs_per_scan": {"scalar": round(tot[3] / nscans, 2), "branch": round(tot[4] / nscans, 2),
                              "taken": round(tot[5] / nscans, 2)},
           "saved_per_job": {"scalar": round((tot[0] - tot[3]) / jobs, 2), "branch": round((tot[1] - tot[4]) / jobs, 2)},
           "taken_added_per_job": round((tot[5] - tot[2]) / jobs, 2)})


if __name__ == "__main__":
    main()
