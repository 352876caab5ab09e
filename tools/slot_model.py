"""How often the row-wise slot insert of the streamed W16R loop (W16Q) has to re-pick a
row, from the oracle's placements of the C4 stream (256 nodes, scaled arrivals at 90 % load).
(The loop modelled here, W16Q, was removed once calendar rows replaced it; its last tree is e98c6d7.)

The model is the kernel's policy on its 64 lanes x 8 rows of running slots: a current row R and the
set CUR of lanes whose row R is free and not yet handed out; an insert takes CUR's lowest lane; a
release marks the freed (lane, row) in the per-lane free-row bits (for row R: "freed since it became
current"); an insert that finds CUR empty re-picks the first row p = R+1 ... R+8 (mod 8) with a free
lane, which becomes CUR.  Printed: inserts, re-picks, inserts per re-pick, the shortest run between
two re-picks, how often the first row tried was empty, the mean number of free slots after an insert,
and for comparison the re-picks of a cache of one LANE's free rows (W16T, r06: a lane has 8 slots).
The model also checks the policy itself: a handed-out slot is free, and an insert finds no slot only
when all 512 are taken.  Test infrastructure (the oracle).
usage: python tools/slot_model.py [clusters]"""
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


def rows_model(start, finish, dur):
    """-> (inserts, re-picks, shortest run, first row tried empty, sum of free slots after the inserts,
    inserts skipped on a full pool)"""
    taken = np.zeros((LANES, ROWS), bool)
    freed = np.zeros((LANES, ROWS), bool)  # the free-row bits (v89)
    freed[:, 1:] = True                    # entry: R = 0, CUR = every lane, bit 0 clear
    cur, R = list(range(LANES)), 0
    heap = []
    ins = repick = first_empty = free_sum = skipped = 0
    run, shortest = 0, None
    for k in range(len(start)):
        t = int(start[k])
        while heap and heap[0][0] <= t:
            _, lane, row = heapq.heappop(heap)
            assert taken[lane, row]
            taken[lane, row] = False
            freed[lane, row] = True
        if dur[k] == 0:
            continue  # committed and released before the next decision: no slot
        ins += 1
        if not cur:
            repick += 1
            if run and (shortest is None or run < shortest):
                shortest = run
            run = 0
            for i in range(1, ROWS + 1):
                p = (R + i) % ROWS
                lanes = np.nonzero(freed[:, p])[0]
                if len(lanes):
                    cur, R = [int(x) for x in lanes], p
                    freed[:, p] = False
                    break
                first_empty += i == 1
            else:
                assert taken.all(), "no row found although a slot is free"
                skipped += 1
                continue
        lane = cur.pop(0)
        assert not taken[lane, R], "a taken slot was handed out"
        taken[lane, R] = True
        free_sum += LANES * ROWS - int(taken.sum())
        run += 1
        heapq.heappush(heap, (int(finish[k]), lane, R))
    return ins, repick, shortest, first_empty, free_sum, skipped


def lane_model(start, finish, dur):
    """W16T's cache, one LANE's free rows: re-picks (the lowest lane with a free row, as W16R picks)."""
    taken = np.zeros((LANES, ROWS), bool)
    heap, lane, rows, repick = [], 0, list(range(ROWS)), 0
    for k in range(len(start)):
        t = int(start[k])
        while heap and heap[0][0] <= t:
            _, l, r = heapq.heappop(heap)
            taken[l, r] = False
        if dur[k] == 0:
            continue
        rows = [r for r in rows if not taken[lane, r]]
        if not rows:
            repick += 1
            free = np.nonzero(~taken.all(axis=1))[0]
            if not len(free):
                continue
            lane = int(free[0])
            rows = [int(r) for r in np.nonzero(~taken[lane])[0]]
        r = rows.pop(0)
        taken[lane, r] = True
        heapq.heappush(heap, (int(finish[k]), lane, r))
    return repick


def main():
    gp = GenParams(seed=0x4D43535F53494D31, arrival_mode=1, lam=scaled_lambda(N, load=0.9))
    tot = np.zeros(6, np.int64)
    shortest, lane_repicks = None, 0
    for ci in range(int(sys.argv[1]) if len(sys.argv) > 1 else 4):
        a, d, c, m = gen_cluster_host(gp, ci, 32, 24000, J)
        node, start, finish = O.fifo_run(np.full(N, 32, np.uint32), np.full(N, 24000, np.uint32), a, d, c, m)[:3]
        placed = node >= 0
        res = rows_model(start[placed], finish[placed], d[placed])
        tot += [res[0], res[1], 0, res[3], res[4], res[5]]
        if res[2] is not None and (shortest is None or res[2] < shortest):
            shortest = res[2]
        lane_repicks += lane_model(start[placed], finish[placed], d[placed])
    ins, repick = int(tot[0]), int(tot[1])
    print({"inserts": ins, "repicks": repick, "inserts_per_repick": round(ins / max(repick, 1), 1),
           "shortest_run": shortest, "first_row_empty": int(tot[3]),
           "mean_free_slots": round(int(tot[4]) / max(ins, 1), 1), "skipped_full_pool": int(tot[5]),
           "lane_cache_repicks": lane_repicks,
           "lane_cache_inserts_per_repick": round(ins / max(lane_repicks, 1), 2)})


if __name__ == "__main__":
    main()
