"""Workloads that put the hand-scheduled DELAY loop (csrc/mcs_delay_asm.hip) on its structural edges:
Level1's 640-entry LDS slice and its 64-entry rows, the grown-node list G, the mode changes, the ends
of Level0, the 64-bit wait sum and the slot pool.  Shared by tests/test_delay_edges_cpu.py (which proves
from tests/delay_ref.py's trace that each edge is hit, and pins the oracle) and
tests/test_gpu_delay_edges.py.

The construction: "gate" nodes hold all the capacity, every other node has nothing free and every job
needs a core.  A blocker takes a whole gate for D seconds; the jobs behind it arrive with it, fail as
Level0 heads and move to Level1 one per second from t = max_wait_s on.  The blocker's release starts a
pass that places every other fitting entry (D6 steps over each successor); a prefix of P entries that
fit no node shifts the placements to later positions and rows, a suffix of Q such entries follows them.
Every cluster has 129-256 nodes (but the 1-node one of the mixed launch) and free values < 0x7FFF.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, List, Optional

import numpy as np

from mcs_amd import ClusterArrays, JobStreams

BIG = 700  # a gate that takes a whole Level1 of one-core jobs
L1CAP = 640


@dataclass
class Case:
    name: str
    free_c: List[int]
    free_m: List[int]
    jobs: List[tuple]  # (arrival, dur, cores, mem), in arrival order
    hit: Optional[Callable] = None  # (stats, trace) -> True when the edge the case is built for was reached


def pack(cases):
    fc = np.concatenate([np.asarray(c.free_c, np.uint32) for c in cases])
    fm = np.concatenate([np.asarray(c.free_m, np.uint32) for c in cases])
    assert fc.max() < 0x7FFF and fm.max() < 0x7FFF
    noff = np.zeros(len(cases) + 1, np.uint32)
    noff[1:] = np.cumsum([len(c.free_c) for c in cases])
    joff = np.zeros(len(cases) + 1, np.uint64)
    joff[1:] = np.cumsum([len(c.jobs) for c in cases])
    j = np.array([x for c in cases for x in c.jobs], np.uint32).reshape(-1, 4)
    return (ClusterArrays(fc.copy(), fm.copy(), fc, fm, noff),
            JobStreams(j[:, 0].copy(), j[:, 1].copy(), j[:, 2].copy(), j[:, 3].copy(), joff))


def nodes(gates, n_nodes=256):
    fc, fm = [0] * n_nodes, [0] * n_nodes
    for k, (c, m) in gates.items():
        fc[k], fm[k] = c, m
    return fc, fm


# ---- what a trace shows -------------------------------------------------------------------------
def placed_at(tr, pos, longer=True):
    """a Level1 placement at list position pos (with an entry behind it, which D6 steps over)"""
    return any(p == pos and (not longer or ((t, p + 1) in tr["skip"] and n > p + 1)) for t, p, n, _ in tr["place"])


def lane63(tr):
    return any(p % 64 == 63 and n > p + 1 and (t, p + 1) in tr["skip"] for t, p, n, _ in tr["place"])


def grown(tr, g, placing=False):
    ts = {t for t, _, _, _ in tr["place"]}
    return any(k == g and (not placing or t in ts) for t, _, k in tr["pass"])


def rows_touched(tr):
    return {p // 64 for _, p, _, _ in tr["place"]}


# ---- the blocked-gate construction --------------------------------------------------------------
def blocked(N, P=0, Q=0, mw=10, gate_c=BIG, jd=3, t0=0):
    """the jobs of one blocked gate: the blocker, P entries that fit no node, N one-core jobs, Q more
    that fit no node; all arrive at t0, the blocker leaves at t0 + D"""
    D = mw + P + N + Q + 30
    never = (t0, 5, gate_c + 1, 0)
    return [(t0, D, gate_c, 0)] + [never] * P + [(t0, jd, 1, 1)] * N + [never] * Q, D


def rows(N, P=0, Q=0, mw=10, gate=0, gate_c=BIG, jd=3, n_nodes=256, name=None, hit=None):
    fc, fm = nodes({gate: (gate_c, 1000)}, n_nodes)
    jobs, _ = blocked(N, P, Q, mw, gate_c, jd)
    return Case(name or f"rows_N{N}_P{P}_Q{Q}", fc, fm, jobs, hit)


def rows_family(mw=10):
    out = []
    for N in (63, 64, 65, 128, 129):
        # P = 0 places the even positions, P = 1 the odd ones: lane 63, then lane 0 of the next row stepped over
        out.append(rows(N, 0, mw=mw, hit=lambda st, tr, N=N: placed_at(tr, (N - 1) & ~1, longer=N % 2 == 0)
                        and st["peak_l1"] == N and grown(tr, 0, placing=True)))
        out.append(rows(N, 1, mw=mw, hit=lambda st, tr, N=N: st["peak_l1"] == N + 1 and (lane63(tr) or N < 64)
                        and placed_at(tr, 1)))
    for P in (63, 64, 65):  # rows without removals ahead of and behind the rows with removals
        out.append(rows(64, P, 64, mw=mw, hit=lambda st, tr, P=P: rows_touched(tr) == {P // 64, (P + 62) // 64}
                        and st["l1_left"] == P + 64 and st["flags"] == 1))
    return out


def capacity(K):
    """Level1 peaks at exactly K: K - 3 entries that fit no node and 3 that fit the blocked gate, while
    small jobs run from Level0 on a second gate (their releases start passes that place nothing)"""
    fc, fm = nodes({0: (BIG, 1000), 9: (2, 1000)})
    q = []
    for i in range(K - 3):
        if i % 100 == 50:
            q.append((0, 2, 1, 1))
        q.append((0, 5, BIG + 1, 0))
    q += [(0, 3, 3, 1)] * 3
    D = 10 + len(q) + 40
    last = K - 1
    return Case(f"capacity_K{K}", fc, fm, [(0, D, BIG, 0)] + q,
                lambda st, tr: st["peak_l1"] == K and placed_at(tr, last, longer=False) and placed_at(tr, last - 2))


def capacity_family():
    return [capacity(639), capacity(640), capacity(641),
            rows(64, 576, name="capacity_last_row",
                 hit=lambda st, tr: st["peak_l1"] == L1CAP and rows_touched(tr) == {9} and placed_at(tr, 638))]


def gates(idxs, N, gate_c=1, jd=3, name=None, hit=None):
    """one blocker per gate, placed one per second in node order and all released at the same second"""
    idxs = sorted(idxs)
    fc, fm = nodes({k: (gate_c, 1000) for k in idxs})
    D = 10 + len(idxs) + N + 30
    jobs = [(0, D - b, gate_c, 0) for b in range(len(idxs))] + [(0, jd, 1, 1)] * N
    return Case(name or "gates_" + "_".join(map(str, idxs)), fc, fm, jobs, hit)


def one_field():
    """node 10 grows in cores only (its blocker takes no memory), node 20 in memory only (its blocker
    takes no cores and fits no other node), at different seconds; the Level1 jobs need both"""
    fc, fm = nodes({10: (8, 50), 20: (8, 500)})
    jobs = [(0, 60, 8, 0), (0, 80, 0, 500)] + [(0, 3, 1, 40), (0, 3, 1, 400)] * 3  # (the second starts at t = 1)
    return Case("one_field", fc, fm, jobs,
                lambda st, tr: {(t, k) for t, _, _, k in tr["place"]} >= {(60, 10), (81, 20)} and
                [g for t, _, g in tr["pass"] if t in (60, 81)] == [1, 1])


def g_family():
    def on(nodes_):
        return lambda st, tr: {k for _, _, _, k in tr["place"]} == set(nodes_) and grown(tr, len(nodes_), placing=True)

    out = [gates([k], 5, gate_c=2, hit=on([k])) for k in (0, 1, 2, 3, 255)]
    mixed = [0, 5, 130, 255]  # one node of each chunk (node = lane * 4 + chunk)
    out.append(gates(mixed, 12, hit=on(mixed)))
    out.append(gates(range(64), 140, name="gates_64", hit=lambda st, tr: grown(tr, 64, placing=True)))
    out.append(gates(range(0, 130, 2), 140, name="gates_65", hit=lambda st, tr: grown(tr, 65, placing=True)))
    out.append(one_field())
    # nothing grown, a pass for the D6-untested entries alone: the second after the release
    out.append(rows(9, 0, jd=50, name="untested_alone", hit=lambda st, tr: grown(tr, 0, placing=True)))
    # two entries of one row fit only the same one-core gate: the second fails the re-test after the commit
    out.append(rows(5, 0, gate_c=1, jd=7, name="retest", hit=lambda st, tr: [p for t, p, _, _ in tr["place"]][:2] == [0, 0]
                    and len({t for t, _, _, _ in tr["place"]}) == 5))
    return out


def refill():
    """Level1 drains to empty and fills again (mode 1 -> 0 -> 1 -> 0)"""
    fc, fm = nodes({3: (BIG, 1000)})
    a, _ = blocked(5)
    b, _ = blocked(4, t0=200)
    return Case("refill", fc, fm, a + b,
                lambda st, tr: st["moved_l1"] == 9 and st["placed_l1"] == 9 and st["peak_l1"] == 5 and st["flags"] == 0)


def ends(J, dead):
    """Level0 runs out (J jobs in all) while Level1 holds jobs; then a drain, or a Level1 deadlock"""
    fc, fm = nodes({0: (BIG, 1000)})
    if J == 1:
        return Case("ends_J1_dead", fc, fm, [(0, 5, BIG + 1, 0)], lambda st, tr: st["flags"] == 1 and st["l1_left"] == 1)
    jobs, _ = blocked(J - 1 - int(dead), int(dead))
    return Case(f"ends_J{J}_{'dead' if dead else 'drain'}", fc, fm, jobs,
                lambda st, tr: st["moved_l1"] == J - 1 and st["flags"] == int(dead) and st["l1_left"] == int(dead))


def modes_family():
    out = [refill(), ends(1, True)]
    out += [ends(J, dead) for J in (64, 65, 128) for dead in (False, True)]
    fc, fm = nodes({0: (BIG, 1000)})
    out.append(Case("empty", fc, fm, [], lambda st, tr: st["t_end"] == 0 and st["jobs_count"] == 0))
    out.append(rows(65, 1, jd=0, name="zero_duration", hit=lambda st, tr: st["placed_l1"] == 65 and lane63(tr)))
    return out


def wide_family():
    """the seconds sum of the Level1 waits passes 2^32 under the checked horizon (last arrival + the sum
    of dur + 1 + max_wait_s stays below 2^32 - 1)"""
    fc, fm = nodes({0: (BIG, 1000)})
    wide = lambda st, tr: st["total_wait_ms"] >= 1000 << 32 and st["placed_l1"] == 5
    late = 3_000_000_000
    return [Case("wide_blocker", fc, fm, [(0, late, BIG, 0)] + [(0, 3, 1, 1)] * 5, wide),
            Case("wide_arrivals", fc, fm, [(late, 10 ** 9, BIG, 0)] + [(late, 3, 1, 1)] * 5, wide)]


def pool_case():
    """700 one-core 2000 s jobs at t = 0: one starts per second, the peak passes the 512 running slots"""
    return Case("pool", [64] * 256, [1000] * 256, [(0, 2000, 1, 1)] * 700, lambda st, tr: st["peak_running"] == 700)


def mixed_family():
    one = Case("one_node", [4], [100], [(0, 30, 4, 1), (0, 2, 1, 1), (0, 2, 5, 1)],
               lambda st, tr: st["flags"] == 1 and st["placed_l1"] == 1)
    return [rows(3, name="quiet"), capacity(641), pool_case(), ends(64, True), modes_family()[-2], one, rows(65, 1)]


FAMILIES = {"capacity": capacity_family, "rows": rows_family, "g": g_family, "modes": modes_family,
            "wide": wide_family, "pool": lambda: [pool_case()], "mixed": mixed_family}


# ---- the hand-derived DKATs inside 256-node clusters ----------------------------------------------
def embed_kat(k, offset):
    """the DKAT's cluster with `offset` nodes of nothing free before it and such nodes after it up to
    256; returns (case, expected node, start, finish)"""
    from kat_util import kat_cluster, kat_expect, kat_streams

    cl, s = kat_cluster(k), kat_streams(k)
    fc = [0] * offset + [n.CoresAvailable for n in cl.Nodes]
    fm = [0] * offset + [n.MemoryAvailable for n in cl.Nodes]
    fc += [0] * (256 - len(fc))
    fm += [0] * (256 - len(fm))
    en, es, ef = kat_expect(k)
    en = np.where(en >= 0, en + offset, en).astype(np.int32)
    jobs = list(zip(s.arrival.tolist(), s.dur.tolist(), s.cores.tolist(), s.mem.tolist()))
    return Case(f"{k['name']}+{offset}", fc, fm, jobs), en, es, ef


def embedded_kats(dkats):
    out = []
    for k in dkats:
        free_job = any(j[2] == 0 and j[3] == 0 for j in k["jobs"])  # it would fit a padding node
        out += [embed_kat(k, o) for o in ((0,) if free_job else (0, 1, 2, 3, 61))]
    return out
