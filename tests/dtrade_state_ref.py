"""Brute-force host reference of the ClusterState record after a DELAY trading run
(mcs_dtrade_state_series), from the run's public outputs only: the placements, the
Foreign log, the virtual-node capacities (O.dtrade_run or the engine's readers) and the inputs.

The record of cluster c at second t, after the Delay iteration of t and before its trader rounds:
  - rows: the N physical nodes, then the virtual nodes c received, cap = free0 = the contract's size;
  - an own job with node >= 0 holds {cores, mem} of its row on start <= t < finish;
  - a Foreign job with responder == c holds {c, m} of its row on start < t < finish (strict);
  - counters are Go uint64: free = free0 - held (mod 2^64), over Python ints;
  - utilization = (sum in row order, in float32, of float32(cap) - float32(uint64 free)) / float32 of
    the uint32 sum of the physical capacities;
  - running = own + Foreign jobs holding; queued = own jobs arrived by t and not started by t.

The switches select the wrong readings the tests tell from the right one."""
import numpy as np

from mcs_amd import CLUSTER_SAMPLE_DTYPE

M64 = (1 << 64) - 1
M32 = (1 << 32) - 1


def f32_of_u64(x: int) -> np.float32:
    """Go's float32(uint64): round to nearest even, computed on the integer (no double rounding)."""
    x = int(x)
    if x < (1 << 24):
        return np.float32(x)
    sh = x.bit_length() - 24
    q, r, half = x >> sh, x & ((1 << sh) - 1), 1 << (sh - 1)
    if r > half or (r == half and (q & 1)):
        q += 1
    return np.float32(q) * np.float32(2.0 ** sh)  # q <= 2^24 and a power of two: exact


def serial_sum(terms: np.ndarray) -> np.float32:
    """x = 0; for v in terms: x += v, in float32 (np.add.accumulate runs in order)."""
    if len(terms) == 0:
        return np.float32(0.0)
    return np.add.accumulate(terms.astype(np.float32), dtype=np.float32)[-1]


class ClusterRows:
    def __init__(self, arrays, vnodes, c, with_vnodes=True):
        ns = arrays.nodes_of(c)
        self.n_phys = ns.stop - ns.start
        vn = list(vnodes[c]) if with_vnodes else []
        self.cap = [[int(x) for x in arrays.cap_c[ns]] + [int(v[0]) for v in vn],
                    [int(x) for x in arrays.cap_m[ns]] + [int(v[1]) for v in vn]]
        self.free0 = [[int(x) for x in arrays.free_c[ns]] + [int(v[0]) for v in vn],
                      [int(x) for x in arrays.free_m[ns]] + [int(v[1]) for v in vn]]
        self.n = len(self.cap[0])
        self.total = [np.float32(sum(self.cap[r][:self.n_phys]) & M32) for r in (0, 1)]
        self.base = [np.array([np.float32(cp) - f32_of_u64(fr) for cp, fr in zip(self.cap[r], self.free0[r])],
                              np.float32) for r in (0, 1)]

    def utilization(self, held, mask=M64):
        """held: ({row: cores}, {row: mem}) -> (cu, mu) as float32"""
        out = []
        for r in (0, 1):
            terms = self.base[r].copy()
            for k, h in held[r].items():
                terms[k] = np.float32(self.cap[r][k]) - f32_of_u64((self.free0[r][k] - h) & mask)
            with np.errstate(divide="ignore", invalid="ignore"):
                out.append(np.float32(serial_sum(terms)) / self.total[r])
        return out


def series_ref(arrays, streams, res, t0, period, n, strict=True, with_foreign=True, with_vnodes=True, u32=False):
    """res: node, start, finish, foreign (fields responder, node, start, finish, c, m) and vnodes (per
    cluster a list of (cores, mem)).  Returns (n_clusters, n) samples of CLUSTER_SAMPLE_DTYPE.
    strict=False: a Foreign job holds from its start tick on; with_foreign=False: no Foreign job holds;
    with_vnodes=False: the virtual rows are left out (a job on one holds nothing); u32=True: the
    counters are truncated to 32 bits."""
    node, start, fin, foreign = res["node"], res["start"], res["finish"], res["foreign"]
    out = np.zeros((arrays.n_clusters, n), CLUSTER_SAMPLE_DTYPE)
    mask = M32 if u32 else M64
    for c in range(arrays.n_clusters):
        rows = ClusterRows(arrays, res["vnodes"], c, with_vnodes)
        js = streams.of(c)
        nd, st, fi = node[js].astype(np.int64), start[js].astype(np.int64), fin[js].astype(np.int64)
        arr = streams.arrival[js].astype(np.int64)
        cores, mem = [int(x) for x in streams.cores[js]], [int(x) for x in streams.mem[js]]
        fr = foreign[foreign["responder"] == c] if with_foreign else foreign[:0]
        fn, fs, ff = fr["node"].astype(np.int64), fr["start"].astype(np.int64), fr["finish"].astype(np.int64)
        fc, fm = [int(x) for x in fr["c"]], [int(x) for x in fr["m"]]
        for k in range(n):
            t = t0 + k * period
            run = np.nonzero((nd >= 0) & (st <= t) & (t < fi))[0]
            frun = np.nonzero(((fs < t) if strict else (fs <= t)) & (t < ff))[0]
            held = ({}, {})
            for i in run:
                if nd[i] < rows.n:
                    held[0][int(nd[i])] = held[0].get(int(nd[i]), 0) + cores[i]
                    held[1][int(nd[i])] = held[1].get(int(nd[i]), 0) + mem[i]
            for i in frun:
                if fn[i] < rows.n:
                    held[0][int(fn[i])] = held[0].get(int(fn[i]), 0) + fc[i]
                    held[1][int(fn[i])] = held[1].get(int(fn[i]), 0) + fm[i]
            cu, mu = rows.utilization(held, mask)
            queued = int(((arr <= t) & ((nd < 0) | (st > t))).sum())
            out[c, k] = (cu, mu, len(run) + len(frun), queued)
    return out


def golden_series(kat, n_clusters, n):
    """Per-second samples [0, n) of a fixture of tests/golden/kats_dtrade_state.json: per cluster the
    segments [t_from, t_to, cores sum, memory sum, running, queued] (the sums are the exact float32
    values of the row sums, written as integers) and the totals the sums are divided by."""
    out = np.zeros((n_clusters, n), CLUSTER_SAMPLE_DTYPE)
    for c in range(n_clusters):
        tc, tm = (np.float32(x) for x in kat["totals"][c])
        seen = np.zeros(n, bool)
        for t_from, t_to, cs, ms, running, queued in kat["segments"][str(c)]:
            for t in range(t_from, min(t_to, n - 1) + 1):
                out[c, t] = (np.float32(float(cs)) / tc, np.float32(float(ms)) / tm, running, queued)
                seen[t] = True
        assert seen.all(), (kat["name"], c)
    return out


def bits(samples):
    """The samples as comparable words (NaNs equal to themselves)."""
    return np.stack([samples["cores_utilization"].view(np.uint32), samples["memory_utilization"].view(np.uint32),
                     samples["running"], samples["queued"]], axis=-1)
