"""The retire rule of the start-stream cursor (mcs_stream_next), pinned without a GPU.

A stream keeps per batch of 256 rows what no later horizon can change and retires, against a frontier F,
every full batch whose rows are all decided and finished below F.  From then on it computes the samples
at t >= F from the other (live) batches plus one carried constant per cluster, the retired rows' sum of
s - a.  Here that computation is restated in numpy over the oracle's FIFO and DELAY runs, truncated at
several horizons h as tests/test_online_series_ref.py truncates them, and compared at every second of
[F, h) with the whole run's values: wait_ref's replay of the Go loop and the brute-force series_ref.

The (h, F) pairs are picked from the run so that the cases the rule has to survive occur, and each is
asserted first: a starved Level1 row inside an otherwise finished batch, a zero-duration job that starts
at F, a D6 skip whose placement lies below F while the stepped-over entry is still live, and retired
batches that are not a prefix of their cluster."""
import numpy as np
import pytest

import oracle_ref as O
import wait_ref as R
from mcs_amd import JobStreams, replicate, uniform_cluster
from test_gpu_state_series import assert_samples_equal, series_ref
from test_online_series_ref import truncate

W = 10
BATCH = 256
JOBS = 1100
INF = 1 << 60


def workload(policy, seed=3, clusters=2):
    """Five nodes of 32 cores at about 70 % load; every 90th job asks for a whole node and waits in
    Level1 while smaller jobs pass; one 500 s job early in each cluster keeps its batch live long after
    the next one has finished.  Under DELAY row 600 of the last cluster asks for more cores than a node
    has: it starves in Level1 for good while its batch finishes around it (under FIFO it would block the
    queue's head, and the run would end there)."""
    arrays = replicate(uniform_cluster(5, cores=32, memory=24000), clusters)
    rng = np.random.default_rng(seed)
    parts = []
    for c in range(clusters):
        arr = np.cumsum(rng.poisson(1.0, JOBS))
        dur, cores, mem = rng.integers(0, 20, JOBS), rng.integers(0, 25, JOBS), rng.integers(0, 12001, JOBS)
        cores[45::90] = 32
        dur[100], cores[100] = 500, 1
        if policy == "DELAY" and c == clusters - 1:
            cores[600] = 33
        parts.append((arr, dur, cores, mem))
    off = (np.arange(clusters + 1) * JOBS).astype(np.uint64)
    return arrays, JobStreams(*(np.concatenate([p[f] for p in parts]).astype(np.uint32) for f in range(4)), off)


@pytest.fixture(scope="module", params=["FIFO", "DELAY"])
def full(request):
    policy = request.param
    arrays, streams = workload(policy)
    if policy == "DELAY":
        node, start, fin, stats = O.delay_run_batch(arrays, streams, n_threads=4, max_wait_s=W)
    else:
        node, start, fin, stats = O.fifo_run_batch(arrays, streams, n_threads=4)
    assert int((node < 0).sum()) == (policy == "DELAY")
    T = int(stats["t_end"].max()) + 3
    C = len(streams.job_off) - 1
    reps = [R.replay(streams.arrival[streams.of(c)], start[streams.of(c)], W, T) for c in range(C)] \
        if policy == "DELAY" else None
    want = series_ref(arrays, streams, node, start, fin, 0, 1, T)
    return policy, arrays, streams, node, start, fin, T, reps, want


def retired_batches(n2, f2, F):
    """Per full batch of a cluster's rows: every row decided and finished below F."""
    nb = len(n2) // BATCH
    dec = (n2[:nb * BATCH] >= 0).reshape(nb, BATCH).all(axis=1)
    fmax = f2[:nb * BATCH].astype(np.int64).reshape(nb, BATCH).max(axis=1) if nb else np.zeros(0, np.int64)
    return dec & (fmax < F)


def wait_records(arr, s2):
    """h, m, s of the formulas heading csrc/mcs_wait.hip (s = INF for an undecided row)."""
    d, hs, ms, ss = -1, [], [], []
    for a, s in zip(arr.tolist(), s2.tolist()):
        s = INF if s == R.TIME_NONE else s
        h = max(a, d + 1)
        m = max(h, a + W)
        d = min(s, m)
        hs.append(h), ms.append(m), ss.append(s)
    return hs, ms, ss


def skip_of(P, hs, ms, ss):
    """wait_skip_of: the run of skipped seconds of the entry that P's Level1 placement steps over."""
    u = ss[P]
    if u == INF or u <= ms[P]:
        return 0
    k = None
    for q in range(P + 1, len(hs)):
        if hs[q] >= u:
            break
        if ms[q] < u <= ss[q]:
            k = q
            break
    if k is None:
        return 0
    r, lo = 1, P
    while r <= u:
        tg = u - r
        if ms[k] >= tg:
            break
        f = next((q for q in range(k - 1, lo, -1) if ss[q] == tg and tg > ms[q]), None)
        if f is None:
            break
        r, lo = r + 1, f
    return r


def stream_wait(arr, s2, live_rows, a_base, ts):
    """TotalTime (ms) and JobsCount at the seconds ts from the live rows and the carried constant."""
    hs, ms, ss = wait_records(arr, s2)
    tot, cnt = [], []
    for t in ts:
        A = a_base
        B = 0
        skip = 0
        for j in live_rows:
            if hs[j] <= t:
                A -= int(arr[j])
                B += 1
            if ss[j] <= t:
                A += ss[j]
                B -= 1
            if ss[j] == t:
                skip += skip_of(j, hs, ms, ss)
        tot.append(1000 * (A + t * B - skip))
        cnt.append(int((arr <= t).sum()))
    return tot, cnt


def pairs(policy, streams, node, start, fin, reps):
    """(h, F, what) with F < h <= F + 60, picked from the run; `what` names the case the pair is for."""
    out = []
    arr, dur = streams.arrival.astype(np.int64), streams.dur
    st, fi = start.astype(np.int64), fin.astype(np.int64)
    for c in range(len(streams.job_off) - 1):
        js = streams.of(c)
        a, s, f = arr[js], st[js], fi[js]
        # the row that starves for good: from the second on at which the rest of its batch has finished
        for j in np.nonzero(node[js] < 0)[0]:
            b = j // BATCH
            F = int(np.delete(f[b * BATCH:(b + 1) * BATCH], j - b * BATCH).max()) + 1
            out.append((F + 40, F, "starved"))
        z = np.nonzero((dur[js] == 0) & (s > 300))[0]
        out.append((int(s[z[0]]) + 30, int(s[z[0]]), "zero"))
        # the 500 s job keeps batch 0 live while batch 1 has finished
        F = int(f[BATCH:2 * BATCH].max()) + 1
        assert F < f[100]
        out.append((F + 40, F, "gap"))
        if reps is not None:
            k, t = next((k, t) for k, t in reps[c]["skips"] if t > 200)
            out.append((t + 26, t + 1, "skip"))
    return out


def test_live_batches_and_carried_constants_give_the_whole_history(full):
    policy, arrays, streams, node, start, fin, T, reps, want = full
    seen = set()
    for h, F, what in pairs(policy, streams, node, start, fin, reps):
        assert 0 < F < h <= F + 60 and h < T
        sub, n2, s2, f2 = truncate(streams, node, start, fin, h)
        live_parts = []
        for c in range(len(streams.job_off) - 1):
            j2 = sub.of(c)
            ret = retired_batches(n2[j2], f2[j2], F)
            live = np.ones(j2.stop - j2.start, bool)
            for b in np.nonzero(ret)[0]:
                live[b * BATCH:(b + 1) * BATCH] = False
            # the cases, asserted on the data
            und = n2[j2] < 0
            nb = len(ret)
            if what == "starved":
                for b in range(nb):
                    rows = slice(b * BATCH, (b + 1) * BATCH)
                    done = ~und[rows] & (f2[j2][rows].astype(np.int64) < F)
                    if und[rows].any() and done.sum() == BATCH - und[rows].sum() and not ret[b]:
                        seen.add("starved")
            if what == "zero" and ((sub.dur[j2] == 0) & (s2[j2] == F) & live).any():
                seen.add("zero")
            if ret.any() and not ret[:np.nonzero(ret)[0].max() + 1].all():
                seen.add("gap")
            if reps is not None and any(t < F and live[k] and int(s2[j2][k]) >= F for k, t in reps[c]["skips"]
                                        if k < len(live)):
                seen.add("skip")
            if ret.any():
                seen.add("retired")
            live_parts.append(live)
            # the wait statistics from the live rows and the carried constant
            if reps is not None:
                arr_c, s_c = sub.arrival[j2].astype(np.int64), s2[j2]
                dead = np.nonzero(~live)[0]
                a_base = int((s_c[dead].astype(np.int64) - arr_c[dead]).sum())
                tot, cnt = stream_wait(arr_c, s_c, np.nonzero(live)[0].tolist(), a_base, range(F, h))
                assert tot == reps[c]["total_ms"][F:h].tolist(), f"{what} h {h} F {F} cluster {c}"
                assert cnt == reps[c]["count"][F:h].tolist(), f"{what} h {h} F {F} cluster {c}"
        # the state samples from the live rows alone
        keep = np.concatenate(live_parts)
        off = np.concatenate([[0], np.cumsum([int(p.sum()) for p in live_parts])]).astype(np.uint64)
        lsub = JobStreams(*(getattr(sub, f)[keep] for f in ("arrival", "dur", "cores", "mem")), off)
        got = series_ref(arrays, lsub, n2[keep], s2[keep], f2[keep], F, 1, h - F)
        assert_samples_equal(got, want[:, F:h], f"{what} h {h} F {F}")
    need = {"zero", "gap", "retired"} | ({"starved", "skip"} if policy == "DELAY" else set())  # FIFO has no Level1
    assert need <= seen, f"the inputs do not exercise {sorted(need - seen)}"


def test_the_rule_is_sharp(full):
    """Retiring a batch one second early, while a job of it still runs at F, changes a state sample,
    and (DELAY) dropping the carried constant changes the wait statistics."""
    policy, arrays, streams, node, start, fin, T, reps, want = full
    js = streams.of(0)
    F = int(fin[js][:BATCH].astype(np.int64).max())  # the 500 s job's finish: batch 0 is not retired at F - 1
    h = F + 5
    sub, n2, s2, f2 = truncate(streams, node, start, fin, h)
    assert not retired_batches(n2[sub.of(0)], f2[sub.of(0)], F - 1)[0] and retired_batches(n2[sub.of(0)], f2[sub.of(0)], F + 1)[0]
    keep = np.ones(len(n2), bool)
    keep[:BATCH] = False  # batch 0 of cluster 0 dropped against F - 1
    off = np.array([0] + [int(keep[sub.of(c)].sum()) for c in range(2)], np.uint64).cumsum().astype(np.uint64)
    lsub = JobStreams(*(getattr(sub, f)[keep] for f in ("arrival", "dur", "cores", "mem")), off)
    got = series_ref(arrays, lsub, n2[keep], s2[keep], f2[keep], F - 1, 1, 1)
    assert got["running"][0, 0] == want["running"][0, F - 1] - 1
    if reps is not None:
        j2 = sub.of(0)
        arr_c, s_c = sub.arrival[j2].astype(np.int64), s2[j2]
        tot, _ = stream_wait(arr_c, s_c, list(range(BATCH, len(arr_c))), 0, [F + 1])
        base = int((s_c[:BATCH].astype(np.int64) - arr_c[:BATCH]).sum())
        assert base > 0 and tot[0] == reps[0]["total_ms"][F + 1] - 1000 * base
