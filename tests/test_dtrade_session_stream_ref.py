"""The rules of the cursor on a trading session's Start stream (mcs_trade_stream_next; DESIGN.md §14
"A cursor on a trading session's Start stream"), pinned on the CPU oracle alone.  No GPU needed.

The stream retires, against a frontier F, every full batch of 256 rows whose rows are all decided and
finished below F, on a physical or a virtual node; it keeps the Foreign records with a window that is not
empty and finish_s > F; and it computes the samples at t >= F from the live batches, the carried constant
(the retired rows' sum of s - a) and that list.  Here the computation is restated in numpy on
tests/dtrade_state_ref.py, tests/wait_ref.py and the restatement of tests/test_online_stream_ref.py, over
the oracle's run truncated at h (what the session holds after mcs_run(h),
tests/test_dtrade_session_ref.py), and compared at every second of [F, h) with the per-second references
over the whole run.  The (F, h) pairs are picked from the run so that each case the rule has to survive
occurs, and each is asserted on the data first:
  - a full, all-decided batch whose end_max is attained only by a job on a virtual node, with F between
    the batch's largest physical finish and that job's finish (the plain rule, k < N, would retire it);
  - a Foreign record with finish_s == F (dropped), one with finish_s == F + 1 (kept), one with
    start_s == h - 1, one with start_s == finish_s (never taken);
  - a virtual node received between two frontiers.
The drain rule (F* = t_last + 1 after a drain) and the cost workload's cap are pinned here too."""
import numpy as np
import pytest

import dtrade_state_ref as D
import oracle_ref as O
import wait_ref as R
from kat_util import seeded_workload
from mcs_amd import JobStreams
from test_online_series_ref import truncate
from test_online_stream_ref import BATCH, retired_batches, stream_wait
from test_online_stream_ref import W as MAX_WAIT

PERIOD = 5  # sample_period_s: with h = 1 (mod 5) a tick exists at h - 1, so t_max = h - 1 truncates there


def up(x):
    """the smallest h >= x with h = 1 (mod PERIOD)"""
    return x + (1 - x) % PERIOD


def plain_retired(n2, f2, F, n_phys):
    """WRONG for a trading session: the plain cursor's summary rule, end = finish of the jobs with k < N"""
    nb = len(n2) // BATCH
    dec = (n2[:nb * BATCH] >= 0).reshape(nb, BATCH).all(axis=1)
    f = np.where(n2[:nb * BATCH] < n_phys, f2[:nb * BATCH].astype(np.int64), -1)
    return dec & (f.reshape(nb, BATCH).max(axis=1) < F) if nb else np.zeros(0, bool)


def take(kept, log, seen, F):
    """dt_stream_foreign_kernel: the old list's records with finish > F, then the log records [seen, len)
    with a window that is not empty and finish > F"""
    new = log[seen:]
    return np.concatenate([kept[kept["finish"] > F], new[(new["start"] != new["finish"]) & (new["finish"] > F)]])


def stream_samples(arrays, streams, cut, F, h, flist, rule=None):
    """The samples of [F, h) by the rule: per cluster the rows of the batches that are not retired against
    F, and the Foreign list.  Returns (state samples, per cluster (TotalTime ms, JobsCount), retired)."""
    sub, n2, s2, f2 = truncate(streams, cut["node"], cut["start"], cut["finish"], h)
    nphys = np.diff(arrays.node_off)
    live_parts, waits, retired = [], [], []
    for c in range(arrays.n_clusters):
        j2 = sub.of(c)
        ret = retired_batches(n2[j2], f2[j2], F) if rule is None else rule(n2[j2], f2[j2], F, nphys[c])
        live = np.ones(j2.stop - j2.start, bool)
        for b in np.nonzero(ret)[0]:
            live[b * BATCH:(b + 1) * BATCH] = False
        live_parts.append(live)
        retired.append(ret)
        arr_c, s_c = sub.arrival[j2].astype(np.int64), s2[j2]
        dead = np.nonzero(~live)[0]
        a_base = int((s_c[dead].astype(np.int64) - arr_c[dead]).sum())
        waits.append((arr_c, s_c, np.nonzero(live)[0].tolist(), a_base))
    keep = np.concatenate(live_parts)
    off = np.concatenate([[0], np.cumsum([int(p.sum()) for p in live_parts])]).astype(np.uint64)
    lsub = JobStreams(*(getattr(sub, f)[keep] for f in ("arrival", "dur", "cores", "mem")), off)
    res = dict(node=n2[keep], start=s2[keep], finish=f2[keep], foreign=flist, vnodes=cut["vnodes"])
    return D.series_ref(arrays, lsub, res, F, 1, h - F), waits, retired


LATE = 13100  # arrival of the constructed job


@pytest.fixture(scope="module")
def big():
    """("big", 8, 800) and one more job, constructed: the seeded run ends at second 12426, before any of
    its Foreign jobs with a window finishes (12918 - 12985), so no truncated run of it has a Foreign
    finish at or below a frontier.  A small job that arrives in cluster 0 at second 13100 keeps the
    system running past them and changes nothing before its arrival."""
    arrays, s, _ = seeded_workload("big", 8, 800)
    seeded = O.dtrade_run(arrays, s)
    at = int(s.job_off[1])
    ins = lambda a, v: np.insert(a, at, v).astype(np.uint32)
    off = s.job_off.copy()
    off[1:] += 1
    streams = JobStreams(ins(s.arrival, LATE), ins(s.dur, 5), ins(s.cores, 1), ins(s.mem, 1), off)
    full = O.dtrade_run(arrays, streams)
    f, g = seeded["foreign"], full["foreign"]
    assert int(seeded["t_final"]) < int(f["finish"][f["start"] != f["finish"]].min()) < LATE <= int(full["t_final"])
    assert g[:len(f)].tobytes() == f.tobytes()
    return arrays, streams, full


def pick_pairs(arrays, streams, full):
    """(F, h, what, cluster or None): h = 1 (mod 5), F < h <= F + 60, each picked for the case it names"""
    nphys = np.diff(arrays.node_off)
    f = full["foreign"]
    hold = f[f["start"] != f["finish"]]
    tf = int(full["t_final"])
    out = []
    # the batch a virtual node's job keeps alive
    for c in range(arrays.n_clusters):
        js = streams.of(c)
        nd, st, fn = full["node"][js], full["start"][js].astype(np.int64), full["finish"][js].astype(np.int64)
        for b in range(len(nd) // BATCH):
            s = slice(b * BATCH, (b + 1) * BATCH)
            virt = nd[s] >= nphys[c]
            if (nd[s] < 0).any() or not virt.any() or virt.all():
                continue
            lo = int(max(fn[s][~virt].max(), st[s].max())) + 1
            if int(fn[s][virt].max()) > lo + 5 and up(lo + 20) <= tf:
                out.append((lo, up(lo + 20), "vnode_end_max", c))
                break
        if out:
            break
    early = hold[hold["finish"].astype(np.int64) + 20 <= tf]  # (the truncated runs end below t_final)
    r = early[np.argmax(early["finish"].astype(np.int64) - early["start"])]
    F = int(r["finish"])
    assert up(F + 12) <= tf
    out.append((F, up(F + 12), "finish_eq_F", int(r["responder"])))
    out.append((F - 1, up(F + 12), "finish_eq_F1", int(r["responder"])))
    r = hold[(hold["start"] % PERIOD == 0) & (hold["start"] + 1 <= tf)][-1]
    out.append((int(r["start"]) + 1 - 30, int(r["start"]) + 1, "start_eq_h1", int(r["responder"])))
    z = f[(f["start"] == f["finish"]) & (f["start"] > 100)][0]
    out.append((int(z["start"]) - 3, up(int(z["start"]) + 2), "zero_window", int(z["responder"])))
    won = full["trades"][full["trades"]["winner"] >= 0]
    t = int(won["t"][len(won) // 2])
    out.append((t - 8, up(t + 2), "vnode_between", int(won["requester"][len(won) // 2])))
    return out


def test_live_batches_constants_and_the_foreign_list_give_the_whole_history(big):
    arrays, streams, full = big
    nphys = np.diff(arrays.node_off)
    pairs = pick_pairs(arrays, streams, full)
    hmax = max(h for _, h, _, _ in pairs)
    reps = {c: R.replay(streams.arrival[streams.of(c)], full["start"][streams.of(c)], MAX_WAIT, hmax)
            for c in range(arrays.n_clusters)}
    seen = set()
    for F, h, what, c0 in pairs:
        assert 0 < F < h <= F + 60 and h % PERIOD == 1, (F, h, what)
        cut = O.dtrade_run(arrays, streams, t_max=h - 1)
        before = O.dtrade_run(arrays, streams, t_max=up(F - 4) - 1)  # a frontier one slice earlier
        log = cut["foreign"]
        # the list as two calls build it: the earlier call's list, then the records logged since
        F0 = up(F - 4) - PERIOD
        kept0 = take(log[:0], before["foreign"], 0, F0)
        assert len(before["foreign"]) <= len(log) and before["foreign"].tobytes() == log[:len(before["foreign"])].tobytes()
        flist = take(kept0, log, len(before["foreign"]), F)
        direct = log[(log["start"] != log["finish"]) & (log["finish"] > F)]
        assert sorted(flist.tolist()) == sorted(direct.tolist())
        # the cases, asserted on the data
        if what == "finish_eq_F" and (log["finish"] == F).any() and not (flist["finish"] == F).any():
            seen.add(what)
        if what == "finish_eq_F1" and (flist["finish"] == F + 1).any():
            seen.add(what)
        if what == "start_eq_h1" and (flist["start"] == h - 1).any():
            seen.add(what)
        if what == "zero_window" and ((log["start"] == log["finish"]) & (log["start"] >= F)).any() \
                and not (flist["start"] == flist["finish"]).any():
            seen.add(what)
        if what == "vnode_between" and any(len(a) > len(b) for a, b in zip(cut["vnodes"], before["vnodes"])):
            seen.add(what)
        got, waits, retired = stream_samples(arrays, streams, cut, F, h, flist)
        if what == "vnode_end_max":
            _, _, wrong = stream_samples(arrays, streams, cut, F, F + 1, flist, rule=plain_retired)
            assert wrong[c0].sum() == retired[c0].sum() + 1  # the plain rule retires the batch, the right one does not
            seen.add(what)
        if any(r.any() for r in retired):
            seen.add("retired")
        want = D.series_ref(arrays, streams, full, F, 1, h - F)
        bad = np.nonzero((D.bits(got) != D.bits(want)).any(-1))
        assert len(bad[0]) == 0, f"{what} F {F} h {h}: first (cluster, k) {[(int(c), int(k)) for c, k in zip(*bad)][:3]}"
        for c, (arr_c, s_c, live_rows, a_base) in enumerate(waits):  # the wait statistics of every cluster
            tot, cnt = stream_wait(arr_c, s_c, live_rows, a_base, range(F, h))
            assert tot == reps[c]["total_ms"][F:h].tolist(), f"{what} F {F} h {h} cluster {c}"
            assert cnt == reps[c]["count"][F:h].tolist(), f"{what} F {F} h {h} cluster {c}"
    need = {"vnode_end_max", "finish_eq_F", "finish_eq_F1", "start_eq_h1", "zero_window", "vnode_between", "retired"}
    assert need <= seen, f"the inputs do not exercise {sorted(need - seen)}"


def test_the_plain_summary_rule_is_wrong_for_a_trading_session(big):
    """Retiring the batch that a virtual node's job keeps alive drops that job from `running`."""
    arrays, streams, full = big
    F, h, what, c = pick_pairs(arrays, streams, full)[0]
    assert what == "vnode_end_max"
    cut = O.dtrade_run(arrays, streams, t_max=h - 1)
    log = cut["foreign"]
    flist = log[(log["start"] != log["finish"]) & (log["finish"] > F)]
    got, _, _ = stream_samples(arrays, streams, cut, F, F + 3, flist, rule=plain_retired)
    want = D.series_ref(arrays, streams, full, F, 1, 3)
    assert (got["running"][c] < want["running"][c]).all()


# ---- the drain rule ------------------------------------------------------------------------------------
def test_a_drain_decides_as_a_run_to_t_last_plus_one():
    """The oracle's run over the jobs held stops at T_d.  The run over all jobs (further ones arrive at
    T_d + 1 and later) truncated at t_max = T_d gives the same placements, Foreign log and virtual nodes,
    and every sample at or below T_d agrees: F* = T_d + 1."""
    arrays, streams, _ = seeded_workload("small", 4, 120)
    cutoff = int(np.sort(streams.arrival)[len(streams.arrival) // 2])
    held_m = streams.arrival < cutoff

    def part(m, shift=0):
        off = np.concatenate([[0], np.cumsum([int(m[streams.of(k)].sum()) for k in range(arrays.n_clusters)])])
        return JobStreams((streams.arrival[m].astype(np.int64) + shift).astype(np.uint32), streams.dur[m],
                          streams.cores[m], streams.mem[m], off.astype(np.uint64))

    held = part(held_m)
    o_held = O.dtrade_run(arrays, held)
    td = int(o_held["t_final"])
    assert (o_held["node"] >= 0).all()  # a drain: every job held is decided
    shift = td + 1 - int(streams.arrival[~held_m].min())
    assert shift > 0
    later = part(~held_m, shift)  # the first of them arrives at T_d + 1, where appends are allowed again
    parts, off = [[], [], [], []], [0]
    for k in range(arrays.n_clusters):
        for i, f in enumerate(("arrival", "dur", "cores", "mem")):
            parts[i].append(np.concatenate([getattr(held, f)[held.of(k)], getattr(later, f)[later.of(k)]]))
        off.append(off[-1] + len(parts[0][-1]))
    everything = JobStreams(*[np.concatenate(p).astype(np.uint32) for p in parts], np.array(off, np.uint64))
    o_all = O.dtrade_run(arrays, everything, t_max=td)
    full = O.dtrade_run(arrays, everything)
    assert int(full["t_final"]) > td and o_all["t_final"] == td
    rows = np.concatenate([np.arange(int(everything.job_off[k]), int(everything.job_off[k]) + len(range(*held.of(k).indices(1 << 62))))
                           for k in range(arrays.n_clusters)])
    for k in ("node", "start", "finish"):
        np.testing.assert_array_equal(o_all[k][rows], o_held[k], err_msg=k)
    rest = np.setdiff1d(np.arange(len(everything.arrival)), rows)
    assert (o_all["node"][rest] == -1).all()
    assert o_all["foreign"].tobytes() == o_held["foreign"].tobytes() and o_all["vnodes"] == o_held["vnodes"]
    assert len(o_held["foreign"]) > 0 and sum(len(v) for v in o_held["vnodes"]) > 0
    # every sample at or below T_d: the run over the jobs held, the truncated run and the whole run agree
    n = td + 1
    a = D.series_ref(arrays, held, o_held, 0, 1, n)
    b = D.series_ref(arrays, everything, o_all, 0, 1, n)
    w = D.series_ref(arrays, everything, full, 0, 1, n)
    assert (D.bits(a) == D.bits(b)).all() and (D.bits(b) == D.bits(w)).all()
    for c in range(arrays.n_clusters):
        ra = R.replay(held.arrival[held.of(c)], o_held["start"][held.of(c)], MAX_WAIT, td)
        rw = R.replay(everything.arrival[everything.of(c)], full["start"][everything.of(c)], MAX_WAIT, td)
        np.testing.assert_array_equal(ra["total_ms"], rw["total_ms"], err_msg=f"cluster {c}")
        np.testing.assert_array_equal(ra["count"], rw["count"], err_msg=f"cluster {c}")
    # and the rule is sharp: at T_d + 1 the whole run has a job the drained run never saw
    a1 = D.series_ref(arrays, held, o_held, td + 1, 1, 1)
    w1 = D.series_ref(arrays, everything, full, td + 1, 1, 1)
    assert (D.bits(a1) != D.bits(w1)).any()


# ---- the cost workload's cap ---------------------------------------------------------------------------
def test_the_rule_alone_keeps_the_cost_workload_within_half_a_rescan():
    """tests/test_gpu_dtrade_session_stream.py::test_cost_follows_the_slice, by the rule alone over the
    oracle's run of that workload: 40 equal slices of the arrival span, one call per slice at period 5
    with wait statistics.  A call loads the rows of the batches that were not retired when it began; a
    rescan loads every row held.  The cursor stays within half of the rescan."""
    arrays, s, _ = seeded_workload("small", 4, 4000)
    streams = JobStreams((s.arrival.astype(np.int64) * 5).astype(np.uint32), s.dur, s.cores, s.mem, s.job_off)
    o = O.dtrade_run(arrays, streams)
    assert max(len(v) for v in o["vnodes"]) <= 64 and o["n_foreign"] > 0  # no replay inside the session
    top = int(streams.arrival.max()) + 1
    hs = [top * k // 40 for k in range(1, 41)]
    scanned = held_sum = retired = 0
    for h in hs:
        t_next = (h + PERIOD - 1) // PERIOD * PERIOD
        sub, n2, s2, f2 = truncate(streams, o["node"], o["start"], o["finish"], h)
        held = len(sub.arrival)
        scanned += held - retired
        held_sum += held
        retired = sum(BATCH * int(retired_batches(n2[sub.of(c)], f2[sub.of(c)], t_next).sum()) for c in range(4))
    print(f"rows loaded {scanned} of {held_sum} held over the calls: {scanned / held_sum:.3f}")
    assert 2 * scanned <= held_sum
    assert retired > len(streams.arrival) // 2
