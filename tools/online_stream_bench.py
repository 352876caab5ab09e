#!/usr/bin/env python3
"""Device time of mcs_stream_next against mcs_online_state_series for the same live slice (DESIGN.md §14,
profiles/online_stream/): the `slice` mode of tools/online_series_bench.py with a stream open.

C4 shape (4096 clusters x 256 nodes x 16384 jobs, scaled arrivals at 90 % load, DELAY), the session
advanced to 3/4 of the arrivals.  A stream is opened there at period 1 with the wait statistics, and
--warm slices are taken untimed: the first of them catches up over the history once.  Then --live times:
append the next 5 s of jobs, run(h + 5), mcs_stream_next for the five new seconds, and
mcs_online_state_series for the same five seconds in the same process (with the record at t0, as the
`slice` mode of online_series_bench.py asks for it, and without); the bytes of the two must agree.

Every timed figure is the call's kernel_ms (HIP events on the engine stream, summed over its launches).
The yardstick is the parent commit's mcs_online_state_series: run `online_series_bench.py slice` from a
checkout of the parent in alternating processes.  Under `rocprofv3 --kernel-trace --stats` (a run of its
own, --no-series so that only the stream's kernels are traced) the trace gives the share by kernel.
One JSON object on stdout, and in --out when given."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "multi-cluster-simulator_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))

from online_series_bench import cut, host_streams, load_clusters_only, spread  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--policy", choices=["FIFO", "DELAY"], default="DELAY")
    ap.add_argument("--clusters", type=int, default=4096)
    ap.add_argument("--nodes", type=int, default=256)
    ap.add_argument("--jobs", type=int, default=16384)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--live", type=int, default=5)
    ap.add_argument("--no-series", action="store_true", help="the stream alone (for a kernel trace)")
    ap.add_argument("--out")
    args = ap.parse_args()

    from mcs_amd import Engine
    from mcs_amd import _lib as L

    streams = host_streams(args)
    h = (int(streams.arrival.max()) + 1) * 3 // 4
    with Engine(0, policy=args.policy) as eng:
        load_clusters_only(eng, args)
        eng.append_jobs(cut(streams, 0, h))
        eng.run(h)
        eng.stream_open(h, 1)
        if not args.no_series:
            eng.online_state_series(h - 5, 1, 5)  # warm-up
        runs, nexts, series, series_nofirst, scanned, warm = [], [], [], [], [], []
        for k in range(args.warm + args.live):
            eng.append_jobs(cut(streams, h, h + 5))
            run_ms = eng.run(h + 5).kernel_ms
            samples, wait, st = eng.stream_next(5)
            assert st["n_written"] == 5 and st["t_first"] == h and st["pending"] == 0, st
            if k < args.warm:
                warm.append(dict(kernel_ms=st["kernel_ms"], rows_scanned=st["rows_scanned"]))
            else:
                runs.append(run_ms)
                nexts.append(st["kernel_ms"])
                scanned.append(st["rows_scanned"])
            if not args.no_series:
                s2, w2, _, ms = eng.online_state_series(h, 1, 5, with_time=True)
                assert s2.tobytes() == samples.tobytes() and (wait is None or w2.tobytes() == wait.tobytes())
                if k >= args.warm:
                    series.append(ms)
                    series_nofirst.append(online_no_first(eng, L, h))
            h += 5
        res = dict(mode="stream", lib=os.path.basename(L.LIB_PATH), policy=args.policy, clusters=args.clusters,
                   nodes=args.nodes, jobs_per_cluster=args.jobs, horizon_s=h, jobs_in_session=int(eng.num_jobs),
                   warm_calls=warm, live_calls=args.live, run_5s=spread(runs), stream_next_5s=spread(nexts),
                   rows_scanned=scanned, rows_retired=st["rows_retired"])
        res["live_set"] = live_set(eng, st["t_next"])
        if series:
            res.update(series_5s=spread(series), series_5s_without_first=spread(series_nofirst))
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


def live_set(eng, t_next):
    """The session's batches of 256 rows by what keeps them from retiring against t_next, counted on the
    host from the placements: an undecided row (a Level1 job that starves, or one not yet reached), or
    every row decided but one still running at t_next; and how old the live batches are."""
    import numpy as np

    node, _, fin = eng.placements()
    arr = eng.read_jobs().arrival
    off = eng.job_offsets().astype(np.int64)
    out = dict(batches=0, retirable=0, live_undecided_row=0, live_running_row=0, partial_last=0,
               live_older_than_900s=0, rows=int(off[-1]), rows_retirable=0)
    for c in range(len(off) - 1):
        nd, fn, ar = node[off[c]:off[c + 1]], fin[off[c]:off[c + 1]].astype(np.int64), arr[off[c]:off[c + 1]]
        nb = len(nd) // 256
        und = (nd[:nb * 256] < 0).reshape(nb, 256).any(axis=1)
        late = (fn[:nb * 256].reshape(nb, 256).max(axis=1) >= t_next) & ~und
        old = ar[:nb * 256].astype(np.int64).reshape(nb, 256).max(axis=1) + 900 < t_next
        out["batches"] += nb + (len(nd) > nb * 256)
        out["partial_last"] += int(len(nd) > nb * 256)
        out["live_undecided_row"] += int(und.sum())
        out["live_running_row"] += int(late.sum())
        out["retirable"] += int((~und & ~late).sum())
        out["live_older_than_900s"] += int(((und | late) & old).sum())
    out["rows_retirable"] = 256 * out["retirable"]
    return out


def online_no_first(eng, L, h):
    """mcs_online_state_series for the five seconds from h without the record at t0 (first == NULL):
    what a stream replaces, which hands out no such record."""
    import ctypes as C

    import numpy as np
    from mcs_amd import CLUSTER_SAMPLE_DTYPE, WAIT_SAMPLE_DTYPE

    n = eng.num_clusters
    wait = eng.policy == "DELAY"
    out = np.zeros((n, 5), CLUSTER_SAMPLE_DTYPE)
    wout = np.zeros((n, 5), WAIT_SAMPLE_DTYPE)
    ms = C.c_double(0.0)
    rc = L.lib().mcs_online_state_series(eng._h, h, 1, 5, out.ctypes.data_as(C.POINTER(L.mcs_cluster_sample)),
                                         wout.ctypes.data_as(C.POINTER(L.mcs_wait_sample)) if wait else None, None,
                                         n, C.byref(ms))
    assert rc == L.MCS_OK, rc
    return ms.value


if __name__ == "__main__":
    main()
