#!/usr/bin/env python3
"""Cost of the cursor on a trading session's Start stream (DESIGN.md §14 "A cursor on a trading session's
Start stream") on the C5-DELAY system of `bench.py --config c5 --policy delay` (64 cluster_small
replicas x 2000 jobs, the reference client's arrivals).  kernel_ms from HIP events; prints one JSON line.

  --mode stream    a session run to second --t0, the stream opened at 0 (the first call catches up over
                   the history once), then --slices slices of --step s: append the slice's jobs,
                   mcs_run(h + step), mcs_trade_stream_next for the step's seconds at period 1 with wait
                   statistics.  Reports the catch-up call, the median over the slices after a warm-up
                   of --reps slices, rows_scanned against the rows held, the Foreign list.
  --mode series    the yardstick on the same slices: mcs_trade_session_state_series without `first` for
                   the same seconds (runs on a build without the cursor too)
  --mode batch     mcs_dtrade_state_series after a whole batch run (period 5, wait statistics and
                   `first`): the call that must not move, with the SHA-256 of what it returns
"""
import argparse
import hashlib
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "multi-cluster-simulator_amd")]


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["stream", "series", "batch"], required=True)
    ap.add_argument("--clusters", type=int, default=64)
    ap.add_argument("--jobs-per-cluster", type=int, default=2000)
    ap.add_argument("--t0", type=int, default=6000)
    ap.add_argument("--step", type=int, default=5)
    ap.add_argument("--slices", type=int, default=40)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=lambda s: int(s, 0), default=0x4D43535F53494D31)
    return ap.parse_args()


def med(v):
    return statistics.median(v)


def main():
    a = parse()
    import ctypes as C

    import numpy as np

    from mcs_amd import Cluster, Engine, GenParams, JobStreams, replicate
    from mcs_amd import _lib as L
    from mcs_amd.engine import gen_streams_host

    arrays = replicate(Cluster.load(os.path.join(REPO, "assets", "cluster_small.json")), a.clusters)
    streams = gen_streams_host(GenParams(seed=a.seed), arrays, a.jobs_per_cluster)

    def part(lo, hi):
        parts, off = [[], [], [], []], [0]
        for k in range(a.clusters):
            sl = streams.of(k)
            m = (streams.arrival[sl] >= lo) & (streams.arrival[sl] < hi)
            for i, f in enumerate(("arrival", "dur", "cores", "mem")):
                parts[i].append(getattr(streams, f)[sl][m])
            off.append(off[-1] + int(m.sum()))
        return JobStreams(*[np.concatenate(p).astype(np.uint32) for p in parts], np.array(off, np.uint64))

    out = {"mode": a.mode, "clusters": a.clusters, "jobs_per_cluster": a.jobs_per_cluster, "reps": a.reps,
           "t0": a.t0, "step": a.step, "slices": a.slices}
    hs = [a.t0 + a.step * (i + 1) for i in range(a.slices)]
    if a.mode == "batch":
        with Engine(0, policy="DELAY", trader=True) as eng:
            eng.load_clusters(arrays)
            eng.submit_jobs(streams)
            eng.run()
            n = eng.trade_stats()["t_final"] // 5 + 3
            ser = [eng.dtrade_state_series(0, 5, n, with_time=True)[3] for _ in range(a.reps + 1)][1:]
            sha = hashlib.sha256()
            for arr in eng.dtrade_state_series(0, 5, n):
                sha.update(arr.tobytes())
            out.update(sha256=sha.hexdigest(), n_samples=n, series_kernel_ms=med(ser), series_kernel_ms_all=ser)
        print(json.dumps(out))
        return
    with Engine(0, policy="DELAY", trader=True) as eng:
        eng.load_clusters(arrays)
        eng.submit_jobs(part(0, a.t0))
        eng.run(a.t0)
        n = eng.num_clusters
        if a.mode == "stream":
            eng.trade_stream_open(0, 1, True)
            _, _, first = eng.trade_stream_next(a.t0)
            out.update(catch_up_kernel_ms=first["kernel_ms"], catch_up_samples=first["n_written"],
                       catch_up_rows_scanned=first["rows_scanned"])
        run_ms, ms, scanned, held, live, wall = [], [], [], [], [], []
        samples = np.zeros((n, a.step), dtype=[("cu", "<f4"), ("mu", "<f4"), ("running", "<u4"), ("queued", "<u4")])
        wait = np.zeros((n, a.step), dtype=[("avg", "<f8"), ("total", "<i8"), ("count", "<i8")])
        ps, pw = samples.ctypes.data_as(C.POINTER(L.mcs_cluster_sample)), wait.ctypes.data_as(C.POINTER(L.mcs_wait_sample))
        st, kms = L.mcs_trade_stream_stats() if a.mode == "stream" else None, C.c_double(0.0)
        sha = hashlib.sha256()
        for h in hs:
            new = part(h - a.step, h)
            if len(new.arrival):  # (late in the run every job has arrived)
                eng.append_jobs(new)
            run_ms.append(eng.run(h).kernel_ms)
            if a.mode == "stream":
                rc = L.lib().mcs_trade_stream_next(eng._h, a.step, ps, pw, n, C.byref(st))
                assert rc == 0 and st.n_written == a.step and st.pending == 0, (rc, st.n_written, st.pending)
                ms.append(st.kernel_ms)
                scanned.append(int(st.rows_scanned))
                live.append(int(st.foreign_live))
            else:
                rc = L.lib().mcs_trade_session_state_series(eng._h, h - a.step, 1, a.step, ps, pw, None, n, C.byref(kms))
                assert rc == 0
                ms.append(kms.value)
            held.append(int(eng.job_offsets()[-1]))
            sha.update(samples.tobytes())
            sha.update(wait.tobytes())
        w = a.reps  # warm-up slices
        out.update(kernel_ms=med(ms[w:]), kernel_ms_min=min(ms[w:]), kernel_ms_max=max(ms[w:]),
                   slice_run_kernel_ms=med(run_ms[w:]), rows_held=held[-1], n_foreign=len(eng.foreign()),
                   sha256_samples=sha.hexdigest(), restarts=eng.trade_session_info()["restarts"])
        if a.mode == "stream":
            out.update(rows_scanned=med(scanned[w:]), rows_retired=int(st.rows_retired), foreign_live=live[-1],
                       frontier=int(st.frontier))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
