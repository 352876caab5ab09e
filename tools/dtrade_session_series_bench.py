#!/usr/bin/env python3
"""Cost of the Start stream of a trading session (DESIGN.md §14 "The Start stream of a trading
session") on the C5-DELAY system of `bench.py --config c5 --policy delay` (64 cluster_small replicas x
2000 jobs, the reference client's arrivals).  kernel_ms from HIP events, each figure the median of
--reps calls after a warm-up; prints one JSON line.

  --mode series    a session run to second --t0 (6000), then --slices (40) slices of --step (5) s:
                   append the slice's jobs, mcs_run(h + step), then mcs_trade_session_state_series over
                   the step's seconds at period 1 with wait statistics and `first`, and
                   mcs_trade_session_level1_series over the same seconds.  Reports the median over
                   the slices and, at the last slice, the median of --reps repeated calls; the
                   Foreign log's length; --filter 0 sets MCS_DT_FOREIGN_FILTER=0 (the log scanned as
                   it is) before the engine is created.
  --mode tiles     the scan of the Foreign log in isolation: the session at --t0, then calls without wait
                   statistics over the last 127 * K seconds at period 1, K = 1, 8, 40 tiles, each of which
                   scans the log (or, with the pre-pass, the compacted list) once per cluster; reports the
                   log's length and the records the pre-pass keeps (counted on the host)
  --mode yardstick the only way to those samples without this call: a batch run with
                   t_max_s = t0 + slices * step - 1 from t = 0, then mcs_dtrade_state_series over the last
                   step's seconds (runs on a build without the call too)
  --mode batch     mcs_dtrade_state_series after a whole batch run at the reference cadence (period 5,
                   wait statistics and `first`): the call that must not move, with the SHA-256 of
                   what it returns
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
    ap.add_argument("--mode", choices=["series", "tiles", "yardstick", "batch"], required=True)
    ap.add_argument("--clusters", type=int, default=64)
    ap.add_argument("--jobs-per-cluster", type=int, default=2000)
    ap.add_argument("--t0", type=int, default=6000)
    ap.add_argument("--step", type=int, default=5)
    ap.add_argument("--slices", type=int, default=40)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--filter", choices=["0", "1"], default=None)
    ap.add_argument("--seed", type=lambda s: int(s, 0), default=0x4D43535F53494D31)
    return ap.parse_args()


def med(v):
    return statistics.median(v)


def main():
    a = parse()
    if a.filter is not None:
        os.environ["MCS_DT_FOREIGN_FILTER"] = a.filter
    import numpy as np

    from mcs_amd import Cluster, Engine, GenParams, JobStreams, replicate
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

    def engine(**cfg):
        eng = Engine(0, policy="DELAY", trader=True, **cfg)
        eng.load_clusters(arrays)
        return eng

    out = {"mode": a.mode, "clusters": a.clusters, "jobs_per_cluster": a.jobs_per_cluster, "reps": a.reps,
           "t0": a.t0, "filter": os.environ.get("MCS_DT_FOREIGN_FILTER", "default")}
    h_end = a.t0 + a.slices * a.step
    if a.mode == "yardstick":
        with engine(t_max_s=h_end - 1) as eng:
            eng.submit_jobs(streams)
            run_ms = [eng.run().kernel_ms for _ in range(a.reps + 1)][1:]
            ser = [eng.dtrade_state_series(h_end - a.step, 1, a.step, with_time=True)[3] for _ in range(a.reps + 1)][1:]
            ts = eng.trade_stats()
            n_foreign = len(eng.foreign())
        out.update(t_max_s=h_end - 1, run_kernel_ms=med(run_ms), run_kernel_ms_all=run_ms, series_kernel_ms=med(ser),
                   series_kernel_ms_all=ser, total_kernel_ms=med(run_ms) + med(ser), ticks=ts["ticks"],
                   loop_form=ts["loop_form"], n_foreign=n_foreign)
    elif a.mode == "series":
        hs = [a.t0 + a.step * (i + 1) for i in range(a.slices)]
        with engine() as eng:
            eng.submit_jobs(part(0, a.t0))
            eng.run(a.t0)
            f0 = len(eng.foreign())
            run_ms, ser_ms, l1_ms = [], [], []
            for h in hs:
                new = part(h - a.step, h)
                if len(new.arrival):  # (late in the run every job has arrived)
                    eng.append_jobs(new)
                run_ms.append(eng.run(h).kernel_ms)
                ser_ms.append(eng.trade_session_state_series(h - a.step, 1, a.step, with_time=True)[3])
                l1_ms.append(eng.trade_session_level1_series(h - a.step, 1, a.step, with_time=True)[1])
            h = hs[-1]
            rep = [eng.trade_session_state_series(h - a.step, 1, a.step, with_time=True)[3] for _ in range(a.reps + 1)][1:]
            nowait = [eng.trade_session_state_series(h - a.step, 1, a.step, with_wait=False, with_time=True)[3]
                      for _ in range(a.reps + 1)][1:]
            info = eng.trade_session_info()
            out.update(slice_run_kernel_ms=med(run_ms[1:]), series_kernel_ms_slices=med(ser_ms[1:]),
                       level1_kernel_ms_slices=med(l1_ms[1:]), series_kernel_ms=med(rep), series_kernel_ms_all=rep,
                       series_nowait_kernel_ms=med(nowait), n_foreign_at_t0=f0, n_foreign=len(eng.foreign()),
                       rows=int(eng.job_offsets()[-1]), restarts=info["restarts"])
    elif a.mode == "tiles":
        with engine() as eng:
            eng.submit_jobs(part(0, a.t0))
            eng.run(a.t0)
            f = eng.foreign()
            out.update(n_foreign=len(f))
            for k in (1, 8, 40):
                n, t1 = 127 * k, a.t0 - 1
                ms = [eng.trade_session_state_series(a.t0 - n, 1, n, with_wait=False, with_time=True)[3]
                      for _ in range(a.reps + 1)][1:]
                live = (f["start"] < t1) & (f["finish"] > a.t0 - n) & (f["start"] != f["finish"])
                out[f"tiles{k}_kernel_ms"] = med(ms)
                out[f"tiles{k}_kernel_ms_all"] = ms
                out[f"tiles{k}_live"] = int(live.sum())
    else:
        with engine() as eng:
            eng.submit_jobs(streams)
            eng.run()
            ts = eng.trade_stats()
            n = ts["t_final"] // 5 + 3
            ser = [eng.dtrade_state_series(0, 5, n, with_time=True)[3] for _ in range(a.reps + 1)][1:]
            sha = hashlib.sha256()
            for arr in eng.dtrade_state_series(0, 5, n):
                sha.update(arr.tobytes())
            out["sha256"] = sha.hexdigest()
            nowait = [eng.dtrade_state_series(0, 5, n, with_wait=False, with_time=True)[3] for _ in range(a.reps + 1)][1:]
            out.update(n_samples=n, series_kernel_ms=med(ser), series_kernel_ms_all=ser,
                       series_nowait_kernel_ms=med(nowait), n_foreign=len(eng.foreign()))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
