#!/usr/bin/env python3
"""Cost of trading sessions (DESIGN.md §14 "Trading sessions") on the C5-DELAY system of
`bench.py --config c5 --policy delay` (64 cluster_small replicas x 2000 jobs, the reference client's
arrivals).  kernel_ms from HIP events (mcs_stats), each figure the median of --reps after a warm-up;
prints one JSON line.

  --mode slice     a session run to second --t0 (6000), then --slices (40) slices of --step (5) s:
                   append the slice's jobs, mcs_run(h + step); median kernel_ms and wall time of a slice,
                   the ticks it executed, and the replayed loop's own cost per tick
  --mode whole     the whole run in 10 and in 1000 slices against the batch run, all on the replayed
                   kernels (MCS_DT_RESIDENT=0 is set by this tool)
  --mode yardstick the only way to the state of a slice without sessions: a batch run with
                   t_max_s = t0 + slices * step - 1 from t = 0 (runs on a build without sessions too)
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "multi-cluster-simulator_amd")]


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["slice", "whole", "yardstick"], required=True)
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
    if a.mode == "whole":
        os.environ["MCS_DT_RESIDENT"] = "0"
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

    out = {"mode": a.mode, "clusters": a.clusters, "jobs_per_cluster": a.jobs_per_cluster, "reps": a.reps}
    if a.mode == "yardstick":
        h = a.t0 + a.slices * a.step
        with engine(t_max_s=h - 1) as eng:
            eng.submit_jobs(streams)
            ms = [eng.run().kernel_ms for _ in range(a.reps + 1)][1:]
            ts = eng.trade_stats()
        out.update(t_max_s=h - 1, kernel_ms=med(ms), kernel_ms_all=ms, ticks=ts["ticks"], loop_form=ts["loop_form"])
    elif a.mode == "slice":
        hs = [a.t0 + a.step * (i + 1) for i in range(a.slices)]
        chunks = [part(h - a.step, h) for h in hs]
        first = part(0, a.t0)
        per_rep = []
        with engine() as eng:
            eng.submit_jobs(first)
            for rep in range(a.reps + 1):
                eng.rewind()  # (the appended jobs stay: the first pass appends, the later ones only slice)
                st0 = eng.run(a.t0)
                t0_ticks = eng.trade_session_info()["ticks_total"]
                kms, wall, ticks, app = [], [], [], []
                for h, ch in zip(hs, chunks):
                    w = time.perf_counter()
                    if rep == 0:
                        eng.append_jobs(ch)
                    w1 = time.perf_counter()
                    st = eng.run(h)
                    wall.append((time.perf_counter() - w1) * 1e3)
                    app.append((w1 - w) * 1e3)
                    kms.append(st.kernel_ms)
                    ticks.append(eng.trade_session_info()["ticks_last_run"])
                per_rep.append(dict(to_t0_kernel_ms=st0.kernel_ms, to_t0_ticks=t0_ticks, slice_kernel_ms=med(kms),
                                    slice_wall_ms=med(wall), slice_ticks=med(ticks), append_wall_ms=med(app),
                                    slice_us_per_tick=1e3 * sum(kms) / max(sum(ticks), 1)))
            restarts = eng.trade_session_info()["restarts"]
        first_rep, reps = per_rep[0], per_rep[1:]
        out.update({k: med([r[k] for r in reps]) for k in reps[0]})
        out.update(append_wall_ms=first_rep["append_wall_ms"], restarts=restarts,
                   loop_us_per_tick=1e3 * out["to_t0_kernel_ms"] / max(out["to_t0_ticks"], 1),
                   slice_kernel_ms_all=[r["slice_kernel_ms"] for r in reps])
    else:
        tf = int(streams.arrival.max()) + 1
        with engine() as eng:
            eng.submit_jobs(streams)
            ms = [eng.run().kernel_ms for _ in range(a.reps + 1)][1:]
            ts = eng.trade_stats()
        out.update(batch_kernel_ms=med(ms), batch_kernel_ms_all=ms, ticks=ts["ticks"], loop_form=ts["loop_form"])
        from mcs_amd import MCSError

        for n in (10, 1000) if a.slices else ():  # (--slices 0: the batch figure alone)
            hs = sorted({int(x) for x in np.linspace(0, tf, n + 1)[1:]})
            tot = []
            with engine() as eng:
                eng.submit_jobs(streams)
                try:
                    eng.rewind()
                except MCSError:  # a build without trading sessions: the batch figure alone
                    out["sessions"] = "refused"
                    break
                for _ in range(a.reps + 1):
                    eng.rewind()
                    k = sum(eng.run(h).kernel_ms for h in hs)
                    tot.append(k + eng.run().kernel_ms)
                info = eng.trade_session_info()
            out[f"slices{n}_kernel_ms"] = med(tot[1:])
            out[f"slices{n}_kernel_ms_all"] = tot[1:]
            out[f"slices{n}_ticks"] = info["ticks_total"]
            out[f"slices{n}_restarts"] = info["restarts"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
