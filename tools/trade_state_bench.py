#!/usr/bin/env python3
"""Device time of mcs_cluster_state_series (HIP events, the call's kernel_ms), two measurements:

  plain  the C4 shape (4096 clusters x 256 nodes x 16384 jobs, FIFO, no trading), period 5 from 0 to
         the largest finish: the plain kernels, which must not move when the trading variant changes.
         MCS_LIB selects the library, so the same script measures two builds; --merge folds the
         interleaved runs of two builds into profiles/trade_state/bench_plain_series.json.
  c5     the C5 shape (64 clusters x 256 nodes, FIFO with borrow and trader): the lent-run pre-pass
         and the series at period 5 over the run, next to the same call after a plain FIFO run of the
         same streams.

One JSON object on stdout, and in --out when given."""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "multi-cluster-simulator_amd"))

SEED = 0x4D43535F53494D31


def spread(xs):
    return dict(median_ms=statistics.median(xs), min_ms=min(xs), max_ms=max(xs), runs_ms=xs)


def series_times(eng, n, reps):
    out = []
    for _ in range(reps):
        out.append(eng.cluster_state_series(0, 5, n, with_time=True)[2])
    return out


def load(eng, clusters, nodes, jobs, load_factor=0.9):
    from mcs_amd import GenParams, replicate, uniform_cluster
    from mcs_amd.engine import scaled_lambda

    eng.load_clusters(replicate(uniform_cluster(nodes), clusters))
    eng.generate_jobs(GenParams(seed=SEED, arrival_mode=1, lam=scaled_lambda(nodes, load=load_factor)), jobs)


def plain(args):
    from mcs_amd import Engine
    from mcs_amd import _lib as L

    with Engine(0, policy="FIFO") as eng:
        load(eng, args.clusters or 4096, 256, args.jobs or 16384)
        eng.run()
        t_end = int(eng.cluster_stats()["t_end"].max())
        n = t_end // 5 + 1
        series_times(eng, n, 1)  # warm-up
        ts = series_times(eng, n, args.reps)
    return dict(what="plain C4 series", lib=L.LIB_PATH, clusters=args.clusters or 4096, jobs_per_cluster=args.jobs or 16384,
                period_s=5, n_samples=n, **spread(ts))


def c5(args):
    import numpy as np

    from mcs_amd import Engine

    clusters, jobs = args.clusters or 64, args.jobs or 156250
    res = dict(what="C5 series", clusters=clusters, nodes=256, jobs_per_cluster=jobs, period_s=5)
    with Engine(0, borrow=True, trader=True) as eng:
        load(eng, clusters, 256, jobs)
        st = eng.run()
        ts = eng.trade_stats()
        node, start, fin = eng.placements()
        t_last = max(int(ts["t_final"]), int(fin[node >= 0].max()), int(eng.lent()["finish"].max(initial=0)))
        n = t_last // 5 + 1
        first = eng.cluster_state_series(0, 5, n, with_time=True)[2]  # builds the lent-run lists
        rest = series_times(eng, n, args.reps)
        res.update(n_samples=n, lent_runs=int(ts["lent_runs"]), borrowed=int(ts["borrowed"]), run_kernel_ms=st.kernel_ms,
                   trading=dict(first_call_ms=first, prepass_ms=first - statistics.median(rest), **spread(rest)))
        del node, start, fin
    with Engine(0, policy="FIFO") as eng:
        load(eng, clusters, 256, jobs)
        eng.run()
        series_times(eng, n, 1)
        res["plain_fifo_same_streams"] = spread(series_times(eng, n, args.reps))
    return res


def merge(args):
    runs = [json.load(open(p)) for p in args.merge]
    by = {}
    for r in runs:
        by.setdefault(os.path.basename(os.path.dirname(r["lib"])) + "/" + os.path.basename(r["lib"]), []).append(r)
    out = dict(what="plain C4 series, interleaved runs of two builds", period_s=5, n_samples=runs[0]["n_samples"], builds={})
    for k, rs in by.items():
        meds = [r["median_ms"] for r in rs]
        out["builds"][k] = dict(median_of_run_medians_ms=statistics.median(meds), run_medians_ms=meds,
                                min_ms=min(r["min_ms"] for r in rs), max_ms=max(r["max_ms"] for r in rs),
                                runs_ms=[r["runs_ms"] for r in rs])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["plain", "c5", "merge"])
    ap.add_argument("--clusters", type=int, default=0)
    ap.add_argument("--jobs", type=int, default=0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out")
    ap.add_argument("--merge", nargs="*", default=[])
    args = ap.parse_args()
    res = {"plain": plain, "c5": c5, "merge": merge}[args.mode](args)
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
