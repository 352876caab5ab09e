#!/usr/bin/env python3
"""Device time of mcs_level1_series (csrc/mcs_level1.hip, DESIGN.md §13, profiles/level1_series/)
beside mcs_wait_time_series, the nearest existing post-pass, on one DELAY run of the C4 shape
(--clusters x --nodes nodes x --jobs jobs, scaled arrivals at 90 % load, or --lam per second with
durations U{0..--max-dur - 1}: `--lam 0.95 --max-dur 972` is the Level1-heavy stream of bench.py).

One run; then per period (--periods, default 10 = trader_period_s and 5) the samples from 0 past the
largest t_end: a warm-up call and --reps timed calls of each series, interleaved in this one process.
Every figure is the call's kernel_ms (HIP events on the engine stream, summed over its launches).
Checks on the way: the sample past every t_end holds l1_left, and the largest len of a cluster at
period 1 would be peak_l1 (here: no sampled len exceeds it).  One JSON object on stdout, and in --out
when given.  Under `rocprofv3 --kernel-trace --stats -- python tools/level1_series_bench.py --reps 1
--periods 10` the per-kernel split is the trace's (level1_summary_kernel, level1_series_kernel and
wait_prep_kernel against the wait_*_kernels)."""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "multi-cluster-simulator_amd"))


def spread(xs):
    return dict(median_ms=statistics.median(xs), min_ms=min(xs), max_ms=max(xs), runs_ms=xs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clusters", type=int, default=4096)
    ap.add_argument("--nodes", type=int, default=256)
    ap.add_argument("--jobs", type=int, default=16384)
    ap.add_argument("--load", type=float, default=0.9)
    ap.add_argument("--lam", type=float, default=0.0)
    ap.add_argument("--max-dur", type=int, default=600)
    ap.add_argument("--periods", type=int, nargs="+", default=[10, 5])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()

    from mcs_amd import Engine, GenParams, replicate, uniform_cluster
    from mcs_amd.engine import scaled_lambda

    with Engine(0, policy="DELAY") as eng:
        eng.load_clusters(replicate(uniform_cluster(a.nodes), a.clusters))
        lam = a.lam or scaled_lambda(a.nodes, load=a.load)
        eng.generate_jobs(GenParams(arrival_mode=1, lam=lam, max_dur_s=a.max_dur), a.jobs)  # tools/bench_wait.py's run
        st = eng.run()
        cs, ds = eng.cluster_stats(), eng.delay_stats()
        t_end = int(cs["t_end"].max())
        res = dict(clusters=a.clusters, nodes=a.nodes, jobs_per_cluster=a.jobs, lam=lam, max_dur=a.max_dur,
                   run_kernel_ms=st.kernel_ms, handed_over=st.handed_over, t_end_max=t_end,
                   level1_moved_frac=float(ds["moved_l1"].sum()) / eng.num_jobs,
                   level1_peak=int(ds["peak_l1"].max()), periods={})
        for period in a.periods:
            n = t_end // period + 2
            samples = eng.level1_series(0, period, n)  # warm-up
            eng.wait_time_series(0, period, n)
            assert (samples["len"][:, -1] == ds["l1_left"]).all()
            assert (samples["len"].max(axis=1) <= ds["peak_l1"]).all()
            level1, wait = [], []
            for _ in range(max(a.reps, 1)):
                level1.append(eng.level1_series(0, period, n, with_time=True)[1])
                wait.append(eng.wait_time_series(0, period, n, with_time=True)[1])
            mult = (samples["len"] > 0) & (samples["len"] % 20 == 0)
            res["periods"][str(period)] = dict(
                samples_per_cluster=n, level1_series=spread(level1), wait_series=spread(wait),
                ratio=statistics.median(level1) / statistics.median(wait),
                mean_len=float(samples["len"].mean()), max_len=int(samples["len"].max()),
                nonempty_frac=float((samples["len"] > 0).mean()), walked_frac=float(mult.mean()),
                small_time_nonzero_frac=float((samples["small_time_s"] != 0).mean()))
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
