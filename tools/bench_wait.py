"""Measure the average wait time series (csrc/mcs_wait.hip, mcs_wait_time_series) on a DELAY run of
the C4 shape: --clusters x --nodes nodes x --jobs-per-cluster jobs, scaled arrivals at --load (or
--lam per second, with durations U{0..--max-dur - 1}).  One run, then --steps calls of the series
every --period seconds from 0 to the largest t_end; prints one JSON line with the median kernel ms
(HIP events, summed over the call's launches), the Level1 share of the run and the algorithmic
bytes: per job 28 B read by the scan (record, node, start) and 24 B of scratch written once, per chunk
the 16 B scratch record read again, and 24 B per sample written."""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "multi-cluster-simulator_amd"))
from mcs_amd import Engine, GenParams, replicate, uniform_cluster  # noqa: E402
from mcs_amd.engine import scaled_lambda  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--clusters", type=int, default=4096)
ap.add_argument("--nodes", type=int, default=256)
ap.add_argument("--jobs-per-cluster", type=int, default=16384)
ap.add_argument("--load", type=float, default=0.9)
ap.add_argument("--lam", type=float, default=0.0)
ap.add_argument("--max-dur", type=int, default=600)
ap.add_argument("--period", type=int, default=5)
ap.add_argument("--steps", type=int, default=5)
a = ap.parse_args()

with Engine(0, policy="DELAY") as eng:
    eng.load_clusters(replicate(uniform_cluster(a.nodes), a.clusters))
    lam = a.lam or scaled_lambda(a.nodes, load=a.load)
    eng.generate_jobs(GenParams(arrival_mode=1, lam=lam, max_dur_s=a.max_dur), a.jobs_per_cluster)
    st = eng.run()
    cs, ds = eng.cluster_stats(), eng.delay_stats()
    n = int(cs["t_end"].max()) // a.period + 2
    eng.wait_time_series(0, a.period, n)  # warm-up
    ms = []
    for _ in range(max(a.steps, 1)):
        samples, k = eng.wait_time_series(0, a.period, n, with_time=True)
        ms.append(k)
    # the last sample lies past every t_end: a drained cluster shows the run's final statistics
    drained = (cs["flags"] & 1) == 0
    assert (samples["total_wait_ms"][drained, -1] == ds["total_wait_ms"][drained]).all()
    assert (samples["jobs_count"][:, -1] == ds["jobs_count"]).all()
    jobs = eng.num_jobs
    chunks = -(-n // max(1, min(n, int(os.environ.get("MCS_SERIES_CHUNK", 0)) or (256 << 20) // (24 * a.clusters))))
    alg = (28.0 + 24.0 + 16.0 * chunks) * jobs + 24.0 * a.clusters * n
    med = float(np.median(ms))
    gbs = alg / (med / 1e3) / 1e9
    print(json.dumps({"kernel": "mcs::wait_*_kernel", "clusters": a.clusters, "nodes": a.nodes, "jobs": jobs,
                      "lam": lam, "max_dur": a.max_dur, "period_s": a.period, "samples_per_cluster": n,
                      "chunks": chunks, "kernel_ms_median": med, "kernel_ms_min": min(ms), "kernel_ms_all": ms,
                      "run_kernel_ms": st.kernel_ms, "level1_moved_frac": float(ds["moved_l1"].sum()) / jobs,
                      "level1_placed": int(ds["placed_l1"].sum()), "level1_peak": int(ds["peak_l1"].max()),
                      "average_wait_s_at_end": float(samples["average_wait_time"][:, -1].mean()) / 1e3,
                      "algorithmic_bytes": alg,
                      "roofline": {"bound": "hbm", "achieved": gbs, "peak": 8000.0, "unit": "GB/s",
                                   "frac": gbs / 8000.0}}), flush=True)
