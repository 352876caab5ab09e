"""Measure the ClusterState reduction (csrc/mcs_state.hip) on the C4 workload: one FIFO run of
4096 clusters x 256 nodes x 16384 jobs, then K launches of mcs_cluster_states at a mid-run second.
Algorithmic bytes per launch = 12 B per job scanned (node, start, finish) + 8 B per running job
(its cores and memory); prints one JSON line with the HBM roofline of the launch.

--series adds the time series (series_kernel, mcs_cluster_state_series) over the same run: samples
every --period seconds from 0 to the largest t_end, the median kernel ms of --series-steps calls,
the time the same samples take through the single call (its median launch ms x the sample count,
measured above in the same process), the algorithmic bytes (28 B per job + 16 B per sample) and
how often a job batch was read on average, computed on the host from the batch summaries."""
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
ap.add_argument("--jobs-per-cluster", type=int, default=16384)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--series", action="store_true")
ap.add_argument("--period", type=int, default=5)
ap.add_argument("--series-steps", type=int, default=5)
a = ap.parse_args()


def batch_reads(arrival, node, fin, n_nodes, period, n_samples, n_clusters):
    """Batch reads of one series call over batches: the tiles (series_tile samples each, restarting at
    every chunk the engine splits the call into) whose [t_first, t_last] meets a batch's
    [arrival_min, end_max) window; clusters of equal job counts that are multiples of 256."""
    ts = (min(78 * 1024 // (4 * (2 * n_nodes + 34)), 127) - 1) | 1  # series_tile, csrc/mcs_internal.h
    chunk = max(1, min(n_samples, int(os.environ.get("MCS_SERIES_CHUNK", 0)) or (256 << 20) // (16 * n_clusters)))
    amin = arrival.reshape(-1, 256).min(axis=1).astype(np.int64)
    emax = np.where(node >= 0, fin, 0xFFFFFFFF).reshape(-1, 256).max(axis=1).astype(np.int64)
    reads = 0
    for c0 in range(0, n_samples, chunk):
        for k0 in range(c0, min(c0 + chunk, n_samples), ts):
            k1 = min(k0 + ts, c0 + chunk, n_samples) - 1
            reads += int(((amin <= k1 * period) & (emax > k0 * period)).sum())
    return reads / len(amin), ts


with Engine(0) as eng:
    eng.load_clusters(replicate(uniform_cluster(256), a.clusters))
    eng.generate_jobs(GenParams(arrival_mode=1, lam=scaled_lambda(256, load=0.9)), a.jobs_per_cluster)
    eng.run()
    node, start, fin = eng.placements()
    t = int(np.median(start[node >= 0]))
    eng.cluster_states(t)  # warm-up
    ms = []
    for _ in range(a.steps):
        st, k = eng.cluster_states(t, with_time=True)
        ms.append(k)
    jobs = eng.num_jobs
    running = int(st["running"].sum())
    alg = 12.0 * jobs + 8.0 * running
    avg = sum(ms) / len(ms)
    gbs = alg / (avg / 1e3) / 1e9
    print(json.dumps({"kernel": "mcs::state_kernel", "clusters": a.clusters, "jobs": jobs, "t_s": t,
                      "running_jobs": running, "kernel_ms_avg": avg, "kernel_ms_min": min(ms),
                      "algorithmic_bytes_per_launch": alg, "records_per_s": a.clusters / (avg / 1e3),
                      "roofline": {"bound": "hbm", "achieved": gbs, "peak": 8000.0, "unit": "GB/s",
                                   "frac": gbs / 8000.0}}), flush=True)
    if a.series:
        assert a.jobs_per_cluster % 256 == 0
        single_ms = float(np.median(ms))
        n = int(eng.cluster_stats()["t_end"].max()) // a.period + 1
        eng.cluster_state_series(0, a.period, n)  # warm-up
        sms = []
        for _ in range(max(a.series_steps, 5)):
            samples, first, k = eng.cluster_state_series(0, a.period, n, with_time=True)
            sms.append(k)
        # spot check against the single call, in the same process
        for kk in (0, n // 3, n - 1):
            one = eng.cluster_states(kk * a.period)
            for f in ("cores_utilization", "memory_utilization", "running"):
                assert samples[f][:, kk].tobytes() == one[f].tobytes(), (f, kk)
        rr, ts = batch_reads(eng.read_jobs().arrival, node, fin, 256, a.period, n, a.clusters)
        med = float(np.median(sms))
        alg = 28.0 * jobs + 16.0 * a.clusters * n
        gbs = alg / (med / 1e3) / 1e9
        print(json.dumps({"kernel": "mcs::series_kernel", "clusters": a.clusters, "jobs": jobs, "period_s": a.period,
                          "samples_per_cluster": n, "tile_samples": ts, "kernel_ms_median": med,
                          "kernel_ms_min": min(sms), "kernel_ms_all": sms,
                          "single_call_ms_median": single_ms, "single_call_ms_x_samples": single_ms * n,
                          "speedup_vs_single_calls": single_ms * n / med,
                          "algorithmic_bytes": alg, "batch_reads_per_batch": rr,
                          "roofline": {"bound": "hbm", "achieved": gbs, "peak": 8000.0, "unit": "GB/s",
                                       "frac": gbs / 8000.0}}), flush=True)
