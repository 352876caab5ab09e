#!/usr/bin/env python3
"""Device time of mcs_online_state_series (profiles/online_series/) on the C4 shape
(4096 clusters x 256 nodes x 16384 jobs, scaled arrivals at 90 % load), three modes:

  batch   the streams submitted and run as a batch; mcs_cluster_state_series (and, under DELAY,
          mcs_wait_time_series) at period 5 from 0 to the largest t_end.  MCS_LIB selects the library,
          so the same script measures the parent commit's build.
  online  the same streams appended in --slices slices (run(h) after each), then drained;
          mcs_online_state_series over the same samples, without and (DELAY) with the wait statistics.
  slice   a session advanced to 3/4 of the arrivals, then --live times: append the next 5 s of jobs,
          run(h + 5), and one call over the 5 new seconds at period 1.  Run it under
          `rocprofv3 --kernel-trace --stats` for the share of the summary pre-pass and the wait
          prep/skip passes, which rescan the history.

Every timed figure is the call's kernel_ms (HIP events on the engine stream, summed over its
launches); a warm-up call precedes the --reps timed ones.  batch and online also print the SHA-256 of
the returned bytes: the two must agree.  One JSON object on stdout, and in --out when given."""
import argparse
import hashlib
import json
import os
import statistics
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "multi-cluster-simulator_amd"))

SEED = 0x4D43535F53494D31


def spread(xs):
    return dict(median_ms=statistics.median(xs), min_ms=min(xs), max_ms=max(xs), runs_ms=xs)


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        if a is not None:
            h.update(a.tobytes())
    return h.hexdigest()


def load(eng, args):
    from mcs_amd import GenParams, replicate, uniform_cluster
    from mcs_amd.engine import scaled_lambda

    eng.load_clusters(replicate(uniform_cluster(args.nodes), args.clusters))
    eng.generate_jobs(GenParams(seed=SEED, arrival_mode=1, lam=scaled_lambda(args.nodes, load=0.9)), args.jobs)


def cut(streams, lo, hi):
    """the jobs of every cluster with lo <= arrival < hi, as an appended batch (CSR)"""
    from mcs_amd import JobStreams

    m = (streams.arrival >= lo) & (streams.arrival < hi)
    csum = np.concatenate([[0], np.cumsum(m, dtype=np.uint64)])
    return JobStreams(*(getattr(streams, f)[m] for f in ("arrival", "dur", "cores", "mem")),
                      csum[streams.job_off.astype(np.int64)].astype(np.uint64))


def host_streams(args):
    """the generated streams on the host (a second engine materialises them)"""
    from mcs_amd import Engine

    with Engine(0, policy=args.policy) as eng:
        load(eng, args)
        return eng.read_jobs()


def n_samples(eng):
    return int(eng.cluster_stats()["t_end"].max()) // 5 + 1


def batch(args):
    from mcs_amd import Engine
    from mcs_amd import _lib as L

    delay = args.policy == "DELAY"
    with Engine(0, policy=args.policy) as eng:
        load(eng, args)
        st = eng.run()
        n = n_samples(eng)
        samples, first = eng.cluster_state_series(0, 5, n)  # warm-up
        wait = eng.wait_time_series(0, 5, n) if delay else None
        res = dict(mode="batch", lib=os.path.basename(L.LIB_PATH), run_kernel_ms=st.kernel_ms, n_samples=n,
                   sha256=digest(samples, wait, first),
                   series=spread([eng.cluster_state_series(0, 5, n, with_time=True)[2] for _ in range(args.reps)]))
        if delay:
            res["wait"] = spread([eng.wait_time_series(0, 5, n, with_time=True)[1] for _ in range(args.reps)])
    return res


def online(args):
    from mcs_amd import Engine
    from mcs_amd import _lib as L

    delay = args.policy == "DELAY"
    streams = host_streams(args)
    top = int(streams.arrival.max()) + 1
    hs = [top * k // args.slices for k in range(1, args.slices)]
    with Engine(0, policy=args.policy) as eng:
        load_clusters_only(eng, args)
        prev, run_ms = 0, 0.0
        for h in hs:
            eng.append_jobs(cut(streams, prev, h))
            run_ms += eng.run(h).kernel_ms
            prev = h
        eng.append_jobs(cut(streams, prev, 1 << 32))
        run_ms += eng.run().kernel_ms
        n = n_samples(eng)
        samples, wait, first = eng.online_state_series(0, 5, n)  # warm-up
        res = dict(mode="online", lib=os.path.basename(L.LIB_PATH), horizons=hs, run_kernel_ms=run_ms, n_samples=n,
                   sha256=digest(samples, wait, first),
                   series=spread([eng.online_state_series(0, 5, n, with_wait=False, with_time=True)[3]
                                  for _ in range(args.reps)]))
        if delay:
            both = [eng.online_state_series(0, 5, n, with_time=True)[3] for _ in range(args.reps)]
            res["series_and_wait"] = spread(both)
            res["wait_ms"] = statistics.median(both) - res["series"]["median_ms"]
    return res


def load_clusters_only(eng, args):
    from mcs_amd import replicate, uniform_cluster

    eng.load_clusters(replicate(uniform_cluster(args.nodes), args.clusters))


def live_slice(args):
    from mcs_amd import Engine
    from mcs_amd import _lib as L

    streams = host_streams(args)
    h = (int(streams.arrival.max()) + 1) * 3 // 4
    with Engine(0, policy=args.policy) as eng:
        load_clusters_only(eng, args)
        eng.append_jobs(cut(streams, 0, h))
        eng.run(h)
        eng.online_state_series(h - 5, 1, 5)  # warm-up
        calls, runs = [], []
        for _ in range(args.live):
            eng.append_jobs(cut(streams, h, h + 5))
            runs.append(eng.run(h + 5).kernel_ms)
            calls.append(eng.online_state_series(h, 1, 5, with_time=True)[3])
            h += 5
        res = dict(mode="slice", lib=os.path.basename(L.LIB_PATH), horizon_s=h, jobs_in_session=int(eng.num_jobs),
                   live_calls=args.live, run_5s=spread(runs), series_5s=spread(calls))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["batch", "online", "slice"])
    ap.add_argument("--policy", choices=["FIFO", "DELAY"], default="FIFO")
    ap.add_argument("--clusters", type=int, default=4096)
    ap.add_argument("--nodes", type=int, default=256)
    ap.add_argument("--jobs", type=int, default=16384)
    ap.add_argument("--slices", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--live", type=int, default=5)
    ap.add_argument("--out")
    args = ap.parse_args()
    res = {"batch": batch, "online": online, "slice": live_slice}[args.mode](args)
    res.update(policy=args.policy, clusters=args.clusters, nodes=args.nodes, jobs_per_cluster=args.jobs, period_s=5)
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
