#!/usr/bin/env python3
"""Measurements for mcs_dtrade_state_series (profiles/dtrade_state/), two modes:

  c5delay  the C5-DELAY system of `bench.py --config c5 --policy delay` (64 cluster_small clusters x
           2000 jobs, the same seed): the Foreign-log size, the device time of the series at period 5
           over the run (HIP events, the call's kernel_ms) without and with the wait statistics, and,
           for context, mcs_cluster_state_series and mcs_wait_time_series after a plain DELAY run of
           the same streams.  There is no pre-pass: the kernels scan the Foreign log as it is.
  bytes    SHA-256 of what the plain and the FIFO-trading state calls return for one seeded workload
           (six 64-node clusters at 120 % load, 250 jobs each): run once per build with MCS_LIB and
           compare, the plain and TRADE instantiations must not change a byte.

tools/trade_state_bench.py plain/merge measures the plain C4 series of two builds.
One JSON object on stdout, and in --out when given."""
import argparse
import hashlib
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "multi-cluster-simulator_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))

SEED = 0x4D43535F53494D31


def spread(xs):
    return dict(median_ms=statistics.median(xs), min_ms=min(xs), max_ms=max(xs), runs_ms=xs)


def c5delay(args):
    import numpy as np

    from mcs_amd import Cluster, Engine, GenParams, replicate

    clusters, jobs = args.clusters or 64, args.jobs or 2000
    spec = Cluster.load(os.path.join(REPO, "assets", "cluster_small.json"))
    res = dict(what="C5-DELAY state series", clusters=clusters, jobs_per_cluster=jobs, period_s=5)
    with Engine(0, policy="DELAY", trader=True) as eng:
        eng.load_clusters(replicate(spec, clusters))
        eng.generate_jobs(GenParams(seed=SEED), jobs)
        st = eng.run()
        ts, f = eng.trade_stats(), eng.foreign()
        node, start, fin = eng.placements()
        t_last = max(int(ts["t_final"]), int(fin[node >= 0].max()), int(f["finish"].max(initial=0)))
        n = t_last // 5 + 1
        nv = [len(eng.virtual_node_caps(c)) for c in range(clusters)]
        eng.dtrade_state_series(0, 5, n)  # warm-up
        series = [eng.dtrade_state_series(0, 5, n, with_wait=False, with_time=True)[3] for _ in range(args.reps)]
        both = [eng.dtrade_state_series(0, 5, n, with_time=True)[3] for _ in range(args.reps)]
        res.update(n_samples=n, t_final=int(ts["t_final"]), loop_form=int(ts["loop_form"]), run_kernel_ms=st.kernel_ms,
                   foreign_records=len(f), foreign_log_bytes=40 * len(f), foreign_holding=int((f["finish"] > f["start"] + 1).sum()),
                   foreign_per_responder_max=int(np.bincount(f["responder"], minlength=clusters).max()) if len(f) else 0,
                   virtual_nodes_max=max(nv), jobs_on_virtual_nodes=int((node >= 5).sum()), prepass_ms=None,
                   series=spread(series), series_and_wait=spread(both),
                   wait_ms=statistics.median(both) - statistics.median(series))
    with Engine(0, policy="DELAY") as eng:
        eng.load_clusters(replicate(spec, clusters))
        eng.generate_jobs(GenParams(seed=SEED), jobs)
        eng.run()
        eng.cluster_state_series(0, 5, n)
        eng.wait_time_series(0, 5, n)
        res["plain_delay_same_streams"] = dict(
            series=spread([eng.cluster_state_series(0, 5, n, with_time=True)[2] for _ in range(args.reps)]),
            wait=spread([eng.wait_time_series(0, 5, n, with_time=True)[1] for _ in range(args.reps)]))
    return res


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(a.tobytes())
    return h.hexdigest()


def state_bytes(args):
    from kat_util import seeded_workload
    from mcs_amd import Engine
    from mcs_amd import _lib as L

    arrays, streams, _ = seeded_workload("n64_hot", 6, 250)
    res = dict(what="state calls of one workload, SHA-256 of the returned bytes", lib=L.LIB_PATH, workload="n64_hot 6 x 250")
    for name, cfg in (("plain_fifo", dict(policy="FIFO")), ("plain_delay", dict(policy="DELAY")),
                      ("fifo_trading", dict(borrow=True, trader=True, t_max_s=20_000_000))):
        with Engine(0, **cfg) as eng:
            eng.load_clusters(arrays)
            eng.submit_jobs(streams)
            eng.run()
            node, start, fin = eng.placements()
            n = int(fin[node >= 0].max()) + 6
            out = [*eng.cluster_state_series(0, 1, n), *eng.cluster_state_series(2, 5, n // 5), eng.cluster_states(n // 2)]
            if name == "plain_delay":
                out.append(eng.wait_time_series(0, 1, n))
            res[name] = digest(node, start, fin, *out)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["c5delay", "bytes"])
    ap.add_argument("--clusters", type=int, default=0)
    ap.add_argument("--jobs", type=int, default=0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out")
    args = ap.parse_args()
    res = {"c5delay": c5delay, "bytes": state_bytes}[args.mode](args)
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
