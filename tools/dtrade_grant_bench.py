#!/usr/bin/env python3
"""Cost of the external traders' calls (DESIGN.md §14 "External traders") on the C5-DELAY system of
`bench.py --config c5 --policy delay` (64 cluster_small replicas x 2000 jobs, the reference client's
arrivals) in external mode: a session run to second --t0 (6000), then --slices (40) slices of --step (5) s.
After every slice's mcs_run(h + step): a provide call of 8 requests, one of 64 and a receive call of 8,
each timed next to the slice itself in the same process (kernel_ms from HIP events, wall time around the
call).  Each figure is the median over the slices of the last --reps passes after a warm-up pass; the
yardstick is the slice, re-measured here, not the grant call itself.  Prints one JSON line.

The requests are small ({1, 100} for 1 s: exhausted at row 0, one Foreign job each) and go to distinct
responders, the received nodes are {0, 0}: the calls' fixed cost, which is what a trader pays per slice."""
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
    ap.add_argument("--clusters", type=int, default=64)
    ap.add_argument("--jobs-per-cluster", type=int, default=2000)
    ap.add_argument("--t0", type=int, default=6000)
    ap.add_argument("--step", type=int, default=5)
    ap.add_argument("--slices", type=int, default=40)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=lambda s: int(s, 0), default=0x4D43535F53494D31)
    return ap.parse_args()


def main():
    a = parse()
    import numpy as np

    from mcs_amd import VNODE_GRANT_DTYPE, VNODE_REQUEST_DTYPE, Cluster, Engine, GenParams, replicate
    from mcs_amd.engine import gen_streams_host

    arrays = replicate(Cluster.load(os.path.join(REPO, "assets", "cluster_small.json")), a.clusters)
    streams = gen_streams_host(GenParams(seed=a.seed), arrays, a.jobs_per_cluster)
    C = a.clusters

    def requests(n):
        r = np.zeros(n, VNODE_REQUEST_DTYPE)
        r["responder"] = np.arange(n) % C
        r["requester"] = (np.arange(n) + 1) % C
        r["cores"], r["memory"], r["time_s"] = 1, 100, 1
        return r

    p8, p64 = requests(8), requests(64)
    r8 = np.zeros(8, VNODE_GRANT_DTYPE)
    r8["cluster"] = np.arange(8) % C
    hs = [a.t0 + a.step * (i + 1) for i in range(a.slices)]
    med = statistics.median
    keys = ("slice", "provide8", "provide64", "receive8")
    passes = []
    with Engine(0, policy="DELAY", trader=True) as eng:
        eng.load_clusters(arrays)
        eng.submit_jobs(streams)
        eng.trade_external(True)
        for rep in range(a.reps + 1):
            eng.rewind()
            eng.run(a.t0)
            k = {x: [] for x in keys}
            w = {x: [] for x in keys}
            for h in hs:
                t = time.perf_counter()
                st = eng.run(h)
                w["slice"].append((time.perf_counter() - t) * 1e3)
                k["slice"].append(st.kernel_ms)
                for name, fn, arg in (("provide8", eng.provide_virtual_nodes, p8),
                                      ("provide64", eng.provide_virtual_nodes, p64),
                                      ("receive8", eng.receive_virtual_nodes, r8)):
                    t = time.perf_counter()
                    res = fn(arg)
                    w[name].append((time.perf_counter() - t) * 1e3)
                    k[name].append((res[1] if isinstance(res, tuple) else res)["kernel_ms"])
            passes.append(({x: med(k[x]) for x in keys}, {x: med(w[x]) for x in keys}))
            info = eng.trade_session_info()
    out = {"clusters": C, "jobs_per_cluster": a.jobs_per_cluster, "slices": a.slices, "reps": a.reps,
           "restarts": info["restarts"]}
    for x in keys:
        out[f"{x}_kernel_ms"] = med([p[0][x] for p in passes[1:]])
        out[f"{x}_wall_ms"] = med([p[1][x] for p in passes[1:]])
    for x in keys[1:]:
        out[f"{x}_over_slice_kernel"] = out[f"{x}_kernel_ms"] / out["slice_kernel_ms"]
        out[f"{x}_over_slice_wall"] = out[f"{x}_wall_ms"] / out["slice_wall_ms"]
    out.update(provide_launches=2, provide_syncs=1, receive_launches=1, receive_syncs=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
