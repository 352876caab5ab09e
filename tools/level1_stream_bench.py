#!/usr/bin/env python3
"""Device time of the Level1 samples on a cursor against the Level1 series call for the same live slice
(DESIGN.md §14 "Level1 on the cursors", profiles/level1_stream/).

  --system c4   the C4 shape (4096 clusters x 256 nodes x 16384 jobs, scaled arrivals at 90 % load, DELAY),
                a plain session advanced to 3/4 of the arrivals: mcs_stream_next_level1 against
                mcs_online_level1_series
  --system c5   C5-DELAY (`bench.py --config c5 --policy delay`: 64 cluster_small replicas x 2000 jobs, the
                reference client's arrivals), a trading session run to second 6000:
                mcs_trade_stream_next_level1 against mcs_trade_session_level1_series

Per slice: append the next 5 s of jobs, mcs_run(h + 5), five samples at period 1.

  --mode cursor  a stream opened with Level1 300 s below the horizon (the first call catches up once), then
                 --warm untimed and --live timed slices: the call's kernel_ms, its Level1 share
                 (mcs_level1_stream_stats.kernel_ms) and the rows its Level1 scans loaded; the series call
                 for the same seconds in the same process, whose bytes must agree.  Then the stream is
                 closed and opened again without Level1, and the same number of slices gives
                 mcs_stream_next without Level1.
  --mode series  the series call alone on the same slices: runs on a build without the cursor's Level1 too
                 (the yardstick from a checkout of the parent, in alternating processes).

Every figure is a kernel_ms from HIP events on the engine stream; medians over the timed slices.  Both
modes print the SHA-256 of the Level1 bytes of the timed and untimed slices together.  One JSON object on
stdout, and in --out when given."""
import argparse
import hashlib
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "multi-cluster-simulator_amd"))
sys.path.insert(0, os.path.join(REPO, "tools"))


def spread(xs):
    return dict(median_ms=statistics.median(xs), min_ms=min(xs), max_ms=max(xs), runs_ms=xs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--system", choices=["c4", "c5"], required=True)
    ap.add_argument("--mode", choices=["cursor", "series"], required=True)
    ap.add_argument("--clusters", type=int)
    ap.add_argument("--nodes", type=int, default=256)
    ap.add_argument("--jobs", type=int)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--live", type=int, default=7)
    ap.add_argument("--out")
    args = ap.parse_args()
    args.policy = "DELAY"
    trade = args.system == "c5"
    args.clusters = args.clusters or (64 if trade else 4096)
    args.jobs = args.jobs or (2000 if trade else 16384)

    import numpy as np

    from mcs_amd import Cluster, Engine, GenParams, JobStreams, replicate
    from mcs_amd import _lib as L
    from mcs_amd.engine import gen_streams_host

    if trade:
        arrays = replicate(Cluster.load(os.path.join(REPO, "assets", "cluster_small.json")), args.clusters)
        streams = gen_streams_host(GenParams(seed=0x4D43535F53494D31), arrays, args.jobs)
        h = 6000
        eng = Engine(0, policy="DELAY", trader=True)
        eng.load_clusters(arrays)
    else:
        from online_series_bench import host_streams, load_clusters_only

        streams = host_streams(args)
        h = (int(streams.arrival.max()) + 1) * 3 // 4
        eng = Engine(0, policy="DELAY")
        load_clusters_only(eng, args)

    def cut(lo, hi):
        m = (streams.arrival >= lo) & (streams.arrival < hi)
        csum = np.concatenate([[0], np.cumsum(m, dtype=np.uint64)])
        return JobStreams(*(getattr(streams, f)[m] for f in ("arrival", "dur", "cores", "mem")),
                          csum[streams.job_off.astype(np.int64)].astype(np.uint64))

    def advance(h):
        new = cut(h, h + 5)
        if len(new.arrival):  # (late in a run every job has arrived)
            eng.append_jobs(new)
        return eng.run(h + 5).kernel_ms

    series = eng.trade_session_level1_series if trade else eng.online_level1_series
    res = dict(system=args.system, mode=args.mode, lib=os.path.basename(L.LIB_PATH), clusters=args.clusters,
               jobs_per_cluster=args.jobs, warm=args.warm, live=args.live)
    sha_series, sha_cursor = hashlib.sha256(), hashlib.sha256()
    with eng:
        eng.append_jobs(cut(0, h))
        eng.run(h)
        series(h - 5, 1, 5)  # warm-up
        n_slices = args.warm + args.live
        if args.mode == "series":
            ser, runs = [], []
            for k in range(n_slices):
                run_ms = advance(h)
                got, ms = series(h, 1, 5, with_time=True)
                sha_series.update(got.tobytes())
                if k >= args.warm:
                    ser.append(ms)
                    runs.append(run_ms)
                h += 5
            res.update(series_5s=spread(ser), run_5s=spread(runs), sha256_level1=sha_series.hexdigest())
        else:
            s_open = eng.trade_stream_open if trade else eng.stream_open
            s_next = eng.trade_stream_next if trade else eng.stream_next
            s_close = eng.trade_stream_close if trade else eng.stream_close
            s_open(h - 300, 1, True, with_level1=True)
            _, _, _, st = s_next(300)
            assert st["n_written"] == 300 and st["pending"] == 0, st
            res["catch_up_300s"] = dict(kernel_ms=st["kernel_ms"], level1_kernel_ms=st["level1_kernel_ms"],
                                        rows_scanned=st["rows_scanned"], level1_rows_scanned=st["level1_rows_scanned"])
            nexts, shares, rows, ser, runs, lens = [], [], [], [], [], []
            for k in range(n_slices):
                run_ms = advance(h)
                _, _, l1, st = s_next(5)
                assert st["n_written"] == 5 and st["t_first"] == h and st["pending"] == 0, st
                got, ms = series(h, 1, 5, with_time=True)
                assert got.tobytes() == l1.tobytes(), f"slice at {h}: the cursor's Level1 bytes differ from the series call's"
                sha_series.update(got.tobytes())
                sha_cursor.update(l1.tobytes())
                if k >= args.warm:
                    nexts.append(st["kernel_ms"])
                    shares.append(st["level1_kernel_ms"])
                    rows.append(st["level1_rows_scanned"])
                    ser.append(ms)
                    runs.append(run_ms)
                    lens.append(int(l1["len"].sum()))
                h += 5
            s_close()
            s_open(h, 1, True)  # the same slices again on a stream without Level1
            plain = []
            for k in range(n_slices):
                advance(h)
                _, _, st = s_next(5)
                assert st["n_written"] == 5 and st["pending"] == 0, st
                if k >= args.warm:
                    plain.append(st["kernel_ms"])
                h += 5
            res.update(next_with_level1_5s=spread(nexts), level1_share_5s=spread(shares), series_5s=spread(ser),
                       next_without_level1_5s=spread(plain), run_5s=spread(runs), level1_rows_scanned=rows,
                       level1_members_in_slice=lens, rows_held=int(eng.job_offsets()[-1]),
                       sha256_level1=sha_series.hexdigest(), sha256_level1_cursor=sha_cursor.hexdigest())
        res["horizon_s"] = h
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
