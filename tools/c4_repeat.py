"""BASELINE config 4 at full size (tests/test_gpu_parity.py::test_config4_full_size_parity's launch), repeated
in one engine on the same generated stream: counts the launches whose outputs differ from the first one's or
break finish = start + duration, and prints where.  A launch that differs is read a second time (a differing
second read would be the copy, not the kernel) and its first bad cluster is compared with the oracle.

usage: python tools/c4_repeat.py [launches]      (one MI355X; about 0.7 s per launch)"""
import os, sys, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))  # tools/..
sys.path[:0] = [os.path.join(REPO, "multi-cluster-simulator_amd"), os.path.join(REPO, "tests")]
import numpy as np
import oracle_ref as O
from mcs_amd import Engine, GenParams, replicate, uniform_cluster
from mcs_amd.engine import scaled_lambda

n, J = 4096, 16384
arrays = replicate(uniform_cluster(256), n)
gp = GenParams(seed=0x4D43535F53494D31, arrival_mode=1, lam=scaled_lambda(256, load=0.9))
eng = Engine(0)
first = None
REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 3
nbad = 0
for rep in range(REPS):
    t0 = time.time()
    eng.load_clusters(arrays)
    eng.generate_jobs(gp, J)
    st = eng.run()
    node, start, fin = eng.placements()
    jobs = eng.read_jobs()
    bad = np.nonzero(fin != start + jobs.dur)[0]
    if first is not None and bad.size == 0 and all(np.array_equal(a, b) for a, b in zip(first, (node, start, fin, jobs.dur, jobs.arrival))):
        if rep % 20 == 0:
            print(f'rep {rep} same as run 0', flush=True)
        continue
    nbad += rep > 0
    node2, start2, fin2 = eng.placements()
    jobs2 = eng.read_jobs()
    print(f"rep {rep}: kernel {eng.last_kernel} {st.kernel_ms:.3f} ms placed {st.placed} esc {st.escalations}", flush=True)
    for nm, a, b in (("node", node, node2), ("start", start, start2), ("fin", fin, fin2), ("dur", jobs.dur, jobs2.dur),
                     ("arrival", jobs.arrival, jobs2.arrival)):
        d = np.nonzero(a != b)[0]
        print(f"  second read of {nm}: {d.size} differences", d[:8], flush=True)
    bad = np.nonzero(fin != start + jobs.dur)[0]
    print(f"  fin != start + dur at {bad.size} rows", flush=True)
    if first is None:
        first = (node.copy(), start.copy(), fin.copy(), jobs.dur.copy(), jobs.arrival.copy())
    else:
        for nm, a, b in zip(("node", "start", "fin", "dur", "arrival"), first, (node, start, fin, jobs.dur, jobs.arrival)):
            d = np.nonzero(a != b)[0]
            print(f"  vs run 0, {nm}: {d.size} differences", d[:8], flush=True)
    if bad.size:
        c = int(bad[0] // J)
        print(f"  cluster {c}, jobs {bad[0] % J}..{bad[-1] % J}, clusters {np.unique(bad // J)}")
        sl = slice(c * J, (c + 1) * J)
        on, os_, of, _ = O.fifo_run(arrays.free_c[:256], arrays.free_m[:256], jobs.arrival[sl], jobs.dur[sl], jobs.cores[sl], jobs.mem[sl])
        for i in bad[:64]:
            k = i % J
            print(f"   job {k}: arr {jobs.arrival[i]} dur {jobs.dur[i]} gpu node {node[i]} start {start[i]} fin {fin[i]} | oracle {on[k]} {os_[k]} {of[k]}")
    print(f"  {time.time() - t0:.1f} s", flush=True)
print(f'{nbad} of {REPS} runs differ from run 0 or break fin = start + dur')
eng.close()
