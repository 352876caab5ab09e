"""CPU tests that pin tests/wait_ref.py — the time-resolved WaitTime reference the GPU tests of
mcs_wait_time_series compare against — to the oracle and to hand-traced series, independently of any
kernel; and the host-side pieces of the feature (struct layout, wire.start_stream)."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import oracle_ref as O
import wait_ref as R
from kat_util import GOLDEN, REPO, fuzz_workload, kat_cluster, kat_expect, kat_streams
from mcs_amd import WAIT_SAMPLE_DTYPE, pack_clusters, wire
from mcs_amd import _lib as L

WAITS = (0, 1, 3, 10)


def small_system(rng, J=None):
    """1-6 nodes of 8 cores / 32 memory, a hot stream: gaps from {0, 0, 1, 1, 1, 2}, durations 0-40,
    requests up to a node, now and then one that fits no node."""
    nn = int(rng.integers(1, 7))
    J = int(rng.integers(1, 60)) if J is None else J
    fc, fm = np.full(nn, 8, np.uint32), np.full(nn, 32, np.uint32)
    arr = np.cumsum(rng.choice([0, 0, 1, 1, 1, 2], J)).astype(np.uint32)
    dur = rng.integers(0, 41, J).astype(np.uint32)
    cores, mem = rng.integers(0, 9, J).astype(np.uint32), rng.integers(0, 33, J).astype(np.uint32)
    if rng.random() < 0.3:
        cores[int(rng.integers(0, J))] = 9
    return fc, fm, arr, dur, cores, mem


def test_literal_equals_replay_over_the_oracle_starts():
    rng = np.random.default_rng(0x57414954)
    n_skips = n_unplaced = longest = 0
    for case in range(300):
        fc, fm, arr, dur, cores, mem = small_system(rng)
        W = WAITS[case % len(WAITS)]
        node, start, fin, st = O.delay_run(fc, fm, arr, dur, cores, mem, max_wait_s=W)
        T = max(int(st["t_end"]), int(arr.max())) + 4
        lit = R.literal(list(zip(fc, fm)), (arr, dur, cores, mem), W, T)
        rep = R.replay(arr, start, W, T)
        assert (lit["start"] == start).all(), case  # every placed job has started by T
        assert (lit["total_ms"] == rep["total_ms"]).all() and (lit["count"] == rep["count"]).all(), case
        assert lit["skips"] == rep["skips"], case
        n_skips += len(rep["skips"])
        longest = max(longest, rep["longest_skip_run"])
        n_unplaced += int((node < 0).sum())
    assert n_skips > 1000 and longest >= 2 and n_unplaced > 20


def test_replay_at_t_end_equals_the_oracle_statistics():
    """Every cluster, deadlocked ones included: TotalTime and JobsCount after iteration t_end."""
    rng = np.random.default_rng(0x54454E44)
    for W in WAITS:
        arrays, streams = fuzz_workload("w16s", 40 + W, n_clusters=12, J=250, blocking=True)
        node, start, fin, st = O.delay_run_batch(arrays, streams, n_threads=4, max_wait_s=W)
        assert (st["flags"] & 1).any() and not (st["flags"] & 1).all()
        for c in range(arrays.n_clusters):
            js = streams.of(c)
            t_end = int(st["t_end"][c])
            rep = R.replay(streams.arrival[js], start[js], W, t_end + 3)
            assert rep["total_ms"][t_end] == st["total_wait_ms"][c], (W, c)
            assert rep["count"][t_end] == st["jobs_count"][c], (W, c)
            left = int(st["l1_left"][c])
            assert R.steady_after(rep, streams.arrival[js], start[js], t_end + 3)
            assert len(rep["level1"]) == left
            # the loop continued: nothing more for a drained cluster, t - arrival per job left otherwise
            assert (np.diff(rep["total_ms"][t_end:]) == 1000 * left).all()
    for case in range(80):  # and on the hot small systems, where the D6 skips are
        fc, fm, arr, dur, cores, mem = small_system(rng, J=int(rng.integers(1, 300)))
        W = WAITS[case % len(WAITS)]
        node, start, fin, st = O.delay_run(fc, fm, arr, dur, cores, mem, max_wait_s=W)
        rep = R.replay(arr, start, W, int(st["t_end"]))
        assert rep["total_ms"][-1] == st["total_wait_ms"] and rep["count"][-1] == st["jobs_count"], case


def test_the_wrong_restatements_are_told_apart():
    rng = np.random.default_rng(0x57524F4E)
    gate = skip = 0
    for case in range(60):
        fc, fm, arr, dur, cores, mem = small_system(rng, J=120)
        node, start, fin, st = O.delay_run(fc, fm, arr, dur, cores, mem, max_wait_s=10)
        T = int(st["t_end"])
        rep = R.replay(arr, start, 10, T)
        gate += int((R.replay_no_gate(arr, start, 10, T)["total_ms"] != rep["total_ms"]).any())
        skip += int((R.replay_no_skip(arr, start, 10, T)["total_ms"] != rep["total_ms"]).any())
    assert gate > 30 and skip > 30


def wait_kats():
    with open(os.path.join(GOLDEN, "kats_wait_series.json")) as f:
        series = json.load(f)["series"]
    with open(os.path.join(GOLDEN, "kats_delay.json")) as f:
        dkats = {k["name"]: k for k in json.load(f)["delay"]}
    return [(s, s if "jobs" in s else dkats[s["name"]]) for s in series]


@pytest.mark.parametrize("series,kat", wait_kats(), ids=lambda x: x.get("name"))
def test_hand_traced_series(series, kat):
    arrays, streams = pack_clusters([kat_cluster(kat)]), kat_streams(kat)
    node, start, fin, st = O.delay_run_batch(arrays, streams)
    en, es, ef = kat_expect(kat)
    assert (node == en).all() and (start == es).all() and (fin == ef).all()
    T = len(series["total_s"]) - 1
    assert T > int(st["t_end"][0])
    want = 1000 * np.array(series["total_s"], np.int64)
    rep = R.replay(streams.arrival, start, 10, T)
    assert rep["total_ms"].tolist() == want.tolist()
    assert rep["count"].tolist() == series["count"]
    assert [list(s) for s in rep["skips"]] == series["skips"]
    assert rep["longest_skip_run"] == series["longest_skip_run"]
    assert want[int(st["t_end"][0])] == st["total_wait_ms"][0]
    free = [(n.CoresAvailable, n.MemoryAvailable) for n in kat_cluster(kat).Nodes]
    lit = R.literal(free, (streams.arrival, streams.dur, streams.cores, streams.mem), 10, T)
    assert lit["total_ms"].tolist() == want.tolist() and (lit["start"] == start).all()
    if series["skips"]:  # the restatement without the D6 skip misses these
        assert (R.replay_no_skip(streams.arrival, start, 10, T)["total_ms"] != want).any()
    assert (R.replay_no_gate(streams.arrival, start, 10, T)["total_ms"] != want).any()


def test_wait_sample_layout_matches_the_header(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mcs.h"', "int main(void) {",
             'printf("%zu %zu %zu %zu\\n", sizeof(mcs_wait_sample), offsetof(mcs_wait_sample, average_wait_time),',
             "       offsetof(mcs_wait_sample, total_wait_ms), offsetof(mcs_wait_sample, jobs_count));",
             "return 0; }"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(REPO, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    s = L.mcs_wait_sample
    assert got == [C.sizeof(s), s.average_wait_time.offset, s.total_wait_ms.offset, s.jobs_count.offset]
    assert got == [24, 0, 8, 16]
    assert WAIT_SAMPLE_DTYPE.itemsize == 24
    assert [WAIT_SAMPLE_DTYPE.fields[f][1] for f in ("average_wait_time", "total_wait_ms", "jobs_count")] == [0, 8, 16]
    assert L.lib().mcs_abi_version() == 7


def test_start_stream_carries_one_average_per_message():
    from mcs_amd import CLUSTER_SAMPLE_DTYPE, CLUSTER_STATE_DTYPE

    row = np.zeros(4, CLUSTER_SAMPLE_DTYPE)
    row["cores_utilization"] = [0.0, 0.25, 0.5, 0.125]
    first = np.zeros(1, CLUSTER_STATE_DTYPE)[0]
    first["total_cpu"], first["total_memory"] = 160, 120000
    waits = np.array([0.0, 1000.0 / 3.0, 2500.5, 1e9 / 7.0])
    msgs = wire.start_stream(row, first, waits)
    assert [m.average_wait_time for m in msgs] == waits.tolist()
    assert [wire.unmarshal(wire.ClusterState, wire.marshal(m)).average_wait_time for m in msgs] == waits.tolist()
    assert msgs[0].total_cpu == 160 and all(m.total_cpu is None for m in msgs[1:])
    # a scalar is carried by every message, as before
    same = wire.start_stream(row, first, 12.5)
    assert [wire.marshal(m) for m in same] == [wire.marshal(m) for m in wire.start_stream(row, first, [12.5] * 4)]
    assert [wire.marshal(m) for m in wire.start_stream(row, first)] == \
        [wire.marshal(m) for m in wire.start_stream(row, first, np.zeros(4))]
    with pytest.raises(ValueError):
        wire.start_stream(row, first, waits[:3])
