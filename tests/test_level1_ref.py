"""CPU tests that pin tests/level1_ref.py — the per-second Level1 reference the GPU tests of
mcs_level1_series compare against — to the oracle, independently of any kernel: the two contract
sizings, the DELAY run's Level1 statistics, every contract a trading run logs, the truncation that
online sessions rely on, the membership rule the kernels use, and the coverage conditions of the GPU
tests' seeds; and the host-side pieces of the feature (struct layout, exported symbols)."""
import ctypes as C
import os
import subprocess

import numpy as np

import level1_cases as K
import level1_ref as R
import oracle_ref as O
from kat_util import REPO, seeded_workload
from mcs_amd import LEVEL1_SAMPLE_DTYPE
from mcs_amd import _lib as L

TIME_NONE = 0xFFFFFFFF


def small_system(rng, J=None):
    """1-3 nodes of 8 cores / 32 memory, a hot stream: gaps 0-2, durations 0-40, requests up to a node,
    now and then one that fits no node."""
    nn = int(rng.integers(1, 4))
    J = int(rng.integers(5, 121)) if J is None else J
    fc, fm = np.full(nn, 8, np.uint32), np.full(nn, 32, np.uint32)
    arr = np.cumsum(rng.integers(0, 3, J)).astype(np.uint32)
    dur = rng.integers(0, 41, J).astype(np.uint32)
    cores, mem = rng.integers(0, 9, J).astype(np.uint32), rng.integers(0, 33, J).astype(np.uint32)
    if rng.random() < 0.3:
        cores[int(rng.integers(0, J))] = 9
    return fc, fm, arr, dur, cores, mem


def test_sizing_equals_the_oracle_contracts():
    rng = np.random.default_rng(0x53495A45)
    lengths = [0, 1, 19, 20, 21, 39, 40, 60] + [int(x) for x in rng.integers(0, 90, 120)]
    nonzero_small = zero_small_at_20 = 0
    for n in lengths:
        for big in (False, True):
            hi = 1 << 31 if big else 40  # sums that wrap in uint32 / int32; every request below 2^31
            jobs = [(int(rng.integers(0, hi)), int(rng.integers(0, hi)), int(rng.integers(0, 12))) for _ in range(n)]
            for kind, fn in (("fast", R.contract_fast), ("small", R.contract_small)):
                oc, om, ot, op = O.contract(kind, jobs)
                assert ot % 1000000000 == 0 and op == 0.0
                assert fn(jobs) == (oc, om, ot // 1000000000), (kind, n, big)
            st = R.contract_small(jobs)[2]
            assert st == 0 or (n > 0 and n % 20 == 0)  # a padding job resets the time
            nonzero_small += st != 0
            zero_small_at_20 += n > 0 and n % 20 == 0 and st == 0
    assert nonzero_small >= 3 and zero_small_at_20 >= 3


def test_replay_equals_the_delay_run_statistics():
    rng = np.random.default_rng(0x4C315354)
    moved = left = 0
    for case in range(120):
        fc, fm, arr, dur, cores, mem = small_system(rng)
        W = (1, 10)[case % 2]
        node, start, fin, st = O.delay_run(fc, fm, arr, dur, cores, mem, max_wait_s=W)
        t_end = int(st["t_end"])
        rep = R.replay(arr, start, W, t_end + 3)
        lens = [len(x) for x in rep["lists"]]
        assert lens[t_end] == st["l1_left"], case
        assert max(lens) == st["peak_l1"], case
        assert len(set(rep["moved"])) == len(rep["moved"]) == st["moved_l1"], case
        assert R.steady_after(rep, arr, start) and lens[-1] == st["l1_left"]
        # the rule the kernels use: Level1(t) = { j : m_j <= t < s_j } in stream order, m non-decreasing
        m, s = R.closed_form(arr, start, W)
        assert (np.diff(m) >= 0).all(), case
        heads = [x[0] for x in rep["lists"] if x]
        assert heads == sorted(heads), case
        for t, members in enumerate(rep["lists"]):
            assert list(members) == np.nonzero((m <= t) & (t < s))[0].tolist(), (case, t)
        moved += int(st["moved_l1"])
        left += int(st["l1_left"])
    assert moved > 1000 and left > 10


def trading_system():
    """A small seeded DELAY trading system whose traders log contracts of both policies."""
    arrays, streams, _ = seeded_workload("small", 8, 300)
    return arrays, streams


def contracts_equal_samples(trades, sample_at):
    """Every logged contract equals the sample at its (t, requester): fast fields for policy 0, small
    fields for policy 1.  Returns the contracts with cores > 0 per policy."""
    seen = {0: 0, 1: 0}
    for tr in trades:
        s = sample_at(int(tr["requester"]), int(tr["t"]))
        time_s = s["fast_time_s"] if tr["policy"] == 0 else s["small_time_s"]
        assert (int(tr["cores"]), int(tr["mem"]), int(tr["time_s"])) == (int(s["cores"]), int(s["mem"]), int(time_s)), tr
        seen[int(tr["policy"])] += int(tr["cores"] > 0)
    return seen


def test_logged_contracts_equal_the_reference_at_their_second():
    arrays, streams = trading_system()
    o = O.dtrade_run(arrays, streams)
    assert len(o["trades"]) == o["n_trades"] > 0
    start = np.where(o["node"] >= 0, o["start"], TIME_NONE)
    ref = K.Ref(streams, start, 10)
    T = int(o["trades"]["t"].max())

    def sample_at(c, t):
        js = streams.of(c)
        return R.series(ref.replay(c, T), streams.dur[js], streams.cores[js], streams.mem[js], t, 1, 1)[0]

    seen = contracts_equal_samples(o["trades"], sample_at)
    assert seen[0] > 0 and seen[1] > 0, seen


def test_truncation_leaves_the_seconds_below_the_horizon_unchanged():
    rng = np.random.default_rng(0x5452554E)
    checked = 0
    for case in range(40):
        fc, fm, arr, dur, cores, mem = small_system(rng, J=int(rng.integers(40, 121)))
        W = (1, 10)[case % 2]
        node, start, fin, st = O.delay_run(fc, fm, arr, dur, cores, mem, max_wait_s=W)
        start = np.where(node >= 0, start, TIME_NONE)
        t_end = int(st["t_end"])
        full = R.replay(arr, start, W, t_end)
        for h in sorted({max(1, t_end // 5), max(2, t_end // 2), max(3, (4 * t_end) // 5)}):
            keep = arr < h  # the jobs the session has received when mcs_run(h) returns
            cut = np.where(start[keep] < h, start[keep], TIME_NONE)  # a start at or past h is undecided
            if not ((cut == TIME_NONE) & (arr[keep] < h)).any():
                continue
            checked += 1
            part = R.replay(arr[keep], cut, W, h - 1)
            assert part["lists"] == full["lists"][:h], (case, h)
    assert checked > 40


def test_gpu_test_seeds_meet_their_coverage_conditions():
    """The systems tests/test_gpu_level1_series.py runs, checked on the oracle's placements."""
    arrays, streams = K.hot_five_nodes()
    for W in (10, 1):
        node, start, fin, st = O.delay_run_batch(arrays, streams, n_threads=4, max_wait_s=W)
        assert (node >= 0).all()
        T = int(st["t_end"].max()) + 6
        K.assert_coverage(K.Ref(streams, start, W).want(0, 1, T + 1))
    arrays, streams = K.rounds_system()
    node, start, fin, st = O.delay_run_batch(arrays, streams, n_threads=4, max_wait_s=10)
    T = int(st["t_end"].max()) + 9
    ref = K.Ref(streams, start, 10)
    want = ref.want(0, 1, T + 1)
    assert (want["len"].max(axis=1) > 20).all()
    straddles = [c for c in range(4) for t in range(T + 1)
                 if (m := ref.members(c, t, T)) and m[0] // 256 != m[-1] // 256]
    assert set(straddles) >= {2, 3}, "no Level1 window across a 256-job batch boundary"
    arrays, streams = K.deadlock_system()
    node, start, fin, st = O.delay_run_batch(arrays, streams, n_threads=1, max_wait_s=10)
    assert st["flags"].tolist() == [1, 0, 0] and st["l1_left"].tolist() == [14, 0, 0] and st["moved_l1"][K.CALM] == 0
    js = streams.of(K.DEAD)
    assert int(streams.mem[js][node[js] < 0].astype(np.uint64).sum()) == 14 << 30 > 1 << 32


def test_level1_sample_layout_matches_the_header(tmp_path):
    fields = ("len", "cores", "mem", "fast_time_s", "small_time_s", "head")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mcs.h"', "int main(void) {",
             'printf("%zu", sizeof(mcs_level1_sample));'] + \
            [f'printf(" %zu", offsetof(mcs_level1_sample, {f}));' for f in fields] + ["return 0; }"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(REPO, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    s = L.mcs_level1_sample
    assert got == [C.sizeof(s)] + [getattr(s, f).offset for f in fields] == [24, 0, 4, 8, 12, 16, 20]
    assert LEVEL1_SAMPLE_DTYPE == R.LEVEL1 and LEVEL1_SAMPLE_DTYPE.itemsize == 24
    assert [LEVEL1_SAMPLE_DTYPE.fields[f][1] for f in fields] == got[1:]
    lib = L.lib()
    assert lib.mcs_abi_version() == 7
    null = C.POINTER(L.mcs_level1_sample)()
    assert lib.mcs_level1_series(None, 0, 1, 1, null, 0, None) == L.MCS_E_INVALID
    assert lib.mcs_online_level1_series(None, 0, 1, 1, null, 0, None) == L.MCS_E_INVALID
    assert lib.mcs_read_level1(None, 0, 0, None, 0, None) == L.MCS_E_INVALID
