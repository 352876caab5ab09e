"""CPU tests of the oracle (oracle/mcs_oracle.c) against the known-answer vectors, plus the
properties that pin the fast-forward restatement to the literal one-second Go loop.

The reference has no tests; these KATs (tests/golden/kats.json) are hand-derived from its source
(SURVEY Appendix B).  No GPU needed.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

import oracle_ref as O
import util_ref as U
from kat_util import GOLDEN, kat_cluster, kat_expect, kat_streams, load_kats, seeded_workload
from mcs_amd import pack_clusters

KATS = load_kats()
with open(os.path.join(GOLDEN, "kats_util.json")) as _f:
    UTIL_KATS = json.load(_f)["resource_utilization"]


@pytest.mark.parametrize("literal", [False, True])
@pytest.mark.parametrize("k", KATS["fifo"], ids=[k["name"] for k in KATS["fifo"]])
def test_oracle_fifo_kats(k, literal):
    cl = pack_clusters([kat_cluster(k)])
    s = kat_streams(k)
    node, st, fi, stats = O.fifo_run(cl.free_c, cl.free_m, s.arrival, s.dur, s.cores, s.mem, literal=literal,
                                     cap_c=cl.cap_c, cap_m=cl.cap_m)
    en, es, ef = kat_expect(k)
    np.testing.assert_array_equal(node, en)
    np.testing.assert_array_equal(st, es)
    np.testing.assert_array_equal(fi, ef)
    assert stats["placed"] == int((en >= 0).sum())


@pytest.mark.parametrize("c", KATS["approve_trade"]["cases"])
def test_oracle_approve_trade(c):
    got = O.approve_trade(c["total_c"], c["total_m"], np.float32(c["cu"]), np.float32(c["mu"]), c["cores"],
                          c["mem"], c["time_ns"], np.float32(c["price"]))
    assert got == c["expect"]


def test_kat6_float32_availability():
    # SURVEY KAT6: util 0.79999995f gives avail 32.000008f (float32 T - T*u, trader.go:149)
    t = np.float32(160.0)
    u = np.float32(0.79999995)
    avail = np.float32(t - np.float32(t * u))
    assert avail == np.float32(32.000008)


@pytest.mark.parametrize("c", KATS["heap_order"]["cases"])
def test_oracle_heap_order(c):
    assert O.heap_order(c["prices"]) == c["expect"]


@pytest.mark.parametrize("c", KATS["allocate_virtual_node"]["cases"])
def test_oracle_allocate_virtual_node(c):
    fc = np.full(5, 32, np.uint64)
    fm = np.full(5, 24000, np.uint64)
    rc, nfc, nfm, foreign = O.allocate_virtual_node(fc, fm, c["req_c"], c["req_m"])
    assert rc == c["expect_rc"]
    assert [list(f) for f in foreign] == c["expect_foreign"]
    assert [int(nfc[0]), int(nfm[0])] == c["expect_free0"]


@pytest.mark.parametrize("c", KATS["contract"]["cases"])
def test_oracle_contract_sizing(c):
    got = O.contract(c["kind"], c["jobs"])
    assert list(got[:3]) == c["expect"][:3]
    assert got[3] == c["expect"][3]


def test_contract_small_no_padding_keeps_time():
    # 20 jobs: no nil padding (trader_server.go:79), the last job's end sets Time when it exceeds
    jobs = [(1, 1, 5)] * 19 + [(1, 1, 9)]
    c, m, t, p = O.contract("small", jobs)
    assert (c, m, t) == (20, 20, 9 * 10**9)


def test_schedule_job_and_lend_strictness():
    fc = np.array([4, 8], np.uint64)
    fm = np.array([100, 200], np.uint64)
    assert O.schedule_job(fc, fm, 4, 100) == 0  # >= (scheduler.go:131)
    assert O.schedule_job(fc, fm, 5, 100) == 1
    assert O.schedule_job(fc, fm, 9, 1) == -1
    assert not O.lend(np.array([4], np.uint64), np.array([100], np.uint64), 4, 99)  # strict > (:197)
    assert O.lend(np.array([5], np.uint64), np.array([101], np.uint64), 4, 100)


def test_resource_utilization_float32_order():
    cap_c = np.full(5, 32, np.uint64)
    cap_m = np.full(5, 24000, np.uint64)
    free_c = np.array([0, 16, 32, 31, 7], np.uint64)
    free_m = np.array([1, 24000, 12000, 5, 0], np.uint64)
    cu, mu = O.resource_utilization(cap_c, cap_m, free_c, free_m)
    # restated in numpy float32, node order (cluster.go:53-62)
    c = np.float32(0)
    m = np.float32(0)
    for i in range(5):
        c = np.float32(c + np.float32(np.float32(cap_c[i]) - np.float32(free_c[i])))
        m = np.float32(m + np.float32(np.float32(cap_m[i]) - np.float32(free_m[i])))
    assert cu == np.float32(c / np.float32(160))
    assert mu == np.float32(m / np.float32(120000))


def _f32_from_json(v):
    return {"nan": np.float32("nan"), "+inf": np.float32("inf")}[v] if not v.startswith("0x") else \
        np.array([int(v, 16)], np.uint32).view(np.float32)[0]


@pytest.mark.parametrize("k", UTIL_KATS, ids=[k["name"] for k in UTIL_KATS])
def test_resource_utilization_rounding_kats(k):
    """tests/golden/kats_util.json, derived by hand from cluster.go:46-63 with float32 = 24-bit
    significand, round to nearest even (odd integers in (2^24, 2^25) are ties between their even
    neighbours; the one whose half is even wins):
      order                 0 + 2^24 = 2^24; 2^24 + 1 is a tie -> 2^24 (even significand), twice.  Reversed
                            1 + 1 = 2, 2 + 2^24 = 2^24 + 2 exactly; so does the integer sum.  Divisor
                            float32(2^24 + 2) is exact; 2^24 / (2^24 + 2) = 1 - 2^-23 + O(2^-46) -> 1 - 2^-23.
      convert before sub.   float32(2^24 + 1) = 2^24 (tie, down to even); 2^24 - 1 = 16777215 exactly.
                            Subtracting in integers first gives 2^24.  16777215 / 2^24 = 1 - 2^-24 exactly.
      conversion ties       2^24 + 1 -> 2^24 (2^23 is even); 2^24 + 3 lies between 2^24 + 2 = 2 (2^23 + 1)
                            and 2^24 + 4 = 2 (2^23 + 2): up to the even one.  Sum and divisor convert alike: 1.0.
      total wraps to small  2^31 + 2^31 + 5 = 5 mod 2^32; terms 0, 0, 3; 3.0f / 5.0f = 0.6f = 0x3F19999A.
      total wraps to 0      4 * 2^30 = 0 mod 2^32: 2^30 / 0.0f = +Inf when a node is in use, 0 / 0 = NaN idle.
      empty cluster         no term, total 0: 0 / 0 = NaN.
    Every case is checked on both columns, against the oracle and the numpy restatement."""
    cap, free = np.array(k["cap"], np.uint64), np.array(k["free"], np.uint64)
    want = _f32_from_json(k["util"])
    assert U.total_u32(cap) == k["total"]
    assert U.serial_sum(cap, free) == np.float32(k["sum"]) and float(np.float32(k["sum"])) == k["sum"]
    assert U.same(U.utilization(cap, free), want)
    # the oracle's sum alone (a divisor of 1), then its utilization over the wrapping uint32 total
    cu, mu = C.c_float(), C.c_float()
    p = [np.ascontiguousarray(x).ctypes.data_as(O.u64p) for x in (cap, cap, free, free)]
    O.lib().or_resource_utilization(len(cap), *p, 1, 1, C.byref(cu), C.byref(mu))
    assert cu.value == k["sum"] and mu.value == k["sum"]
    cu, mu = O.resource_utilization(cap, cap, free, free)
    assert U.same(np.float32(cu), want) and U.same(np.float32(mu), want), (cu, mu, want)
    if k["name"] == "order":
        w = U.wrong_sums(cap, free)
        assert w["reversed"] == 16777218 and w["integer"] == 16777218
    if k["name"] == "convert_before_subtracting":
        assert U.wrong_sums(cap, free)["integer"] == 16777216


def w32_clusters(n=200, seed=0x7532):
    rng = np.random.default_rng(seed)
    return [U.w32_cluster(rng) for _ in range(n)]


def test_resource_utilization_equals_numpy_restatement_where_sums_round():
    """200 clusters of the 'w32' fuzz range: the memory sums pass 2^24, so every addition rounds."""
    rounded = 0
    for cap_c, cap_m, free_c, free_m in w32_clusters():
        cu, mu = O.resource_utilization(cap_c, cap_m, free_c, free_m)
        wc, wm = U.resource_utilization(cap_c, cap_m, free_c, free_m)
        assert U.same(np.float32(cu), wc) and U.same(np.float32(mu), wm), (cu, wc, mu, wm)
        rounded += float(U.serial_sum(cap_m, free_m)) != float(sum(int(c) - int(f) for c, f in zip(cap_m, free_m)))
    assert rounded >= 100, rounded


def test_wrong_sums_differ_from_the_serial_sum():
    """The inputs above tell the Go sum from each wrong method in at least half of the clusters."""
    differ = {}
    for cap_c, cap_m, free_c, free_m in w32_clusters():
        for name, d in U.discriminates(cap_m, free_m).items():
            differ[name] = differ.get(name, 0) + d
    assert sorted(differ) == ["float64", "integer", "reversed", "tree"]
    assert min(differ.values()) >= 100, differ


@pytest.mark.parametrize("kind,jobs", [("small", 600), ("big", 600), ("n64", 400), ("n64_hot", 400)])
def test_fast_forward_equals_literal_loop(kind, jobs):
    """Appendix A.3: the fast-forwarded oracle equals the literal 1-second Go loop."""
    arrays, streams, _ = seeded_workload(kind, 3, jobs, seed=1234)
    for k in range(arrays.n_clusters):
        ns = arrays.nodes_of(k)
        js = streams.of(k)
        args = (arrays.free_c[ns], arrays.free_m[ns], streams.arrival[js], streams.dur[js], streams.cores[js],
                streams.mem[js])
        a = O.fifo_run(*args, literal=False)
        b = O.fifo_run(*args, literal=True)
        for x, y in zip(a[:3], b[:3]):
            np.testing.assert_array_equal(x, y)
        for key in ("t_end", "placed", "waited", "peak_running", "flags"):
            assert a[3][key] == b[3][key], key
        assert a[3]["ticks"] <= b[3]["ticks"]


@pytest.mark.parametrize("kind", ["small", "big", "n256"])
def test_oracle_properties(kind):
    """Conservation and FIFO order: every job placed, starts non-decreasing in job order (strict
    head-of-line blocking), start >= arrival, finish = start + dur, and the resources held at every
    instant fit every node."""
    arrays, streams, _ = seeded_workload(kind, 2, 500, seed=99)
    node, st, fi, sd = O.fifo_run_batch(arrays, streams)
    assert (node >= 0).all()
    np.testing.assert_array_equal(fi, st + streams.dur)
    assert (st >= streams.arrival).all()
    for k in range(arrays.n_clusters):
        js = streams.of(k)
        assert (np.diff(st[js].astype(np.int64)) >= 0).all()
        ns = arrays.nodes_of(k)
        cap_c = arrays.free_c[ns].astype(np.int64)
        cap_m = arrays.free_m[ns].astype(np.int64)
        # sweep events: usage at each start instant (after releases due then) must fit
        ev_t = np.concatenate([st[js], fi[js]])
        order = np.lexsort((np.r_[np.ones(len(st[js])), np.zeros(len(fi[js]))], ev_t))
        use_c = np.zeros_like(cap_c)
        use_m = np.zeros_like(cap_m)
        nd = np.r_[node[js], node[js]]
        cc = np.r_[streams.cores[js], -streams.cores[js].astype(np.int64)]
        mm = np.r_[streams.mem[js], -streams.mem[js].astype(np.int64)]
        for i in order:
            use_c[nd[i]] += cc[i]
            use_m[nd[i]] += mm[i]
            assert (use_c <= cap_c).all() and (use_m <= cap_m).all()


def test_oracle_batch_matches_single():
    arrays, streams, _ = seeded_workload("small", 4, 300, seed=5)
    bn, bs, bf, sd = O.fifo_run_batch(arrays, streams, n_threads=2)
    for k in range(4):
        ns, js = arrays.nodes_of(k), streams.of(k)
        n, s, f, st = O.fifo_run(arrays.free_c[ns], arrays.free_m[ns], streams.arrival[js], streams.dur[js],
                                 streams.cores[js], streams.mem[js])
        np.testing.assert_array_equal(bn[js], n)
        np.testing.assert_array_equal(bs[js], s)
        assert sd[k]["t_end"] == st["t_end"]
