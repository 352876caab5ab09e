"""CPU checks of the host reference of the ClusterState series after a FIFO trading run
(trade_series_ref, tests/test_gpu_trade_state.py): on the hand-built borrow system it gives the
written answers of tests/golden/kats_trade_state.json, and with borrow and trader off it is the plain
reference series_ref over the FIFO oracle's placements."""
import numpy as np

import oracle_ref as O
from kat_util import seeded_workload
from test_gpu_state_series import assert_samples_equal, series_ref
from test_gpu_trade_state import kat_expected, load_state_kat, local_lent_rows, oracle_trade, parity_conditions, \
    trade_series_ref, workload_p
from test_trade_oracle import kat_inputs


def test_reference_gives_the_written_answers():
    k = load_state_kat()
    arrays, streams = kat_inputs(k)
    o = oracle_trade(arrays, streams, borrow=bool(k["borrow"]), trader=bool(k["trader"]))
    e = k["expect"]
    assert o["node"].tolist() == e["node"] and o["start"].tolist() == e["start"] and o["finish"].tolist() == e["finish"]
    assert local_lent_rows(o, streams) == sorted(e["lent"])
    want = kat_expected(k)
    assert_samples_equal(trade_series_ref(arrays, streams, o, 0, 1, want.shape[1]), want)
    # cluster 1's utilization and running rise at the lent start and fall at its finish
    assert want["running"][1, 6:12].tolist() == [0, 1, 1, 1, 1, 0]
    assert want["cores_utilization"][1, 6:12].tolist() == [0.0, 0.75, 0.75, 0.75, 0.75, 0.0]
    # cluster 0's queue drops at the borrow tick
    assert want["queued"][0, 4:8].tolist() == [1, 1, 0, 0]


def test_reference_without_trading_is_the_plain_reference():
    arrays, streams, _ = seeded_workload("n64_hot", 3, 200)
    node, start, fin = O.fifo_run_batch(arrays, streams)[:3]
    o = oracle_trade(arrays, streams, borrow=False, trader=False)
    assert np.array_equal(o["node"], node) and np.array_equal(o["start"], start) and np.array_equal(o["finish"], fin)
    assert len(o["lent"]) == 0
    n = int(fin[node >= 0].max()) // 4 + 5
    assert_samples_equal(trade_series_ref(arrays, streams, o, 0, 4, n), series_ref(arrays, streams, node, start, fin, 0, 4, n))


def test_parity_workload_tells_the_record_from_its_wrong_readings():
    """The conditions of the GPU parity test hold on the oracle alone."""
    arrays, streams = workload_p()
    o = oracle_trade(arrays, streams)
    parity_conditions(arrays, streams, o, int(o["t_final"]) + 6)
